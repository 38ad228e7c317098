"""Cloned voices per utterance on the GPU: ChatTTSPlusPipeline.clone_voices (all clips through one encoder call), params_per_utterance entries with
spk_smp / txt_smp on infer()'s paths and in a serving session, score(wavs=[...]).  The engine runs under batch_invariant, where an utterance's tokens and
hidden rows do not depend on its batch: every utterance of a mixed batch must be, bit for bit, its own batch-1 run with the voice given the old way
(params_infer_code.spk_smp / txt_smp, or spk_emb) under the same noise key (request seed, utterance id)."""
import os

import numpy as np
import pytest
import torch

from chatttsplus_amd import codec, synth
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[Stts]", "[Ptts]", "[spk_emb]", "[empty_spk]", "[uv_break]", "[break_0]",
         "[Ebreak]", "[speed_5]", "a", "b", "c", "d"]
TEXTS = ["a b c", "c d", "b a d"]
NEW, SEED = 12, 4242


def _tokenizer(tmp_path):
    from transformers import BertTokenizerFast
    from chatttsplus_amd.tokenizer import Tokenizer
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB))
    bt = BertTokenizerFast(vocab_file=str(tmp_path / "vocab.txt"), do_lower_case=False)
    bt.add_special_tokens({"additional_special_tokens": [v for v in VOCAB if v.startswith("[") and v not in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")]})
    return Tokenizer(tokenizer=bt)


def _make_pipe(tmp_path, max_batch=8, max_seq_len=256):
    """ChatTTSPlusPipeline on synthetic checkpoints written to tmp_path (the drop-in path: YAML -> infer_type "hip" -> hip_models), batch-invariant engine."""
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, load_config
    cfg = load_config(os.path.join(os.path.dirname(GOLDEN), "..", "configs", "infer", "chattts_plus_hip.yaml"))
    cfg["MODELS"]["gpt"]["kwargs"].update(weight_dtype="fp32", max_batch=max_batch, max_seq_len=max_seq_len, options={"batch_invariant": 1})
    os.makedirs(tmp_path / "asset")
    gsd = synth.gpt_state_dict(synth.GPT_REAL, 1234)
    dsd = synth.dvae_state_dict(synth.DVAE_REAL, 1234)
    vsd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    esd = synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234)
    esd.update(synth.dvae_full_decoder_state_dict(synth.DVAE_FULL_DEC, 1234))        # DVAE_full.pt = encode side + decode side + quantiser (one coef)
    for name, sd in (("GPT.pt", gsd), ("Decoder.pt", dsd), ("Vocos.pt", vsd), ("DVAE_full.pt", esd)):
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "asset" / name)
    tok = _tokenizer(tmp_path)
    pipe = ChatTTSPlusPipeline(cfg, device="cuda", tokenizer=tok, checkpoint_dir=str(tmp_path))
    return pipe, tok, dict(gpt=gsd, dvae=dsd, vocos=vsd, enc=esd)


def _params(**kw):
    from chatttsplus_amd.pipeline import InferCodeParams
    return InferCodeParams(prompt="[speed_5]", max_new_token=NEW, min_new_token=NEW, show_tqdm=False, **kw)


def _infer(pipe, texts, params, **kw):
    out = list(pipe.infer(list(texts), skip_refine_text=True, do_text_optimization=False, params_infer_code=params, noise="device", noise_seed=SEED, **kw))
    assert len(out) == 1
    return out[0]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The pipeline, two cloned voices and a speaker string, and every utterance's own batch-1 run (waveform and ids) with its voice given the old way --
    computed once, never written."""
    from scipy.io import wavfile
    from chatttsplus_amd import audio
    tmp = tmp_path_factory.mktemp("cloned")
    pipe, tok, _ = _make_pipe(tmp)
    spk = torch.load(os.path.join(GOLDEN, "speakers", "2222.pt"), weights_only=True)
    clip_a = torch.from_numpy(synth.speaker_wave(9, 16000))                          # 16000 samples at 24 kHz, given as a waveform
    clip_b = synth.speaker_wave(10, 20000)                                           # 30000 samples at 24 kHz, given as a 16 kHz stereo file
    wavfile.write(tmp / "b.wav", 16000, np.stack([clip_b, 0.5 * clip_b], 1))
    mono_b = torch.mean(audio.resample(torch.from_numpy(np.stack([clip_b, 0.5 * clip_b], 0)), 16000, 24000), 0)
    assert mono_b.shape[0] == 30000
    smp = [pipe.sample_audio_speaker(clip_a), pipe.sample_audio_speaker(mono_b)]     # the old way, clip by clip
    old = [_params(spk_smp=smp[0], txt_smp="a b"), _params(spk_smp=smp[1], txt_smp="c d a"), _params(spk_emb=spk)]
    ref_wavs, ref_ids = [], []
    for u, (t, p) in enumerate(zip(TEXTS, old)):
        w = _infer(pipe, [t], p, utt_ids=[u])[0]
        d = _infer(pipe, [t], p, utt_ids=[u], return_details=True)
        assert torch.equal(d.wavs[0], w) and w.shape[0] == 256 * (2 * NEW - 1)
        ref_wavs.append(w.clone())
        ref_ids.append(d.ids[0].clone())
    return dict(pipe=pipe, spk=spk, clips=[clip_a, str(tmp / "b.wav")], smp=smp, wavs=ref_wavs, ids=ref_ids)


def _voices(world):
    from chatttsplus_amd.pipeline import ClonedVoice
    return [ClonedVoice(world["smp"][0], "a b"), ClonedVoice(world["smp"][1], "c d a")]


def test_clone_voices_is_sample_audio_speaker_clip_by_clip(world):
    voices = world["pipe"].clone_voices(world["clips"], ["a b", "c d a"])
    assert [v.spk_smp for v in voices] == world["smp"] and [v.txt_smp for v in voices] == ["a b", "c d a"]
    assert [tuple(v.codes.shape) for v in voices] == [(4, 31), (4, 59)]
    assert all(torch.equal(v.codes, codec.decode_prompt(s)) for v, s in zip(voices, world["smp"]))


def test_infer_with_a_voice_per_utterance(world):
    a, b = _voices(world)
    got = _infer(world["pipe"], TEXTS, _params(), params_per_utterance=[a.overrides(), b.overrides(), {"spk_emb": world["spk"]}])
    assert len(got) == 3
    for u in range(3):
        d = float((got[u] - world["wavs"][u]).abs().max()) if got[u].shape == world["wavs"][u].shape else None
        print(f"utterance {u}: max |mixed batch - batch 1| = {d}")
        assert torch.equal(got[u], world["wavs"][u]), f"utterance {u}: not its batch-1 run with the voice given the old way"
    # the same through row re-use (3 utterances over 2 decode rows)
    cont = [w for ws in world["pipe"].infer(list(TEXTS), skip_refine_text=True, do_text_optimization=False, params_infer_code=_params(), noise="device",
                                             noise_seed=SEED, continuous=True, slice_size=2,
                                             params_per_utterance=[a.overrides(), b.overrides(), {"spk_emb": world["spk"]}]) for w in ws]
    assert len(cont) == 3 and all(torch.equal(cont[u], world["wavs"][u]) for u in range(3))


def test_session_with_a_voice_per_utterance(world):
    from chatttsplus_amd.pipeline import SessionChunk
    a, b = _voices(world)
    pipe = world["pipe"]
    with pipe.open_session(_params(spk_emb=world["spk"]), seed=SEED) as ses:
        tks = [ses.submit(TEXTS[0], params=a.overrides(), utt_id=0), ses.submit(TEXTS[1], params=b.overrides(), utt_id=1, stream="exact", stream_batch=4),
               ses.submit(TEXTS[2], params={"spk_emb": world["spk"]}, utt_id=2)]
        out = ses.drain()
    got = {}
    for tk, w, cancelled in out:
        assert not cancelled
        if isinstance(w, SessionChunk):
            assert w.start == sum(int(c.shape[0]) for c in got.get(tk, []))
            got.setdefault(tk, []).append(w.wav)
        else:
            got[tk] = [w]
    for u, tk in enumerate(tks):
        assert torch.equal(torch.cat(got[tk]), world["wavs"][u]), f"utterance {u}"


def test_candidates_of_an_utterance_share_its_voice(world):
    a, b = _voices(world)
    pipe = world["pipe"]
    d = _infer(pipe, TEXTS[:2], _params(), params_per_utterance=[a.overrides(), b.overrides()], num_candidates=2, return_details=True)
    assert pipe.models_dict["gpt"].shared_prompts == [(4, 2)]                       # one prompt pass per utterance, two rows each
    for u in range(2):
        assert len(d.candidates[u]) == 2
        assert torch.equal(d.candidates[u][0].ids.cpu(), world["ids"][u].cpu()), f"utterance {u}: candidate 0 is not the plain run in that voice"


def test_default_mode_mixed_batch_runs(world):
    a, b = _voices(world)
    gpt = world["pipe"].models_dict["gpt"]
    gpt.set_option("batch_invariant", 0)
    try:
        got = _infer(world["pipe"], TEXTS, _params(), params_per_utterance=[a.overrides(), b.overrides(), {"spk_emb": world["spk"]}])
    finally:
        gpt.set_option("batch_invariant", 1)
    assert len(got) == 3
    assert [int(w.shape[0]) for w in got] == [256 * (2 * NEW - 1)] * 3


def test_score_encodes_its_clips_in_one_call(world):
    pipe = world["pipe"]
    enc = pipe.models_dict["dvae_encode"]
    clips = [torch.from_numpy(synth.speaker_wave(100 + n, n)) for n in (6000, 9000, 12800)]
    codes = [enc.encode(c).t().cpu() for c in clips]                                # per clip, the single-clip call: [n, 4]
    assert [int(c.shape[0]) for c in codes] == [12, 18, 25]
    calls = []
    orig = enc.encode_batch
    enc.encode_batch = lambda wavs, **kw: calls.append(len(wavs)) or orig(wavs, **kw)
    try:
        res_w = pipe.score(list(TEXTS), wavs=clips, params_infer_code=_params(spk_emb=world["spk"]))
    finally:
        del enc.encode_batch
    assert calls == [3]
    res_c = pipe.score(list(TEXTS), codes=codes, params_infer_code=_params(spk_emb=world["spk"]))
    assert [int(lp.shape[0]) for lp in res_w.logprob] == [int(c.shape[0]) + 1 for c in codes]      # the targets are the clip's codes + EOS
    for u in range(3):
        assert torch.equal(res_w.logprob[u], res_c.logprob[u]) and torch.equal(res_w.argmax[u], res_c.argmax[u]), u
    assert res_w.loss == res_c.loss and res_w.accuracy == res_c.accuracy


def test_a_voice_that_does_not_fit_is_refused_by_utterance(world):
    from chatttsplus_amd import _lib
    from chatttsplus_amd.pipeline import ClonedVoice
    pipe = world["pipe"]
    long_voice = ClonedVoice(codec.encode_prompt(torch.zeros(4, 250, dtype=torch.int64)), "a")      # 250 codes + text + 12 new tokens > max_seq_len 256
    a, _ = _voices(world)
    with pytest.raises(_lib.HipBackendError, match="utterance 1"):
        _infer(pipe, TEXTS[:2], _params(), params_per_utterance=[a.overrides(), long_voice.overrides()])
    with pipe.open_session(_params(spk_emb=world["spk"]), seed=SEED) as ses:
        with pytest.raises(_lib.HipBackendError, match="utterance 7"):
            ses.submit(TEXTS[0], params=long_voice.overrides(), utt_id=7)
    got = _infer(pipe, TEXTS[:1], _params(), params_per_utterance=[a.overrides()], utt_ids=[0])    # the engine is free and unharmed
    assert torch.equal(got[0], world["wavs"][0])
