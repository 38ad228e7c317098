"""Host side of per-utterance cloned voices (no GPU): the ragged audio-prompt builder of Tokenizer.encode, the spk_smp / txt_smp entries of
per_utterance_overrides, ClonedVoice and the per-row voice table the pipeline's prompt builder reads."""
import dataclasses

import pytest
import torch

from chatttsplus_amd import _lib, codec
from chatttsplus_amd.pipeline import PER_UTTERANCE_FIELDS, ClonedVoice, InferCodeParams, per_utterance_overrides, utterance_voices

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[Stts]", "[Ptts]", "[spk_emb]", "[empty_spk]", "[uv_break]", "[break_0]",
         "[Ebreak]", "[speed_5]", "a", "b", "c", "d"]


def _tokenizer(tmp_path):
    from transformers import BertTokenizerFast
    from chatttsplus_amd.tokenizer import Tokenizer
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB))
    bt = BertTokenizerFast(vocab_file=str(tmp_path / "vocab.txt"), do_lower_case=False)
    bt.add_special_tokens({"additional_special_tokens": [v for v in VOCAB if v.startswith("[") and v not in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")]})
    return Tokenizer(tokenizer=bt)


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return codec.encode_prompt(torch.randint(0, 625, (4, n), generator=g))


TEXTS = ["[Stts][empty_spk]a b[speed_5]a b c d [uv_break][Ptts]", "[Stts][spk_emb][speed_5]c [uv_break][Ptts]", "[Stts][empty_spk]d[speed_5]b a d [uv_break][Ptts]"]


def test_a_list_of_equal_prompt_strings_is_the_single_string(tmp_path):
    tok = _tokenizer(tmp_path)
    p = _prompt(7, 0)
    want = tok.encode(TEXTS, 4, prompt_str=p)
    got = tok.encode(TEXTS, 4, prompt_str=[p, p, p])
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and torch.equal(w, g)
    none = tok.encode(TEXTS, 4, prompt_str=[None, None, None])
    for w, g in zip(tok.encode(TEXTS, 4), none):
        assert w.dtype == g.dtype and torch.equal(w, g)
    with pytest.raises(ValueError):
        tok.encode(TEXTS, 4, prompt_str=[p, p])


def test_ragged_prompts_are_the_batch_1_rows_left_padded(tmp_path):
    tok = _tokenizer(tmp_path)
    prompts = [_prompt(11, 1), None, _prompt(3, 2)]
    ids, att, tm = tok.encode(TEXTS, 4, prompt_str=prompts)
    assert ids.shape[0] == 3 and ids.shape[2] == 4 and att.shape == tm.shape == ids.shape[:2]
    lens = []
    for i, (t, p) in enumerate(zip(TEXTS, prompts)):
        ids1, att1, tm1 = tok.encode([t], 4, prompt_str=p)
        n = ids1.shape[1]
        lens.append(n)
        pad = ids.shape[1] - n
        assert torch.equal(ids[i, pad:], ids1[0]) and torch.equal(att[i, pad:], att1[0]) and torch.equal(tm[i, pad:], tm1[0]), i
        assert ids1.dtype == ids.dtype and att1.dtype == att.dtype and tm1.dtype == tm.dtype
        assert not bool(att[i, :pad].any()) and not bool(tm[i, :pad].any()) and not bool(ids[i, :pad].any())
        n_codes = 0 if p is None else codec.decode_prompt(p).shape[1]
        assert int(att[i].sum()) == n and int(tm[i].sum()) == n - n_codes          # attention over text and codes, text_mask 0 over the codes
        if n_codes:
            assert torch.equal(ids[i, ids.shape[1] - n_codes:], codec.decode_prompt(p).t())
    assert ids.shape[1] == max(lens) and len(set(lens)) == 3


def test_per_utterance_overrides_take_cloned_voices():
    assert "spk_smp" in PER_UTTERANCE_FIELDS and "txt_smp" in PER_UTTERANCE_FIELDS
    base = InferCodeParams(spk_emb="call-speaker")
    pa, pb = _prompt(5, 3), _prompt(9, 4)
    diffs = per_utterance_overrides(base, [{"spk_smp": pa, "txt_smp": "a b", "spk_emb": None}, None, dataclasses.replace(base, spk_smp=pb), {"spk_emb": "other"}])
    assert diffs == [{"spk_smp": pa, "txt_smp": "a b"}, {}, {"spk_smp": pb}, {"spk_emb": "other"}]
    # a cloned row speaks without a speaker vector; the others keep the call's speaker row
    assert utterance_voices(base, diffs) == [("[empty_spk]", "a b", pa), ("[spk_emb]", "", None), ("[empty_spk]", "", pb), ("[spk_emb]", "", None)]
    assert utterance_voices(base, [{}, {"temperature": 0.5}]) is None
    # a call that itself names a cloned voice: rows inherit it, a row may replace the transcript or the clip
    call = InferCodeParams(spk_smp=pa, txt_smp="c")
    assert utterance_voices(call, per_utterance_overrides(call, [None, {"txt_smp": "d"}, {"spk_smp": pb}])) == [
        ("[empty_spk]", "c", pa), ("[empty_spk]", "d", pa), ("[empty_spk]", "c", pb)]
    with pytest.raises(_lib.HipBackendError, match="stream_batch"):
        per_utterance_overrides(base, [{"spk_smp": pa, "stream_batch": 7}])
    with pytest.raises(_lib.HipBackendError, match="spk_smp.*spk_emb"):
        per_utterance_overrides(base, [None, {"spk_smp": pa, "spk_emb": "other"}])


def test_cloned_voice_overrides_round_trip():
    codes = torch.randint(0, 625, (4, 13), generator=torch.Generator().manual_seed(5))
    v = ClonedVoice(spk_smp=codec.encode_prompt(codes), txt_smp="a b c")
    o = v.overrides()
    assert set(o) == {"spk_smp", "txt_smp", "spk_emb"} and o["spk_emb"] is None and o["txt_smp"] == "a b c"
    assert torch.equal(codec.decode_prompt(o["spk_smp"]), codes) and torch.equal(v.codes, codes)
    diff = per_utterance_overrides(InferCodeParams(spk_emb="x"), [o])[0]
    assert diff == {"spk_smp": v.spk_smp, "txt_smp": "a b c"}


def test_code_prompt_builds_every_row_with_its_own_voice(tmp_path):
    """_code_prompt with a voice table: row i is "[Stts]{tag_i}{txt_smp_i}{prompt}{text}[Ptts]" followed by its own codes."""
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    tok = _tokenizer(tmp_path)
    pipe = object.__new__(ChatTTSPlusPipeline)
    pipe.models_dict, pipe.device = {"tokenizer": tok}, torch.device("cpu")

    class G:
        num_vq = 4
    pa, pb = _prompt(5, 3), _prompt(9, 4)
    texts = ["a b c [uv_break]", "c d [uv_break]", "b a d [uv_break]"]
    voices = [("[empty_spk]", "a b", pa), ("[empty_spk]", "", pb), ("[spk_emb]", "", None)]
    ids, att, tm = pipe._code_prompt(list(texts), InferCodeParams(spk_emb="x"), G(), None, voices)
    for i, (t, old) in enumerate(zip(texts, [InferCodeParams(spk_smp=pa, txt_smp="a b"), InferCodeParams(spk_smp=pb), InferCodeParams(spk_emb="x")])):
        ids1, att1, tm1 = pipe._code_prompt([t], old, G())          # the voice given the old way, batch 1
        pad = ids.shape[1] - ids1.shape[1]
        assert torch.equal(ids[i, pad:], ids1[0]) and torch.equal(att[i, pad:], att1[0]) and torch.equal(tm[i, pad:], tm1[0]) and not bool(att[i, :pad].any()), i


class _FakeEncoder:
    """Stands in for DVAEEncoder.encode_batch: clip i -> codes [4, 3 + i]; the clips listed in `bad` carry the encoder's mark of non-finite features, id -1."""

    def __init__(self, bad=()):
        self.bad, self.calls = set(bad), 0

    def encode_batch(self, wavs):
        self.calls += 1
        out = []
        for i, _ in enumerate(wavs):
            c = torch.randint(0, 625, (4, 3 + i), generator=torch.Generator().manual_seed(i), dtype=torch.int32)
            if i in self.bad:
                c[:, 1] = -1
            out.append(c)
        return out


def test_encode_clips_refuses_a_clip_with_negative_codes():
    from chatttsplus_amd.pipeline import encode_clips
    wavs = [torch.zeros(600)] * 3
    clean = encode_clips(_FakeEncoder(), wavs)
    assert [tuple(c.shape) for c in clean] == [(4, 3), (4, 4), (4, 5)] and all(c.dtype == torch.int32 and c.device.type == "cpu" for c in clean)
    assert all(torch.equal(a, b) for a, b in zip(clean, _FakeEncoder().encode_batch(wavs)))
    with pytest.raises(_lib.HipBackendError, match=r"clip 1: 1 of 4 code frames"):
        encode_clips(_FakeEncoder(bad=[1]), wavs)
    with pytest.raises(_lib.HipBackendError, match=r"clip 0"):                    # the first bad clip is the one named
        encode_clips(_FakeEncoder(bad=[0, 2]), wavs)
    one = torch.full((4, 3), 7, dtype=torch.int32)
    one[2, 0] = -1                                                               # a single negative id (one group of one frame) is enough

    class One:
        def encode_batch(self, wavs):
            return [one]
    with pytest.raises(_lib.HipBackendError, match=r"clip 0: 1 of 3"):
        encode_clips(One(), wavs[:1])


def test_every_caller_of_the_clip_encoder_goes_through_the_check():
    """sample_audio_speaker, clone_voices and score(wavs=) refuse a clip whose codes are negative instead of writing it into a prompt string (astype("<u2") would
    turn -1 into 65535) or scoring it."""
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    pipe = object.__new__(ChatTTSPlusPipeline)
    pipe.device = torch.device("cpu")
    good, bad = _FakeEncoder(), _FakeEncoder(bad=[1])
    pipe.models_dict = {"dvae_encode": good}
    s = pipe.sample_audio_speaker(torch.zeros(600))
    assert torch.equal(codec.decode_prompt(s), good.encode_batch([None])[0].to(torch.int64))
    voices = pipe.clone_voices([torch.zeros(600), torch.zeros(700)], ["a", "b"])
    assert [v.codes.shape[1] for v in voices] == [3, 4] and voices[0].spk_smp == s and voices[1].txt_smp == "b"
    assert torch.equal(codec.decode_prompt(voices[1].spk_smp), voices[1].codes)
    pipe.models_dict = {"dvae_encode": bad}
    with pytest.raises(_lib.HipBackendError, match="clip 1"):
        pipe.clone_voices([torch.zeros(600), torch.zeros(700)], ["a", "b"])
    with pytest.raises(_lib.HipBackendError, match="score: waveform 1"):
        pipe.score(["a", "b"], wavs=[torch.zeros(600), torch.zeros(700)])
    pipe.models_dict = {"dvae_encode": _FakeEncoder(bad=[0])}
    with pytest.raises(_lib.HipBackendError, match="clip 0"):
        pipe.sample_audio_speaker(torch.zeros(600))
