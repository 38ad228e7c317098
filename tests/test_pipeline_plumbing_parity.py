"""Argument plumbing of the pipeline mirror against the reference pipeline (chattts_plus/pipelines/chattts_plus_pipeline.py): `_infer_code`
(:157-235), `_refine_text` (:237-277) and the text preamble + slicing of `_infer` (:349-416).  The pipeline is built without models
(`object.__new__`) around a recording stand-in for the GPT and a tiny BERT vocabulary; what it hands to `tokenizer.encode`, `gpt(...)` and
`gpt.generate(...)` must be identical to what the imported reference pipeline handed the same stand-in, recorded in
tests/golden/pipeline_plumbing.json (oracle/make_golden_plumbing.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from chatttsplus_amd import codec, text_frontend
from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, RefineTextParams
from chatttsplus_amd.tokenizer import Tokenizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[Stts]", "[Ptts]", "[spk_emb]", "[empty_spk]", "[uv_break]", "[break_0]", "[Ebreak]",
         "[speed_5]", "[speed_3]", "[laugh]", "[Sbreak]", "[Pbreak]", "[oral_2]", "a", "b", "c", "d", "two", "and", "你", "好", "，", "。"]


class RecordingGPT:
    """Stands in for models_dict["gpt"] on both sides: remembers every call."""
    num_vq = 4
    max_batch = 4

    def __init__(self):
        self.emb_code = [types.SimpleNamespace(num_embeddings=626)]
        self.calls = []

    def __call__(self, input_ids, text_mask, **kw):
        self.calls.append(("embed", input_ids.clone(), text_mask.clone()))
        return torch.zeros(input_ids.shape[0], input_ids.shape[1], 768)

    def generate(self, emb, inputs_ids, **kw):
        rec = dict(kw)
        rec["temperature"] = [round(float(t), 6) for t in kw["temperature"]]
        rec["attention_mask"] = kw["attention_mask"].tolist()
        for key in ("logits_warpers", "logits_processors"):
            rec[key] = [sorted((a, round(float(getattr(o, a)), 6)) for a in ("top_p", "top_k", "min_tokens_to_keep", "penalty", "past_window", "max_input_ids")
                               if hasattr(o, a)) for o in kw[key]]
        rec.pop("context", None)
        self.calls.append(("generate", tuple(emb.shape), inputs_ids.clone(), rec))
        B = emb.shape[0]
        out = types.SimpleNamespace(ids=[torch.tensor([18, 19, 10, 20]) for _ in range(B)], hiddens=[torch.zeros(1, 768)] * B, attentions=[])
        return iter([out])


def _bert(tmp_path):
    from transformers import BertTokenizerFast
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB), encoding="utf-8")
    bt = BertTokenizerFast(vocab_file=str(tmp_path / "vocab.txt"), do_lower_case=False)
    bt.add_special_tokens({"additional_special_tokens": [v for v in VOCAB if v.startswith("[") and v not in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")]})
    return bt


def homophones_map(tmp_path):
    hmap = tmp_path / "homophones_map.json"
    hmap.write_text('{"粘": "年"}', encoding="utf-8")
    return str(hmap)


def encode_calls(calls):
    """The recorded calls as JSON values: tensors as {"tensor": nested list}, tuples as lists."""
    def enc(x):
        if isinstance(x, torch.Tensor):
            return {"tensor": x.tolist()}
        if isinstance(x, (list, tuple)):
            return [enc(v) for v in x]
        if isinstance(x, dict):
            return {k: enc(v) for k, v in x.items()}
        return x
    return json.loads(json.dumps(enc(calls), ensure_ascii=False))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "pipeline_plumbing.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture()
def mine(tmp_path):
    bt = _bert(tmp_path)
    pipe = object.__new__(ChatTTSPlusPipeline)
    pipe.logger = __import__("logging").getLogger("mine")
    pipe.device = torch.device("cpu")
    pipe.models_dict = {"gpt": RecordingGPT(), "tokenizer": Tokenizer(tokenizer=bt)}
    pipe.normalizer = text_frontend.Normalizer(homophones_map(tmp_path))
    pipe.text_splitter = lambda lines: text_frontend.split_text(lines, zh_reader=lambda s: s)   # the minting stand-in of zh_normalization passes text through
    pipe._gpt_for_lora = lambda path: pipe.models_dict["gpt"]
    pipe._decode_to_wavs = lambda hiddens, use_decoder: [torch.zeros(256)] * len(hiddens)
    return pipe


def _same_calls(want, got):
    got = encode_calls(got)
    assert len(want) == len(got) and [c[0] for c in want] == [c[0] for c in got]
    assert sum(c[0] == "generate" for c in want) >= 1
    for x, y in zip(want, got):
        if x[0] == "embed":
            assert x[1] == y[1] and x[2] == y[2]
        else:
            assert x[1] == y[1] and x[2] == y[2]
            assert x[3] == y[3], (x[3], y[3])


PROMPT = codec.encode_prompt((torch.arange(4 * 5).reshape(4, 5) * 7 % 626).to(torch.int32))
INFER_CODE_PARAMS = [
    dict(),
    dict(spk_emb="anything", temperature=[0.2, 0.3, 0.4, 0.5], top_P=0.9, top_K=8, repetition_penalty=1.2, max_new_token=77, min_new_token=3),
    dict(prompt="[speed_3]", txt_smp="a b", spk_smp=PROMPT, ensure_non_empty=False, stream_batch=5, show_tqdm=False),
    dict(prompt="", spk_emb="x", temperature=0.0003),
]
INFER_CODE_TEXT = ["a b c [uv_break]", "[Stts][spk_emb]d d[Ptts] [uv_break]", " 你 好 ， a"]
REFINE_TEXT_PARAMS = [dict(), dict(prompt="[oral_2]", temperature=0.5, top_P=0.8, top_K=10, max_new_token=33, min_new_token=1, show_tqdm=False)]
REFINE_TEXT = ["a b c", "你 好 ， d"]
INFER_FLAGS = [
    dict(),
    dict(do_text_optimization=False),
    dict(do_text_normalization=False, do_homophone_replacement=False),
    dict(lang="zh"),
    dict(skip_refine_text=False),
    dict(skip_refine_text=False, refine_text_only=True),
]
INFER_TEXT = ["a b 2 c\nd and (b)!", "粘 好 ， 你", ("c d a b, " * 30).strip(), "a", "b [laugh] c", "d d d d d d d d d d d d d d d d d d d d d d d d d d d d d d"]
E2E_TEXTS = ["a b c d a b", "c a"]
E2E_SEED = 11


@pytest.mark.parametrize("params", INFER_CODE_PARAMS)
def test_infer_code_hands_the_generator_the_same_arguments(mine, recorded, params):
    mine._infer_code(list(INFER_CODE_TEXT), False, True, InferCodeParams(**params))
    _same_calls(recorded[f"infer_code/{INFER_CODE_PARAMS.index(params)}"]["calls"], mine.models_dict["gpt"].calls)


@pytest.mark.parametrize("params", REFINE_TEXT_PARAMS)
def test_refine_text_hands_the_generator_the_same_arguments(mine, recorded, params):
    mine._refine_text(list(REFINE_TEXT), RefineTextParams(**params))
    _same_calls(recorded[f"refine_text/{REFINE_TEXT_PARAMS.index(params)}"]["calls"], mine.models_dict["gpt"].calls)


@pytest.mark.parametrize("flags", INFER_FLAGS)
def test_infer_preamble_and_slicing_match(mine, recorded, flags):
    """Text optimisation (split, number spelling, short-sentence merge), Normalizer, slices of 4, the refine-text round trip through the
    tokenizer, the '[uv_break]' suffix: the sequence of embed / generate calls is identical."""
    want = recorded[f"infer/{INFER_FLAGS.index(flags)}"]
    kw = dict(skip_refine_text=True)
    kw.update(flags)
    out_mine = list(mine._infer(list(INFER_TEXT), params_refine_text=RefineTextParams(show_tqdm=False), params_infer_code=InferCodeParams(show_tqdm=False),
                                slice_size=4, **kw))
    _same_calls(want["calls"], mine.models_dict["gpt"].calls)
    assert want["n_out"] == len(out_mine)
    if flags.get("refine_text_only"):
        assert want["out"] == json.loads(json.dumps(out_mine, ensure_ascii=False))


def test_reference_pipeline_end_to_end_equals_the_oracle_chain(tmp_path):
    """The reference pipeline's own `_infer` (text wrapping -> tokenizer -> GPT.generate -> per-utterance DVAE -> Vocos) with the reference's
    real GPT and DVAE modules on synthetic weights (its waveforms recorded in tests/golden/pipeline_e2e_ref.npz), against the chain the GPU
    test compares the HIP pipeline with (tests/test_gpu_pipeline.py::test_pipeline_infer_matches_oracle_chain): tokenizer.encode -> OracleGPT ->
    ref_cpu.dvae_decode -> ref_cpu.vocos_decode.  Vocos is absent from the image: both sides vocode with the oracle's restatement, so the
    waveform comparison pins everything up to the mel plus the per-utterance loop, not Vocos itself."""
    from chatttsplus_amd import synth
    from oracle import ref_cpu
    rec = np.load(os.path.join(GOLDEN, "pipeline_e2e_ref.npz"))
    assert sorted(rec.files) == ["wav0", "wav1"]
    gsd = synth.gpt_state_dict(synth.GPT_REAL, 1234)
    dsd = synth.dvae_state_dict(synth.DVAE_REAL, 1234)
    vsd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    spk = torch.load(os.path.join(GOLDEN, "speakers", "2222.pt"), weights_only=True)
    mine_tok = Tokenizer(tokenizer=_bert(tmp_path))
    wrapped = [f"[Stts][spk_emb][speed_5]{t} [uv_break][Ptts]" for t in E2E_TEXTS]
    ids, att, tm = mine_tok.encode(wrapped, 4)
    o = ref_cpu.OracleGPT(gsd, 12)
    emb = o.apply_spk_emb(o.embed(ids, tm), torch.from_numpy(codec.decode_spk_emb(spk)), ids, mine_tok.spk_emb_ids)
    torch.manual_seed(E2E_SEED)
    gen = o.generate(emb, ids, ref_cpu.SamplerParams(min_new_token=2), attention_mask=att, max_new_token=10)
    for b in range(2):
        n = gen.ids[b].shape[0]
        wav_ref = rec[f"wav{b}"]
        assert wav_ref.shape[0] == 256 * (2 * n - 1)
        wav = ref_cpu.vocos_decode(vsd, ref_cpu.dvae_decode(dsd, gen.hiddens[b])).numpy()
        rms = float(np.sqrt(np.mean((wav - wav_ref) ** 2))) / float(np.sqrt(np.mean(wav_ref ** 2)))
        assert rms <= 5e-4, (b, rms)                           # measured 2e-4: fp32 hiddens differ by ~5e-6, Vocos exponentiates magnitudes
