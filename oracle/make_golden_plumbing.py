"""Mint tests/golden/pipeline_plumbing.json and tests/golden/pipeline_e2e_ref.npz by running the *imported, unmodified* reference pipeline
(chattts_plus/pipelines/chattts_plus_pipeline.py) around the recording stand-ins of tests/test_pipeline_plumbing_parity.py.

TEST INFRASTRUCTURE.  Runs only where the reference tree is present (oracle/ref_import.py):

    python -m oracle.make_golden_plumbing

The reference pipeline is built without models (`object.__new__`) around the test module's RecordingGPT and tiny BERT vocabulary; the
fixture holds what it handed to `gpt(...)` / `gpt.generate(...)` for every case of the test module, and what `_infer` returned.  The
import needs stand-ins for packages the image lacks (tensorrt-backed `trt_models`, `onnx2trt`, numba, zh_normalization) -- none of them
is executed on these paths.  The end-to-end case runs the reference's own `_infer` with its real GPT and DVAE modules on synthetic
weights and stores the waveforms.
"""
from __future__ import annotations

import importlib
import importlib.util
import json
import logging
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import codec  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT, load_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _test_module():
    spec = importlib.util.spec_from_file_location("plumbing_parity", os.path.join(ROOT, "tests", "test_pipeline_plumbing_parity.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build_ref(t, tmp_path):
    """The reference pipeline around t.RecordingGPT and the tiny vocabulary (what the test module's `mine` fixture builds on the product side)."""
    from oracle import make_golden_text as mg
    load_reference()
    mg._install_stand_ins()
    for name, attrs in (("chattts_plus.trt_models", dict(__path__=[])), ("chattts_plus.commons.onnx2trt", dict(convert_onnx_to_trt=lambda *a, **k: None)),
                        ("chattts_plus.pipelines", dict(__path__=[os.path.join(REFERENCE_ROOT, "chattts_plus", "pipelines")]))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    ref_pipe_mod = importlib.import_module("chattts_plus.pipelines.chattts_plus_pipeline")
    ref_tok_mod = importlib.import_module("chattts_plus.models.tokenizer")
    ref_norm_mod = importlib.import_module("chattts_plus.commons.norm")
    bt = t._bert(tmp_path)
    if not hasattr(type(bt), "encode_plus"):                  # transformers 5 dropped the 4.x alias the reference calls (tokenizer.py:70)
        type(bt).encode_plus = lambda self, *a, **k: self(*a, **k)
    ref_tok = object.__new__(ref_tok_mod.Tokenizer)
    ref_tok._tokenizer, ref_tok._decode_prompt = bt, codec.decode_prompt
    ref_tok.spk_emb_ids, ref_tok.break_0_ids, ref_tok.eos_token = (bt.convert_tokens_to_ids(x) for x in ("[spk_emb]", "[break_0]", "[Ebreak]"))
    ref_tok.len = len(bt)
    ref_tok.decode = bt.batch_decode
    ref_tok.apply_spk_emb = lambda emb, spk, ids, dev: emb       # the speaker overwrite is a kernel on the HIP side (ctts_gpt_embed); not plumbing
    ref = object.__new__(ref_pipe_mod.ChatTTSPlusPipeline)
    ref.logger = logging.getLogger("ref")
    ref.device, ref.dtype, ref.infer_type = torch.device("cpu"), torch.float32, "pytorch"
    ref.models_dict = {"gpt": t.RecordingGPT(), "tokenizer": ref_tok}
    ref.normalizer = ref_norm_mod.Normalizer(t.homophones_map(tmp_path))
    ref._decode_to_wavs = lambda hiddens, use_decoder: [torch.zeros(256)] * len(hiddens)
    return ref


def ref_params(cls, kw):
    return getattr(importlib.import_module("chattts_plus.commons.utils"), cls)(**kw)


def record_cases(t):
    out = {}

    def fresh():
        return build_ref(t, Path(tempfile.mkdtemp()))

    for i, params in enumerate(t.INFER_CODE_PARAMS):
        ref = fresh()
        ref._infer_code(list(t.INFER_CODE_TEXT), False, True, ref_params("InferCodeParams", params))
        out[f"infer_code/{i}"] = dict(calls=t.encode_calls(ref.models_dict["gpt"].calls))
    for i, params in enumerate(t.REFINE_TEXT_PARAMS):
        ref = fresh()
        ref._refine_text(list(t.REFINE_TEXT), ref_params("RefineTextParams", params))
        out[f"refine_text/{i}"] = dict(calls=t.encode_calls(ref.models_dict["gpt"].calls))
    for i, flags in enumerate(t.INFER_FLAGS):
        ref = fresh()
        kw = dict(skip_refine_text=True)
        kw.update(flags)
        res = list(ref._infer(list(t.INFER_TEXT), params_refine_text=ref_params("RefineTextParams", dict(show_tqdm=False)),
                              params_infer_code=ref_params("InferCodeParams", dict(show_tqdm=False)), **kw))
        out[f"infer/{i}"] = dict(calls=t.encode_calls(ref.models_dict["gpt"].calls), n_out=len(res),
                                 out=res if flags.get("refine_text_only") else None)
    return out


def record_end_to_end(t):
    """The reference pipeline's own `_infer` (text wrapping -> tokenizer -> GPT.generate -> per-utterance DVAE -> Vocos) with the reference's real
    GPT and DVAE modules on synthetic weights; Vocos is absent from the image and vocodes with the oracle's restatement."""
    from chatttsplus_amd import synth
    from oracle import make_golden as mgold
    from oracle import ref_cpu
    ref = build_ref(t, Path(tempfile.mkdtemp()))
    refmods = load_reference()
    gsd = synth.gpt_state_dict(synth.GPT_REAL, 1234)
    dsd = synth.dvae_state_dict(synth.DVAE_REAL, 1234)
    vsd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    cfg = synth.DVAE_REAL
    dvae = refmods.dvae.DVAE(decoder_config=dict(idim=cfg["idim"], odim=cfg["odim"], hidden=cfg["hidden"], n_layer=cfg["n_layer"], bn_dim=cfg["bn_dim"]),
                             dim=cfg["dim"]).eval()
    dvae.load_state_dict({k: torch.from_numpy(v) for k, v in dsd.items()}, strict=True)

    class OracleVocos:                                         # stand-in for the absent third-party package (pipeline:93-111,303)
        def parameters(self):
            return iter([torch.zeros(1)])

        def decode(self, mel):
            return ref_cpu.vocos_decode(vsd, mel[0])[None]

    tok = ref.models_dict["tokenizer"]
    tok._decode_spk_emb = codec.decode_spk_emb                 # pybase16384 is absent; the codec is pinned on the bundled speaker files
    del tok.apply_spk_emb                                      # the reference's own speaker overwrite runs here
    ref.models_dict = {"gpt": mgold.build_ref_gpt(refmods, synth.GPT_REAL, gsd), "tokenizer": tok, "dvae_decode": dvae, "vocos": OracleVocos()}
    del ref._decode_to_wavs                                    # ... and the reference's own per-utterance loop (pipeline:286-305)
    spk = torch.load(os.path.join(GOLDEN, "speakers", "2222.pt"), weights_only=True)
    params = ref_params("InferCodeParams", dict(prompt="[speed_5]", spk_emb=spk, max_new_token=10, min_new_token=2, show_tqdm=False))
    torch.manual_seed(t.E2E_SEED)
    outs = list(ref._infer(list(t.E2E_TEXTS), False, None, True, False, True, True, False, True, ref_params("RefineTextParams", {}), params))
    assert len(outs) == 1
    return {f"wav{b}": w.numpy().astype(np.float32) for b, w in enumerate(outs[0])}


def main():
    t = _test_module()
    path = os.path.join(GOLDEN, "pipeline_plumbing.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(record_cases(t), f, ensure_ascii=False)
    print("wrote", path)
    path = os.path.join(GOLDEN, "pipeline_e2e_ref.npz")
    np.savez_compressed(path, **record_end_to_end(t))
    print("wrote", path)


if __name__ == "__main__":
    main()
