"""Mint tests/golden/tokenizer_encode.json by running the *imported, unmodified* reference Tokenizer.encode
(chattts_plus/models/tokenizer.py:49-137) on the cases of tests/test_tokenizer_parity.py.

TEST INFRASTRUCTURE.  Runs only where the reference tree is present (oracle/ref_import.py):

    python -m oracle.make_golden_tokenizer

The reference's __init__ unpickles tokenizer.pt, which is not part of its tree: the object is built with `object.__new__` around the test's tiny
BERT vocabulary.  The audio-prompt string is decoded by this repo's codec (pybase16384 is absent from the image).
"""
from __future__ import annotations

import importlib
import importlib.util
import json
import os
import sys
import tempfile
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import codec  # noqa: E402
from chatttsplus_amd.tokenizer import Tokenizer  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("tokenizer_parity", os.path.join(ROOT, "tests", "test_tokenizer_parity.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    load_reference()
    ref_mod = importlib.import_module("chattts_plus.models.tokenizer")
    bt = t._bert(Path(tempfile.mkdtemp()))
    if not hasattr(type(bt), "encode_plus"):                   # transformers 5 dropped the 4.x alias the reference calls (tokenizer.py:70):
        type(bt).encode_plus = lambda self, *a, **k: self(*a, **k)  # for one text it was the same call as __call__
    ref_tok = object.__new__(ref_mod.Tokenizer)
    ref_tok._tokenizer = bt
    ref_tok._decode_prompt = codec.decode_prompt
    out = []
    for case in t.CASES:
        ids, att, tm = ref_tok.encode(list(case["text"]), 4, t._prompt_string() if case["prompt"] else None, "cpu")
        out.append(dict(ids=ids.tolist(), attention_mask=att.tolist(), text_mask=tm.to(torch.int64).tolist()))
    mine = Tokenizer(tokenizer=bt)
    with open(t.FIX, "w", encoding="utf-8") as f:
        json.dump(dict(vocab=t.VOCAB, cases=out, special=[mine.spk_emb_ids, mine.break_0_ids, mine.eos_token, mine.len]), f, ensure_ascii=False)
    print("wrote", t.FIX)


if __name__ == "__main__":
    main()
