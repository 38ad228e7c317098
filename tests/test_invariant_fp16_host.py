"""Host-side checks of the fp16 batch-invariance option ("schedule_invariant"): where the header documents it, and that the recorded probe says what the docs quote."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_documents_the_option_outside_the_named_options_comment():
    text = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    start, end = text.index("/* Named engine options"), text.index("Unknown names are an error. */")
    assert '"schedule_invariant"' not in text[start:end], "tests/test_gpu_options.py reads this comment as the list of options IT knows"
    after = text[end:]
    assert '"schedule_invariant"' in after
    for pin in ("persistent_rows 0", "split_rows 0", "down_splitk_rows 1", "nbg2_rows 0", "decode_splits 1", "attn_wide_blocks INT_MAX", "split_decode_rows 0", "prefill_split_rows 0", "valu_rows 0"):
        assert pin in after, f"the header does not state what {pin.split()[0]} reads on fp16 engines under the option"


def test_option_table_row():
    src = open(os.path.join(ROOT, "chatttsplus_amd", "csrc", "gpt_engine.hip")).read()
    row = re.search(r'\{"schedule_invariant", &ctts_gpt::(\w+), OPT_ANY, (OPT_RW \| OPT_FLAG), 0, (\w+)\}', src)
    ref = re.search(r'\{"batch_invariant", &ctts_gpt::(\w+), OPT_ANY, (OPT_RW \| OPT_FLAG), 0, (\w+)\}', src)
    assert row and ref and row.groups() == ref.groups(), "the dtype-independent name must be the same field, flags and hook as batch_invariant"


def test_recorded_probe_holds_what_the_docs_quote():
    lines = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "invariant_fp16_probe.jsonl"))]
    modes = {"default", "schedule_invariant"}
    steps = {(r["mode"], r["rows"]) for r in lines if r["probe"] == "step"}
    assert steps == {(m, b) for m in modes for b in (1, 2, 4, 5, 6, 8, 9, 16, 17, 32, 33, 56, 57, 64, 128)}
    assert {(r["mode"], r["B"], r["T"]) for r in lines if r["probe"] == "prompt"} == {(m, b, t) for m in modes for b, t in ((32, 512), (8, 56), (1, 96))}
    req = [r for r in lines if r["probe"] == "request"]
    assert len(req) == 12 and all(r["dtype"] == "fp16" and r["utterances"] == 256 for r in req)
    assert all(r["identical_to_32_rows_longest_first"] == 256 for r in req if r["mode"] == "schedule_invariant")
    off = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "invariant_fp16_offpath.jsonl"))]
    dig = {r["tree"]: r["sha256"] for r in off if r["probe"] == "offpath_digest"}
    assert set(dig) == {"parent", "this"} and dig["parent"] == dig["this"]
    assert sorted((r["tree"], r["run"]) for r in off if r["probe"] == "bench_headline") == [(t, i) for t in ("parent", "this") for i in (1, 2, 3, 4)]
