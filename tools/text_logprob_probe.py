"""Log-probs of the refine-text pass (ctts_gpt_set_text_logprob_out; ctts_gpt_score_text): what they cost (report, not a gate; no figure is fixed in advance), and
that a call which does not ask for them costs what it did.

Appends to profiles/text_logprob_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, max_batch 32).
  off_vs_baseline  (--baseline-lib PATH: a libctts_hip.so built from the parent commit)  GPU ms per text step (ctts_gpt_time_decode, 64 steps) of an infer_text call
                   at 1 / 8 / 32 rows, unguided and guided, WITHOUT the feature, the baseline library against this tree's: child processes that load one library
                   each (CTTS_HIP_LIB), alternating baseline / tree, three of each; medians, spread = max - min over a library's three runs.  "slower": the tree's
                   median exceeds the baseline's by more than the baseline's own spread.
  step             this tree's library, one process: off / lp_sampled only / both buffers, alternating, medians of three -- the cost of the feature per step.
                   Expectation from the code alone: lp_sampled is one owner thread's logf; lp_raw is two more block reductions and one more pass over the row's
                   85 KB of logits in L2.
  score_text       ms per ctts_gpt_score_text call (hipEvents around the call, median of three after a warm-up) for one small and one multi-chunk shape.

    python tools/text_logprob_probe.py [--out profiles/text_logprob_probe.jsonl] [--baseline-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import _lib, synth                            # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402
from chatttsplus_amd.hip_models.gpt import TextGuide, sampler_cfg_from_objects   # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
ROWS, MAX_NEW, T = 32, 128, 24
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
FREE = [9, 1023, 1024, 5000, 21176]
N_SRC = MAX_NEW - 8                                                # a guided row cannot end before its 120 source ids are out: none ends inside the timed steps
LEGS = [(B, guided) for B in (1, 8, 32) for guided in (False, True)]


def engine():
    g = GPT(LLAMA, max_batch=ROWS, max_seq_len=T + MAX_NEW + 8, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def step_ms(g, B, guided, lp="off", steps=64):
    """ms per step (ctts_gpt_time_decode) of an infer_text call with B rows; lp: "off" (the entry point is not called), "sampled" (lp_raw NULL) or "both" """
    lib, h, dev = g._lib, g._h, g.device
    ids, mask = synth.prompt_ids(B, T, synth.GPT_REAL["num_text_tokens"], 7)
    emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool)).contiguous()
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sc = sampler_cfg_from_objects(torch.tensor([0.7]), 21177, MAX_NEW, MAX_NEW - 1, LW, [], 4, infer_text=True)
    out = dict(ids=torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev), fin=torch.zeros(B, dtype=torch.int32, device=dev),
               end=torch.zeros(B, dtype=torch.int32, device=dev), lp=torch.empty(2, B, MAX_NEW, device=dev))
    io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=5)
    _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    if guided:
        rng = np.random.Generator(np.random.Philox(key=11))
        g._set_text_guide(st, TextGuide(FREE, 2))
        g._set_guides(st, list(range(B)), [[int(i) for i in rng.integers(2100, 20000, size=N_SRC)] for _ in range(B)])
    if lp != "off":
        _lib.check(lib.ctts_gpt_set_text_logprob_out(h, out["lp"][0].data_ptr() if lp == "both" else None, out["lp"][1].data_ptr(), st), "set_text_logprob_out")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    _lib.check(lib.ctts_gpt_sample(h, st), "sample")
    ms = C.c_float(0)
    _lib.check(lib.ctts_gpt_time_decode(h, steps, C.byref(ms), st), "time_decode")
    torch.cuda.synchronize()
    assert int(out["end"].min()) >= steps, "a row ended inside the timed steps"
    return float(ms.value)


def child_off():
    """--child-off: every leg with the feature off on the library CTTS_HIP_LIB names; one JSON line {leg: ms}"""
    have = C.CDLL(_lib.LIB_PATH)                                   # (a baseline library predates the newer entry points: bind what it has)
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(have, s[0])]
    g = engine()
    try:
        res = {}
        for B, guided in LEGS:
            step_ms(g, B, guided, steps=16)                        # warm-up: graphs captured
            res[f"{B}-{int(guided)}"] = step_ms(g, B, guided)
    finally:
        g.close()
    print("RESULT " + json.dumps(res), flush=True)


def off_vs_baseline(baseline):
    runs = {"baseline": [], "tree": []}
    for _ in range(3):
        for name, lib in (("baseline", baseline), ("tree", None)):
            env = dict(os.environ)
            env.pop("CTTS_HIP_LIB", None)
            if lib is not None:
                env["CTTS_HIP_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-off"], env=env, check=True, timeout=300, capture_output=True, text=True)
            runs[name].append(json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
            print(f"# {name}: {runs[name][-1]}", flush=True)
    rows = []
    for B, guided in LEGS:
        k = f"{B}-{int(guided)}"
        b, t = [r[k] for r in runs["baseline"]], [r[k] for r in runs["tree"]]
        mb, mt = statistics.median(b), statistics.median(t)
        rows.append(dict(kind="off_vs_baseline", rows=B, guided=guided, baseline=round(mb, 4), baseline_spread=round(max(b) - min(b), 4), tree=round(mt, 4),
                         tree_spread=round(max(t) - min(t), 4), tree_minus_baseline_us=round((mt - mb) * 1e3, 2), slower=bool(mt - mb > max(b) - min(b))))
    return rows


def step_rows(g):
    rows = []
    modes = ("off", "sampled", "both")
    for B, guided in LEGS:
        for lp in modes:
            step_ms(g, B, guided, lp, 16)
        runs = {m: [] for m in modes}
        for _ in range(3):
            for lp in modes:
                runs[lp].append(step_ms(g, B, guided, lp))
        med = {m: statistics.median(v) for m, v in runs.items()}
        rows.append(dict(kind="ms_per_step", rows=B, guided=guided, **{m: round(med[m], 4) for m in modes}, **{m + "_spread": round(max(runs[m]) - min(runs[m]), 4) for m in modes},
                         sampled_minus_off_us=round((med["sampled"] - med["off"]) * 1e3, 2), both_minus_off_us=round((med["both"] - med["off"]) * 1e3, 2)))
    return rows


def score_rows(g):
    rows = []
    dev = g.device
    chunk = g.get_option("score_text_chunk")
    for name, B, Tn, n in (("small", 2, 24, 8), ("multi_chunk", 8, 120, 100)):
        ids, mask = synth.prompt_ids(B, Tn, synth.GPT_REAL["num_text_tokens"], 9)
        emb = g(torch.from_numpy(ids), torch.ones(B, Tn, dtype=torch.bool)).contiguous()
        msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
        tg = torch.randint(0, 21177, (B, n), dtype=torch.int32, device=dev)
        nt = np.full(B, n, dtype=np.int32)
        lp, am = torch.empty(B, n, device=dev), torch.empty(B, n, dtype=torch.int32, device=dev)
        ms = []
        for i in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(g._lib.ctts_gpt_score_text(g._h, B, Tn, msk.data_ptr(), emb.data_ptr(), tg.data_ptr(), nt.ctypes.data_as(C.c_void_p), n, lp.data_ptr(), am.data_ptr(),
                                                  g._stream()), "score_text")
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        rows.append(dict(kind="score_text", shape=name, B=B, T=Tn, targets_per_sequence=n, target_rows=B * n, chunk_rows=chunk, chunks=-(-B * n // chunk),
                         ms=round(statistics.median(ms), 3), spread=round(max(ms) - min(ms), 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/text_logprob_probe.jsonl")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child-off", action="store_true")
    args = ap.parse_args()
    if args.child_off:
        child_off()
        return
    rows = [dict(note="fp32 20-layer engine, max_batch 32; infer_text calls of 1 / 8 / 32 rows, unguided and every row guided; ctts_gpt_time_decode over 64 steps; "
                      "off_vs_baseline = the feature off, parent-commit library against this tree's, alternating child processes, medians of three, spread = max - min; "
                      "ms_per_step = off / lp_sampled only / both buffers, alternating in one process, medians of three; score_text = ms per call")]
    if args.baseline_lib:
        rows += off_vs_baseline(args.baseline_lib)
    g = engine()
    try:
        rows += step_rows(g)
        rows += score_rows(g)
    finally:
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
