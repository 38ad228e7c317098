"""Guided refine-text (ctts_gpt_set_text_guide / ctts_gpt_set_guides; sampler_text_kernel<true>): what a guided step costs against an unguided one (report, not a
gate; no figure is fixed in advance).

Writes profiles/text_guide_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, max_batch 32).
  step      GPU ms per decode step (ctts_gpt_time_decode, 64 steps), unguided against guided, alternating in one process, medians of three (spread = max - min):
            "text": a text-mode call (infer_text) with 1 / 8 / 32 text rows, every row guided;  "mixed": one text row among 1 / 8 / 32 rows of a code call, that
            row guided.  Expectation from the code alone: not slower than unguided -- a guided block reads at most 65 logits and reduces over at most 65 candidates.
            A guided leg slower than the unguided one by more than the unguided leg's own spread is flagged ("slower": true).
  dispatch  sampler_text_kernel<true> against <false>, per dispatch, from a `rocprofv3 --kernel-trace --stats` run of this program's --child mode (a run of its own;
            the program goes after `--`); skipped with --no-trace or without rocprofv3.

    python tools/text_guide_probe.py [--out profiles/text_guide_probe.jsonl] [--no-trace]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

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
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
FREE = [9, 1023, 1024, 5000, 21176]
N_SRC = MAX_NEW - 8                                                # a guided row cannot end before its 120 source ids are out: none ends inside the timed steps


def engine():
    g = GPT(LLAMA, max_batch=ROWS, max_seq_len=T + MAX_NEW + 8, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def step_ms(g, B, leg, guided, steps=64):
    """leg "text": B text rows of an infer_text call; "mixed": row 0 a text row among B rows of a code call.  ms per step of ctts_gpt_time_decode"""
    lib, h, dev = g._lib, g._h, g.device
    ids, mask = synth.prompt_ids(B, T, synth.GPT_REAL["num_text_tokens"], 7)
    emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool)).contiguous()
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tsc = sampler_cfg_from_objects(torch.tensor([0.7]), 21177, MAX_NEW, MAX_NEW - 1, LW, [], 4, infer_text=True)
    sc = tsc if leg == "text" else sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, MAX_NEW, MAX_NEW - 1, LW, LP, 4)
    out = dict(ids=torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev), tids=torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev),
               fin=torch.zeros(B, dtype=torch.int32, device=dev), end=torch.zeros(B, dtype=torch.int32, device=dev))
    io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=5)
    modes = np.ascontiguousarray([1 if b == 0 else 0 for b in range(B)], dtype=np.int32)
    if leg == "mixed":
        _lib.check(lib.ctts_gpt_set_row_modes(h, modes.ctypes.data_as(C.c_void_p), B), "set_row_modes")
    try:
        _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    finally:
        lib.ctts_gpt_set_row_modes(h, None, 0)
    if leg == "mixed":
        _lib.check(lib.ctts_gpt_enable_text_rows(h, C.byref(tsc), out["tids"].data_ptr(), st), "enable_text_rows")
    if guided:
        rng = np.random.Generator(np.random.Philox(key=11))
        slots = list(range(B)) if leg == "text" else [0]
        g._set_text_guide(st, TextGuide(FREE, 2))
        g._set_guides(st, slots, [[int(i) for i in rng.integers(2100, 20000, size=N_SRC)] for _ in slots])
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    _lib.check(lib.ctts_gpt_sample(h, st), "sample")
    ms = C.c_float(0)
    _lib.check(lib.ctts_gpt_time_decode(h, steps, C.byref(ms), st), "time_decode")
    torch.cuda.synchronize()
    assert int(out["end"].min()) >= steps, "a row ended inside the timed steps"
    return float(ms.value)


def step_rows():
    g = engine()
    rows = []
    try:
        for leg in ("text", "mixed"):
            for B in (1, 8, 32):
                for guided in (False, True):
                    step_ms(g, B, leg, guided, 16)                 # warm-up: graphs captured
                runs = {False: [], True: []}
                for _ in range(3):
                    for guided in (False, True):
                        runs[guided].append(step_ms(g, B, leg, guided))
                med = {k: statistics.median(v) for k, v in runs.items()}
                spread = {k: max(v) - min(v) for k, v in runs.items()}
                rows.append(dict(kind="ms_per_step", leg=leg, rows=B, unguided=round(med[False], 4), unguided_spread=round(spread[False], 4),
                                 guided=round(med[True], 4), guided_spread=round(spread[True], 4), guided_minus_unguided_us=round((med[True] - med[False]) * 1e3, 2),
                                 slower=bool(med[True] - med[False] > spread[False])))
    finally:
        g.close()
    return rows


def child(B):
    """--child B: 32 steps of a text-mode call at B rows, unguided and guided, twice; run under rocprofv3 by the parent"""
    g = engine()
    for guided in (False, True, False, True):
        step_ms(g, B, "text", guided, 32)
    g.close()


def kernel_rows():
    exe = shutil.which("rocprofv3")
    if exe is None:
        return []
    out = []
    for B in (1, 8, 32):
        with tempfile.TemporaryDirectory() as d:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", str(B)]
            subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            acc = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                rd = csv.DictReader(open(path))
                cols = rd.fieldnames or []
                name_c = next((c for c in ("Kernel_Name", "Name") if c in cols), None)
                t0_c = next((c for c in ("Start_Timestamp", "Start") if c in cols), None)
                t1_c = next((c for c in ("End_Timestamp", "End") if c in cols), None)
                if not (name_c and t0_c and t1_c):
                    out.append(dict(kind="kernel_trace_error", rows=B, columns=cols))
                    continue
                for r in rd:
                    if "sampler_text_kernel" in r[name_c]:
                        acc.setdefault(r[name_c], []).append((int(r[t1_c]) - int(r[t0_c])) / 1e3)
            for name, us in sorted(acc.items()):
                out.append(dict(kind="dispatch", rows=B, kernel=name[:120], calls=len(us), mean_us=round(statistics.mean(us), 3), median_us=round(statistics.median(us), 3),
                                min_us=round(min(us), 3), max_us=round(max(us), 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/text_guide_probe.jsonl")
    ap.add_argument("--child", type=int, default=0, metavar="ROWS")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    rows = [dict(note="fp32 20-layer engine, max_batch 32; ctts_gpt_time_decode over 64 steps, unguided vs guided alternating in one process, medians of three, "
                      "spread = max - min; leg text = an infer_text call with every row guided, leg mixed = one (guided) text row among the rows of a code call; "
                      "slower = guided - unguided exceeds the unguided leg's own spread; dispatch = per dispatch of a rocprofv3 --kernel-trace --stats run of its own")]
    rows += step_rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    if not args.no_trace:
        for r in kernel_rows():
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
