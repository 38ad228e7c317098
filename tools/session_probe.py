"""Serving session (GPT.open_session; ctts_gpt_grow / ctts_gpt_cancel): what an elastic decode batch buys over a call opened at its peak width (report, not a gate).

Writes profiles/session_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, max_batch 32).  One scripted arrival schedule, keyed by the number
of decode steps launched so that both ways see the same arrivals: one utterance at step 0, a burst of 7 at step 32 (8 rows), a burst of 24 at step 64 (32 rows),
then a trickle of one utterance every 24 steps.  Token limits 48..128.  Served two ways, alternating in one process, medians of three (spread = max - min):
  session   a DecodeSession: the batch is as wide as the utterances in flight (grow + admit on arrival, compact when they end)
  wide      a call opened 32 rows wide that carries dead rows: the same session code with compaction off, opened with the first utterance and 31 one-token
            utterances whose rows stay in the batch as finished rows; arrivals are admitted into them
Reported per way: per-utterance time from submit to delivery of the last token (mean, median, max over the utterances; the lone first utterance's own),
decode steps launched, and the mean GPU ms per step by row count (events around every ctts_gpt_decode call).  Steps after every row has finished exit on the
device, and the session keeps two chunks enqueued, so the chunk in which the last live row ends is partly idle and the one behind it wholly: only chunks whose
own row report (the ctts_gpt_rows_enqueue right behind them) still shows a live row are timed; the others are counted as `idle_chunks`.
  kernel    grow_rows_kernel / cancel_rows_kernel mean durations from a `rocprofv3 --kernel-trace --stats` run of this program's --child mode (the program
            goes after `--`); skipped with --no-trace or without rocprofv3

    python tools/session_probe.py [--out profiles/session_probe.jsonl] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import synth                                  # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
ROWS, MAX_NEW, T = 32, 128, 24
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]


def schedule():
    """[(decode steps launched at arrival, utterance index)], token limits"""
    arrivals = [(0, 0)] + [(32, 1 + i) for i in range(7)] + [(64, 8 + i) for i in range(24)] + [(160 + 24 * i, 32 + i) for i in range(8)]
    rng = np.random.Generator(np.random.Philox(key=77))
    lims = [int(x) for x in rng.integers(48, MAX_NEW + 1, size=len(arrivals))]
    return arrivals, lims


class TimedDecode:
    """the library handle with GPU events around every ctts_gpt_decode call: (rows, steps, start event, end event)"""

    def __init__(self, lib, rows_now):
        self._lib, self._rows_now, self.chunks = lib, rows_now, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ctts_gpt_decode":
            return fn

        def timed(h, n, graph, st):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(h, n, graph, st)
            e1.record()
            self.chunks.append((self._rows_now(), n, e0, e1))
            return rc
        return timed


def serve(g, emb, mask, way, cancel=()):
    """one pass over the schedule; returns (latencies ms by utterance, steps launched, {rows: [ms per step of each chunk]}, batch_trace)"""
    arrivals, lims = schedule()
    lib = g._lib
    keep_compact = g.compact
    g.compact = way == "session"
    lat, t_sub, utt_of = {}, {}, {}
    try:
        with g.open_session(torch.tensor([0.3] * 4), 625, MAX_NEW, min_new_token=8, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=11, rows=ROWS,
                            out_slots=3 * ROWS) as ses:
            timed = g._lib = TimedDecode(lib, lambda: len(ses.book.book.row_tk))
            pending = list(arrivals)
            if way == "wide":                              # 31 one-token utterances: their rows stay in the batch as finished rows
                for i in range(ROWS - 1):
                    ses.submit(emb[0], mask[0], 10_000 + i, limit=1)
            live_after = []                                # per chunk, in launch order (reports are read in that order): did its own row report show a live row
            book_report = ses.book.report

            def noting_report(layout, states):
                live_after.append(any(int(fin) == 0 for fin, _ in states))
                return book_report(layout, states)
            ses.book.report = noting_report
            to_cancel, skipped = set(cancel), 0            # `skipped`: steps the schedule's clock was moved up while nothing was in flight
            torch.cuda.synchronize()
            while pending or not ses.book.idle():
                now = ses.launched + skipped
                while pending and pending[0][0] <= now:
                    _, u = pending.pop(0)
                    tk = ses.submit(emb[u], mask[u], u, limit=lims[u])
                    utt_of[tk], t_sub[u] = u, time.perf_counter()
                for tk, u in utt_of.items():
                    if u in to_cancel and now >= t_cancel(u, arrivals):
                        ses.cancel(tk)
                        to_cancel.discard(u)
                for r in ses.step():
                    u = utt_of.get(r.ticket)
                    if u is not None and not r.cancelled:
                        lat[u] = (time.perf_counter() - t_sub[u]) * 1e3
                if pending and ses.book.idle():
                    skipped = pending[0][0] - ses.launched
            trace, launched = list(ses.batch_trace), ses.launched
        torch.cuda.synchronize()
        per_rows, idle = {}, 0
        for k, (rows, n, e0, e1) in enumerate(timed.chunks):
            if k < len(live_after) and live_after[k]:
                per_rows.setdefault(rows, []).append(e0.elapsed_time(e1) / n)
            else:                                          # every row had finished by the chunk's end (or its report was never read: the last chunk)
                idle += 1
        per_rows["idle_chunks"] = idle
    finally:
        g._lib, g.compact = lib, keep_compact
    return lat, launched, per_rows, trace


def t_cancel(u, arrivals):
    return next(s for s, v in arrivals if v == u) + 16


def inputs(g):
    n = len(schedule()[0])
    ids, mask = synth.prompt_ids(n, T, synth.GPT_REAL["num_text_tokens"], 7, pad_left=[u % 9 for u in range(n)])
    return g(torch.from_numpy(ids), torch.ones(n, T, dtype=torch.bool)), torch.from_numpy(mask)


def engine():
    g = GPT(LLAMA, max_batch=ROWS, max_seq_len=T + MAX_NEW + 8, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def child():
    """--child: two passes of the schedule through a session, four utterances cancelled in each; run under rocprofv3 by the parent"""
    g = engine()
    emb, mask = inputs(g)
    for _ in range(2):
        serve(g, emb, mask, "session", cancel=(3, 9, 20, 33))
    g.close()


def kernel_rows():
    exe = shutil.which("rocprofv3")
    if exe is None:
        return []
    out = []
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child"]
        subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ("grow_rows_kernel", "cancel_rows_kernel", "admit_rows_kernel", "compact_scatter_kernel"):
                    if k in row["Name"]:
                        out.append(dict(kind="kernel", kernel=k, calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 3),
                                        min_us=round(float(row.get("MinNs", "nan")) / 1e3, 3), max_us=round(float(row.get("MaxNs", "nan")) / 1e3, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/session_probe.jsonl")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        child()
        return
    g = engine()
    emb, mask = inputs(g)
    rows = [dict(note="fp32 20-layer engine, max_batch 32; arrivals keyed by decode steps launched: 1 at step 0, 7 at 32, 24 at 64, then 1 every 24 steps x 8; "
                      "token limits 48..128; session = elastic batch, wide = opened 32 rows wide with dead rows; alternating, medians of three, spread = max - min")]
    for way in ("session", "wide"):
        serve(g, emb, mask, way)                                        # warm-up: graphs captured
    runs = {"session": [], "wide": []}
    for _ in range(3):
        for way in ("session", "wide"):
            runs[way].append(serve(g, emb, mask, way))
    g.close()
    n = len(schedule()[0])
    for way in ("session", "wide"):
        stats = []
        for lat, launched, per_rows, trace in runs[way]:
            v = [lat[u] for u in range(n)]
            stats.append(dict(mean=statistics.mean(v), median=statistics.median(v), max=max(v), first=lat[0], burst8=statistics.mean(v[1:8]),
                              burst32=statistics.mean(v[8:32]), trickle=statistics.mean(v[32:])))
        row = dict(kind="latency_ms", way=way, utterances=n)
        for k in stats[0]:
            vals = [s[k] for s in stats]
            row[k] = round(statistics.median(vals), 3)
            row[k + "_spread"] = round(max(vals) - min(vals), 3)
        rows.append(row)
        rows.append(dict(kind="steps_launched", way=way, steps=[r[1] for r in runs[way]], idle_chunks_not_timed=[r[2]["idle_chunks"] for r in runs[way]],
                         batch_trace=runs[way][0][3]))
        merged = {}
        for _, _, per_rows, _ in runs[way]:
            for b, ms in per_rows.items():
                if b != "idle_chunks":
                    merged.setdefault(b, []).append((statistics.mean(ms), len(ms)))
        for b in sorted(merged):
            means = [m for m, _ in merged[b]]
            rows.append(dict(kind="ms_per_step", way=way, rows=b, ms_per_step=round(statistics.median(means), 4), spread=round(max(means) - min(means), 4),
                             chunks_per_run=[c for _, c in merged[b]]))
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
