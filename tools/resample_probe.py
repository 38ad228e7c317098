"""Output sample rate (hip_models.Resampler, ctts_resample_windows): what the kernel and a resampled stream cost (report, not a gate).

Writes profiles/resample_probe.jsonl:
  kernel   resample_windows_kernel durations from a `rocprofv3 --kernel-trace --stats` run of this program's --child mode (the program goes after `--`), at
           24 kHz -> 16 kHz and -> 22.05 kHz: 1 / 8 / 32 interior windows of 4096 output samples (buffers cut to in_range, total = -1) and 32 whole 10 s
           waveforms.  The child issues 3 + 20 calls per configuration in a fixed order; the dispatches of the trace are cut into those groups and the
           first 3 of each dropped.  Each figure is read against (input + output + table bytes) at the 6.29 TB/s float4 copy rate the README records, the
           small calls against one launch's price (profiles/mlp_lora_probe.jsonl: 4.1 - 5.0 us).  The same calls timed with events (no profiler) are
           recorded beside them.  Skipped with --no-trace or without rocprofv3.
  stream   the added GPU ms of a poll's window vocoding with a rate: the engine, prompts and arrival schedule of tools/stream_probe.py (40 utterances,
           token limits 48..128), every utterance stream="exact" with stream_batch 8; per poll the windows are vocoded (Synth.synth_windows) and, with a
           rate, vocoded from their lookback as float32 and resampled (Resampler.resample_windows) by SynthSession's rule; events around both.  No rate,
           16 kHz and 22.05 kHz alternate in one process, medians of three (spread = max - min).

    python tools/resample_probe.py [--out profiles/resample_probe.jsonl] [--no-trace] [--no-stream]
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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

COPY_TBPS = 6.29
RATES = (16000, 22050)
WARM, REPS = 3, 20
CONFIGS = [(rate, kind, b) for rate in RATES for kind, b in (("windows_4096", 1), ("windows_4096", 8), ("windows_4096", 32), ("whole_10s", 32))]


def _med(vals, nd=3):
    return round(statistics.median(vals), nd), round(max(vals) - min(vals), nd)


def _calls():
    """[(rate, kind, B, bytes, call)] in CONFIGS order; call() issues one ctts_resample_windows launch"""
    import torch
    from chatttsplus_amd.hip_models import Resampler
    g = torch.Generator().manual_seed(3)
    wav = [(torch.rand(240000, generator=g) * 2 - 1).cuda() for _ in range(32)]
    out = []
    for rate in RATES:
        rs = Resampler(24000, rate)
        for kind, b in [(k, n) for r, k, n in CONFIGS if r == rate]:
            if kind == "whole_10s":
                srcs, args = wav[:b], ([0] * b, [240000] * b, [0] * b, [rs.out_total(240000)] * b)
            else:
                j0 = [rs.tile_outputs * (3 + u) + 5 * u + 1 for u in range(b)]
                rng = [rs.in_range(j, j + 4096) for j in j0]
                srcs, args = [wav[u][lo:hi] for u, (lo, hi) in enumerate(rng)], ([lo for lo, _ in rng], [None] * b, j0, [4096] * b)
            nbytes = sum(int(s.numel()) for s in srcs) * 4 + sum(args[3]) * 4 + rs.K * rs.new * 4
            out.append((rate, kind, b, nbytes, (lambda rs=rs, srcs=srcs, args=args: rs.resample_windows(srcs, *args))))
    return out


def child():
    """--child: WARM + REPS calls per configuration, in CONFIGS order; run under rocprofv3 by the parent"""
    import torch
    for _, _, _, _, call in _calls():
        for _ in range(WARM + REPS):
            call()
        torch.cuda.synchronize()


def kernel_rows(no_trace):
    import torch
    calls = _calls()
    ev = {}
    for rate, kind, b, nbytes, call in calls:
        ms = []
        for rep in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms.append(e0.elapsed_time(e1) * 1e3)
        ev[(rate, kind, b)] = _med(ms, 2)
    traced = {}
    exe = None if no_trace else shutil.which("rocprofv3")
    if exe is not None:
        with tempfile.TemporaryDirectory() as d:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child"]
            subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            disp = []
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if "resample_windows_kernel" in row.get("Kernel_Name", ""):
                        disp.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
            disp.sort()
            if len(disp) == len(CONFIGS) * (WARM + REPS):
                for i, (rate, kind, b) in enumerate(CONFIGS):
                    grp = disp[i * (WARM + REPS) + WARM:(i + 1) * (WARM + REPS)]
                    us = [(e - s) / 1e3 for s, e in grp]
                    traced[(rate, kind, b)] = (round(statistics.mean(us), 2), round(min(us), 2), round(max(us), 2))
            else:
                traced["error"] = f"{len(disp)} resample_windows_kernel dispatches in the trace, expected {len(CONFIGS) * (WARM + REPS)}"
    rows = []
    for rate, kind, b, nbytes, _ in calls:
        bound = nbytes / (COPY_TBPS * 1e12) * 1e6
        row = dict(kind="kernel", rate=rate, call=kind, windows=b, bytes=nbytes, byte_bound_us=round(bound, 2), event_us=ev[(rate, kind, b)][0],
                   event_us_spread=ev[(rate, kind, b)][1])
        if (rate, kind, b) in traced:
            m, lo, hi = traced[(rate, kind, b)]
            row.update(kernel_us_mean=m, kernel_us_min=lo, kernel_us_max=hi, times_byte_bound=round(m / bound, 1))
        else:
            row["kernel_us_unmeasured"] = traced.get("error", "no rocprofv3 run (--no-trace, or rocprofv3 not found)")
        rows.append(row)
    return rows


def serve(g, syn, emb, mask, sp, rs):
    """one pass over session_probe's schedule, every utterance exact8 (rs: its Resampler, or None) -> [(windows in the call, GPU ms)], output samples"""
    import torch
    from chatttsplus_amd.hip_models.vocoder import prefix_samples
    arrivals, lims = sp.schedule()
    calls, J, samples = [], {}, 0
    kw = {} if rs is None else dict(stream_lookback=rs.lookback)
    with g.open_session(torch.tensor([0.3] * 4), 625, sp.MAX_NEW, min_new_token=8, logits_warpers=sp.LW, logits_processors=sp.LP, return_hidden=True, seed=11,
                        rows=sp.ROWS, out_slots=3 * sp.ROWS) as ses:
        pending, skipped = list(arrivals), 0
        torch.cuda.synchronize()
        while pending or not ses.book.idle():
            now = ses.launched + skipped
            while pending and pending[0][0] <= now:
                _, u = pending.pop(0)
                J[ses.submit(emb[u], mask[u], u, limit=lims[u], stream="exact", stream_batch=8, **kw)] = 0
            ses.step()
            wins = ses.take_windows()
            if rs is not None:                                                 # SynthSession._vocode_windows' rule
                cut = []
                for w in wins:
                    j1 = rs.out_settled(w.s1, w.final, prefix_samples(w.n_tokens))
                    if j1 > J[w.ticket]:
                        cut.append((w, J[w.ticket], j1))
                        J[w.ticket] = j1
                wins = [w for w, _, _ in cut]
            else:
                wins = [w for w in wins if w.s1 > w.s0]
            if wins:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = syn.synth_windows([w.hiddens for w in wins], [w.v0 - 2 * w.tok0 * 256 for w in wins], [w.s1 - w.v0 for w in wins])
                if rs is not None:
                    out = rs.resample_windows(out, [w.v0 for w in wins], [prefix_samples(w.n_tokens) if w.final else None for w in wins], [j for _, j, _ in cut],
                                              [j1 - j for _, j, j1 in cut])
                e1.record()
                calls.append((len(wins), e0, e1))
                samples += sum(int(o.shape[0]) for o in [o.cpu() for o in out])
            if pending and ses.book.idle():
                skipped = pending[0][0] - ses.launched
    torch.cuda.synchronize()
    return [(n, e0.elapsed_time(e1)) for n, e0, e1 in calls], samples


def stream_rows():
    sys.path.insert(0, HERE)
    import session_probe as sp
    from chatttsplus_amd import synth
    from chatttsplus_amd.hip_models import Resampler, Synth
    g = sp.engine()
    emb, mask = sp.inputs(g)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * sp.MAX_NEW + 64, max_batch=sp.ROWS)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    ways = {None: None, **{r: Resampler(24000, r) for r in RATES}}
    for rs in ways.values():
        serve(g, syn, emb, mask, sp, rs)                                       # warm-up: graphs captured
    runs = {r: [] for r in ways}
    for _ in range(3):
        for r, rs in ways.items():
            runs[r].append(serve(g, syn, emb, mask, sp, rs))
    g.close()
    rows = [dict(note="fp32 20-layer engine, max_batch 32, the arrival schedule of tools/session_probe.py (40 utterances, token limits 48..128), every utterance "
                      "stream=\"exact\" with stream_batch 8; GPU ms between events around a poll's window vocoding (with a rate: float32 from the lookback + "
                      "one ctts_resample_windows call); the three ways alternating in one process, medians of three, spread = max - min")]
    base = None
    for r in ways:
        tot, ts = _med([sum(ms for _, ms in calls) for calls, _ in runs[r]], 3)
        per, ps = _med([statistics.mean(ms for _, ms in calls) for calls, _ in runs[r]], 4)
        row = dict(kind="stream_window_gpu_ms", rate=r or 24000, window_calls=[len(calls) for calls, _ in runs[r]], windows=[sum(n for n, _ in calls) for calls, _ in runs[r]],
                   samples_out=runs[r][0][1], total_ms=tot, total_ms_spread=ts, per_call_ms=per, per_call_ms_spread=ps)
        if r is None:
            base = (tot, per)
        else:
            row.update(added_total_ms=round(tot - base[0], 3), added_per_call_ms=round(per - base[1], 4))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/resample_probe.jsonl")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    args = ap.parse_args()
    if args.child:
        child()
        return
    rows = kernel_rows(args.no_trace)
    if not args.no_stream:
        rows += stream_rows()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
