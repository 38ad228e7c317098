"""Streaming from a serving session (DecodeSession.submit(stream=...) / take_windows, ctts_synth_windows): time to first audio and what the windows cost (report,
not a gate).

Writes profiles/stream_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, max_batch 32: the engine, prompts and arrival schedule of
tools/session_probe.py -- one utterance at step 0, a burst of 7 at step 32, a burst of 24 at step 64, then one every 24 steps x 8; token limits 48..128).
Every utterance of a pass is served the same way; the ways alternate in one process, medians of three (spread = max - min):
  exact8 / exact24   stream="exact", stream_batch 8 / 24: settled samples only
  eager24            stream="eager", stream_batch 24: infer(stream=True)'s rule
  plain              not streaming: the utterance is vocoded when its last token is out
Per way: time from submit to the first sample ON THE HOST (every chunk is copied to the host as a service would; for `plain` the whole waveform), time to the
last one, the GPU ms of a poll's window vocoding by the number of windows in the call (events around Synth.synth_windows), polls and windows per pass.
  --parent-tree DIR  a built checkout of the parent commit: the host time (enqueue, no sync) and GPU time of one Synth.decode_window call for 1 / 8 / 32 rows
                     -- a 4096-sample interior window of a 400-token prefix each, 115 tokens of it vocoded -- in a fresh process per tree, the trees
                     alternating, three runs each.  The parent's decode_window goes through ctts_synth_batch (one allocation per row, full sub-waveforms,
                     host slicing), this tree's through ctts_synth_windows.  Without the argument the comparison is recorded as unmeasured.

    python tools/stream_probe.py [--out profiles/stream_probe.jsonl] [--parent-tree DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _med(vals, nd=3):
    return round(statistics.median(vals), nd), round(max(vals) - min(vals), nd)


def child_host():
    """--child-host: this process imports the package of the tree it was started in (cwd) and times Synth.decode_window"""
    sys.path.insert(0, os.getcwd())
    import numpy as np
    import torch
    from chatttsplus_amd import synth
    from chatttsplus_amd.hip_models import Synth
    s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=1024, max_batch=32)
    s.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    s.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    rng = np.random.Generator(np.random.Philox(key=5))
    hs = [torch.from_numpy(rng.standard_normal((400, 768)).astype(np.float32)).cuda() for _ in range(32)]
    s0, s1 = 256 * 300, 256 * 300 + 4096
    out = {}
    for rows in (1, 8, 32):
        host, gpu = [], []
        for rep in range(60):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t = time.perf_counter()
            w = s.decode_window(hs[:rows], [s0] * rows, [s1] * rows)
            dt = time.perf_counter() - t
            e1.record()
            torch.cuda.synchronize()
            assert len(w) == rows and w[0].shape[0] == 4096
            if rep >= 10:
                host.append(dt * 1e6)
                gpu.append(e0.elapsed_time(e1))
        out[rows] = dict(host_us=round(statistics.median(host), 1), gpu_ms=round(statistics.median(gpu), 4))
    print("RESULT " + json.dumps(out), flush=True)


def host_rows(parent_tree):
    if not parent_tree:
        return [dict(kind="decode_window_host", unmeasured="no --parent-tree given: the parent commit's decode_window path was not timed")]
    runs = {"parent commit": [], "this commit": []}
    for _ in range(3):
        for name, tree in (("parent commit", os.path.abspath(parent_tree)), ("this commit", ROOT)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-host"], cwd=tree, check=True, timeout=300, capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
    rows = []
    for name, rs in runs.items():
        for b in ("1", "8", "32"):
            h, hs_ = _med([r[b]["host_us"] for r in rs], 1)
            g, gs = _med([r[b]["gpu_ms"] for r in rs], 4)
            rows.append(dict(kind="decode_window_host", tree=name, rows=int(b), window_samples=4096, tokens_vocoded=115, host_us=h, host_us_spread=hs_, gpu_ms=g,
                             gpu_ms_spread=gs, runs=[r[b] for r in rs]))
    return rows


def serve(g, syn, emb, mask, way, sp):
    """one pass over session_probe's schedule; -> (first-audio ms by utterance, last-audio ms by utterance, [(windows in the call, start, end event)], polls)"""
    import torch
    arrivals, lims = sp.schedule()
    stream = None if way == "plain" else way.rstrip("0123456789")
    sb = None if way == "plain" else int(way[len(stream):])
    first, last, t_sub, utt_of, calls = {}, {}, {}, {}, []
    with g.open_session(torch.tensor([0.3] * 4), 625, sp.MAX_NEW, min_new_token=8, logits_warpers=sp.LW, logits_processors=sp.LP, return_hidden=True, seed=11,
                        rows=sp.ROWS, out_slots=3 * sp.ROWS) as ses:
        pending, skipped, polls = list(arrivals), 0, 0
        torch.cuda.synchronize()
        while pending or not ses.book.idle():
            now = ses.launched + skipped
            while pending and pending[0][0] <= now:
                _, u = pending.pop(0)
                tk = ses.submit(emb[u], mask[u], u, limit=lims[u], stream=stream, stream_batch=sb)
                utt_of[tk], t_sub[u] = u, time.perf_counter()
            res = ses.step()
            polls += 1
            if stream is None:
                done = [r for r in res if r.ids.shape[0] > 0]
                if done:
                    host = [w.cpu() for w in syn.decode_batch([r.hiddens for r in done])]
                    t = time.perf_counter()
                    for r in done:
                        first[utt_of[r.ticket]] = last[utt_of[r.ticket]] = (t - t_sub[utt_of[r.ticket]]) * 1e3
            else:
                wins = [w for w in ses.take_windows() if w.s1 > w.s0]
                if wins:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = syn.synth_windows([w.hiddens for w in wins], [w.s0 - 2 * w.tok0 * 256 for w in wins], [w.s1 - w.s0 for w in wins])
                    e1.record()
                    calls.append((len(wins), e0, e1))
                    host = [o.cpu() for o in out]
                    t = time.perf_counter()
                    for w in wins:
                        u = utt_of[w.ticket]
                        first.setdefault(u, (t - t_sub[u]) * 1e3)
                        if w.final:
                            last[u] = (t - t_sub[u]) * 1e3
            if pending and ses.book.idle():
                skipped = pending[0][0] - ses.launched
    torch.cuda.synchronize()
    return first, last, [(n, e0.elapsed_time(e1)) for n, e0, e1 in calls], polls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/stream_probe.jsonl")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-host", action="store_true")
    args = ap.parse_args()
    if args.child_host:
        child_host()
        return
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import session_probe as sp
    from chatttsplus_amd import synth
    from chatttsplus_amd.hip_models import Synth
    g = sp.engine()
    emb, mask = sp.inputs(g)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * sp.MAX_NEW + 64, max_batch=sp.ROWS)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    ways = ("exact8", "exact24", "eager24", "plain")
    rows = [dict(note="fp32 20-layer engine, max_batch 32, the arrival schedule of tools/session_probe.py (40 utterances, token limits 48..128), every utterance of a "
                      "pass served the same way; every chunk is copied to the host; ways alternating in one process, medians of three, spread = max - min")]
    for way in ways:
        serve(g, syn, emb, mask, way, sp)                                   # warm-up: graphs captured
    runs = {w: [] for w in ways}
    for _ in range(3):
        for way in ways:
            runs[way].append(serve(g, syn, emb, mask, way, sp))
    g.close()
    n = len(sp.schedule()[0])
    for way in ways:
        stats = []
        for first, last, calls, polls in runs[way]:
            f, l = [first[u] for u in range(n)], [last[u] for u in range(n)]
            stats.append(dict(first_mean=statistics.mean(f), first_median=statistics.median(f), first_max=max(f), first_lone=f[0], first_burst32=statistics.mean(f[8:32]),
                              last_mean=statistics.mean(l), last_lone=l[0], polls=polls, window_calls=len(calls), windows=sum(c for c, _ in calls),
                              window_gpu_ms_total=sum(ms for _, ms in calls)))
        row = dict(kind="audio_latency_ms", way=way, utterances=n)
        for k in stats[0]:
            row[k], row[k + "_spread"] = _med([s[k] for s in stats])
        rows.append(row)
        by_n = {}
        for _, _, calls, _ in runs[way]:
            per = {}
            for c, ms in calls:
                per.setdefault(c, []).append(ms)
            for c, v in per.items():
                by_n.setdefault(c, []).append((statistics.mean(v), len(v)))
        for c in sorted(by_n):
            if len(by_n[c]) == 3:                                            # (a window count that every run saw)
                m, s = _med([x for x, _ in by_n[c]], 4)
                rows.append(dict(kind="window_gpu_ms_per_poll", way=way, windows_in_call=c, gpu_ms=m, spread=s, calls_per_run=[k for _, k in by_n[c]]))
    rows += host_rows(args.parent_tree)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
