"""The zero-shot encoder, clip by clip against batched (report, not a gate).

Writes profiles/encode_probe.jsonl (synthetic weights at real size, DVAEEncoder with its default max_seconds = 60; clips of 3-10 s at 24 kHz, lengths drawn once
from a fixed key).  For 1 / 8 / 32 clips two ways alternate in one process, three runs each, medians with spread = max - min; a run is the median of 20 timed
repetitions after 5 warm-up ones:
  loop    the parent commit's way: one DVAEEncoder.encode (ctts_dvae_encode) per clip
  batch   one DVAEEncoder.encode_batch (ctts_dvae_encode_batch) for all clips
Per way: GPU ms between two events around the call(s), and, separately, the host time of the call(s) (enqueue only, no synchronisation inside the timed region).
The outputs of the two ways are compared once (they must be bit-identical).

    python tools/encode_probe.py [--out profiles/encode_probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _med(vals, nd=3):
    return round(statistics.median(vals), nd), round(max(vals) - min(vals), nd)


def timed(fn, reps=20, warm=5):
    import torch
    host, gpu = [], []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t = time.perf_counter()
        fn()
        dt = time.perf_counter() - t
        e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            host.append(dt * 1e3)
            gpu.append(e0.elapsed_time(e1))
    return statistics.median(gpu), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/encode_probe.jsonl")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from chatttsplus_amd import synth
    from chatttsplus_amd.hip_models import DVAEEncoder
    enc = DVAEEncoder(dim=512).load_state_dict(synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234))
    rng = np.random.Generator(np.random.Philox(key=17))
    lengths = [int(n) for n in rng.integers(3 * 24000, 10 * 24000 + 1, size=32)]
    clips = [torch.from_numpy(synth.speaker_wave(100 + i, n)).cuda() for i, n in enumerate(lengths)]
    rows = [dict(note="DVAEEncoder (max_seconds 60), synthetic weights at real size; clips of 3-10 s at 24 kHz already on the device; loop = one ctts_dvae_encode per "
                      "clip (the parent commit's way), batch = one ctts_dvae_encode_batch; ways alternating in one process, three runs each (a run: median of 20 "
                      "repetitions after 5 warm-up ones), median and spread = max - min; gpu_ms between events, host_ms = the call(s) without synchronisation",
                 clip_samples=lengths)]
    for B in (1, 8, 32):
        ws = clips[:B]
        ways = dict(loop=lambda: [enc.encode(w) for w in ws], batch=lambda: enc.encode_batch(ws))
        same = all(torch.equal(a, b) for a, b in zip(ways["loop"](), ways["batch"]()))
        runs = {k: [] for k in ways}
        for _ in range(3):
            for k, fn in ways.items():
                runs[k].append(timed(fn))
        for k in ways:
            g, gs = _med([r[0] for r in runs[k]], 4)
            h, hs = _med([r[1] for r in runs[k]], 4)
            rows.append(dict(kind="encode", way=k, clips=B, seconds_of_audio=round(sum(lengths[:B]) / 24000, 2), gpu_ms=g, gpu_ms_spread=gs, host_ms=h, host_ms_spread=hs,
                             bit_identical_to_loop=same, runs=[dict(gpu_ms=round(a, 4), host_ms=round(b, 4)) for a, b in runs[k]]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
