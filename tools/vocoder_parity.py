"""Runs every case of tests/vocoder_cases.py (the table behind tests/test_gpu_vocoder_parity.py) through that module's helpers and records what was measured, one
JSON line per case: the kernel's worst-frame error against the float64 oracle, the float32 oracle's worst-frame error against the same reference (the
yardstick, computed on the CPU), their ratio (the test's bound is 8), both global rms errors and the largest activation the float64 run fed a GEMM.
Nothing is asserted here.

    python tools/vocoder_parity.py --out profiles/vocoder_parity.jsonl [--only vocos]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vocoder_parity.jsonl")
    ap.add_argument("--only", default="", help="run the cases whose id contains this")
    args = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # the CPU oracle: as tests/conftest.py
    from tests import vocoder_cases as V
    cases = [c for c in V.CASES if args.only in c.id]
    # one handle at a time: the 8-lane plain handle, the DVAE_full decoder, then one small handle per stress checkpoint
    groups = {}
    for c in cases:
        groups.setdefault(("full" if c.kind == "codes" else c.variant), []).append(c)
    with open(args.out, "w") as f:
        def record(c, got, t0):
            m = V.measure(c, got)
            m["seconds"] = round(time.time() - t0, 2)
            f.write(json.dumps(m) + "\n")
            f.flush()
            print(V.fmt(m), flush=True)
        for name, group in groups.items():
            if name == "full":
                s = V.open_synth("plain", full=True, max_frames=512, max_batch=4)
            elif name == "plain":
                s = V.open_synth("plain", max_frames=512, max_batch=8)
            else:
                s = V.open_synth(name)
            try:
                chain = [c for c in group if c.kind == "chain"]
                for c in group:
                    if c.kind != "chain":
                        t0 = time.time()
                        record(c, V.run_kernel(c, s), t0)
                if chain:                                        # as the test: ONE decode_batch call
                    t0 = time.time()
                    for c, got in zip(chain, V.run_batch(chain, s)):
                        record(c, got, t0)
            finally:
                V.close_synth(s)


if __name__ == "__main__":
    main()
