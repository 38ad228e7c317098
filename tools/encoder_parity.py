"""Runs every case of tests/encoder_cases.py (the table behind tests/test_gpu_encoder_parity.py) through that module's helpers and records what was measured, one
JSON line per (case, quantiser shape): for the log-mel hook, the linear mel and the features the kernel's worst-frame error against the float64 oracle, the
yardstick (the float32 "dft"-form oracle's worst frame against the same reference, floored at 2^-23, computed on the CPU) and their ratio (the test's bound is
8); for the codes eps[r] (8 x the oracle's own float32-vs-float64 pre-round difference per residual level), the largest |p - q| of the teacher-forced digit
check and its excess over 0.5 + eps[r] (<= 0 passes), and the share of float64 digits within eps of a rounding boundary; seconds.  Nothing is asserted here.

    python tools/encoder_parity.py --out profiles/encoder_parity.jsonl [--only ckpt]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/encoder_parity.jsonl")
    ap.add_argument("--only", default="", help="run the cases whose id contains this")
    args = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # the CPU oracle: as tests/conftest.py
    from tests import encoder_cases as E
    cases = [c for c in E.CASES if args.only in c.id]
    # one handle at a time, as the tests: the plain handle (edge lengths longest first, then the input families), one handle per stress checkpoint, the other
    # quantiser shapes over the edge lengths, the handle of exactly the clip's capacity
    runs = [("plain", "g2r2", 1.5, [c for c in cases if c.variant == "plain" and c.id != "capacity-n24000"])]
    runs += [(c.variant, "g2r2", 1.5, [c]) for c in cases if c.variant != "plain"]
    runs += [("plain", q, 1.5, [c for c in cases if c in E.EDGES]) for q in ("g2r2-nobound", "g4r4")]
    runs += [("plain", "g2r2", 1.0, [c for c in cases if c.id == "capacity-n24000"])]
    with open(args.out, "w") as f:
        for variant, quant, seconds, group in runs:
            if not group:
                continue
            e = E.open_encoder(variant, quant, max_seconds=seconds)
            try:
                for c in group:
                    t0 = time.time()
                    ids, hook, feat = E.run_kernel(E.case_input(c), e)
                    m = E.measure(c, ids, hook, feat, quant)
                    m["seconds"] = round(time.time() - t0, 2)
                    f.write(json.dumps(m) + "\n")
                    f.flush()
                    print(E.fmt(m), flush=True)
            finally:
                E.close_encoder(e)


if __name__ == "__main__":
    main()
