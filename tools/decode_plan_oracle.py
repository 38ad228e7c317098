"""Runs every case of tests/test_gpu_decode_plans.py through that file's driver and records what was measured, one JSON line per case: dtype, engine, options,
rows, prompt length, steps, the decode plan, the worst per-row rms-rel and max-abs hidden error and the worst logit error (absolute, and as a fraction of the
test's bound).  Nothing is asserted here; `plan_ok` says whether the case still ran the plan it was written for.

    python tools/decode_plan_oracle.py --out profiles/decode_plan_oracle.jsonl [--only fp16-wide]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/decode_plan_oracle.jsonl")
    ap.add_argument("--only", default="", help="run the cases whose id contains this")
    args = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # the CPU oracle: as tests/conftest.py
    from tests import test_gpu_decode_plans as T
    with open(args.out, "w") as f:
        for c in T.CASES:
            if args.only not in T.case_id(c):
                continue
            t0 = time.time()
            m = T.run_case(c)
            tol = T.TOL[c.wd]
            rec = dict(case=T.case_id(c), dtype=c.wd, engine=c.engine, options=c.opts, rows=c.B, T=c.T, pads=list(c.pads), steps=c.N, plan=m["plans"][-1],
                       plan_same_every_step=all(p == m["plans"][0] for p in m["plans"]), plan_ok=not any(T.plan_mismatches(p, c.expect) for p in m["plans"]),
                       tol=tol, worst_rms_rel=max(r[0] for r in m["rows"]), worst_max_abs=max(r[1] for r in m["rows"]), max_abs_bound=4 * tol * m["scale"],
                       worst_logit_err=max(e for e, _ in m["logits"]), worst_logit_err_of_bound=max(e / (4 * tol * s) for e, s in m["logits"]),
                       saturations=m["saturations"], seconds=round(time.time() - t0, 2))
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec["case"], "plan_ok" if rec["plan_ok"] else "PLAN MISMATCH " + str(T.plan_mismatches(m["plans"][-1], c.expect)),
                  f"rms-rel {rec['worst_rms_rel']:.3e} logits {rec['worst_logit_err_of_bound']:.3f} of bound, {rec['seconds']} s", flush=True)
    T.close_engines()


if __name__ == "__main__":
    main()
