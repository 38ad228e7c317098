"""Runs every case of tests/test_gpu_prompt_plans.py through that file's driver and records what was measured, one JSON line per case: dtype, engine, options,
pass rows, B, T, pads, the prompt plan, and for each of K, V (over the layers) and the last pass's residual rows X the worst per-lane rms-rel and the worst max abs
with the layer / lane / slot where they occur, beside the bounds the test applies; stray bytes, saturations, the invariant engines' decode-row logit error.
Nothing is asserted here; `plan_ok` says whether the case still ran the plan it was written for.

    python tools/prompt_plan_oracle.py --out profiles/prompt_plan_oracle.jsonl [--only fp16-wide]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prompt_plan_oracle.jsonl")
    ap.add_argument("--only", default="", help="run the cases whose id contains one of these (comma separated)")
    args = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # the CPU oracle: as tests/conftest.py
    from tests import test_gpu_prompt_plans as T
    only = args.only.split(",")
    with open(args.out, "w") as f:
        for c in T.CASES:
            if not any(o in T.case_id(c) for o in only):
                continue
            t0 = time.time()
            m = T.run_case(c)
            tol = T.TOL[c.wd]
            bad = T.plan_mismatches(m["plan"], c.expect)
            rec = dict(case=T.case_id(c), dtype=c.wd, engine=c.engine, options=c.opts, pass_rows=c.pass_rows, B=c.B, T=c.T, pads=list(c.pads), plan=m["plan"], plan_ok=not bad,
                       tol=tol, **T.worst(c, m), residual_rows=m["X"]["rows"], stray_bytes=m["stray_bytes"], saturations=m["saturations"])
            if m["inv"]:
                rec.update(logit_err=m["logit_err"], logit_err_bound=4 * tol * m["logit_scale"])
            rec["seconds"] = round(time.time() - t0, 2)
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(rec["case"], "plan_ok" if not bad else "PLAN MISMATCH " + str(bad),
                  " ".join(f"{q} rms-rel {rec[q]['rms_rel']:.3e} max {rec[q]['max_abs'] / rec[q]['max_abs_bound']:.3f} of bound" for q in ("K", "V", "X")),
                  f"stray {rec['stray_bytes']} sat {rec['saturations']}, {rec['seconds']} s", flush=True)
    T.close_engines()


if __name__ == "__main__":
    main()
