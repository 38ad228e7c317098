"""SHA-1 of the raw logprob and argmax bytes GPT.score / GPT.score_text return for the cases of tests/test_gpu_score.py and tests/test_gpu_score_text.py, for
comparing two libraries of one ABI bit for bit: one process per library (CTTS_HIP_LIB selects it), then diff the outputs.

    python tools/score_digests.py > head.txt;  CTTS_HIP_LIB=/path/to/parent/libctts_hip.so python tools/score_digests.py > parent.txt;  diff head.txt parent.txt

Code cases: short, long, several passes (pass_rows 256) and the 9 x 256 chunk-boundary case; text cases: padded, n1_nT, chunks.  Each on an fp32 engine, an fp16
engine and an fp32 engine under batch_invariant."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_score as S                              # noqa: E402
from tests import test_gpu_score_text as ST                        # noqa: E402


def digest(res):
    h = [hashlib.sha1() for _ in range(2)]
    for lp, am in zip(res.logprob, res.argmax):
        h[0].update(lp.contiguous().numpy().tobytes())
        h[1].update(am.to(torch.int32).contiguous().numpy().tobytes())
    return f"logprob {h[0].hexdigest()} argmax {h[1].hexdigest()}"


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))     # the float64 restatement of the text cases runs on the CPU
    ids, mask, tm, targets, nt = S.boundary_case()
    for dtype, opts in (("fp32", None), ("fp16", None), ("fp32", {"batch_invariant": 1})):
        tag = dtype + ("-inv" if opts else "")
        g, gp, g9 = S.engine(dtype, opts), S.engine(dtype, opts, pass_rows=256), S.engine(dtype, opts, max_batch=9, max_seq=256)
        print(tag, "score short", digest(S.run(g, S.case([12, 9], [5, 14], 12, 11))))
        print(tag, "score long", digest(S.run(g, S.case([16, 12, 7], [5, 23, 40], 16, 12))))
        print(tag, "score several_passes", digest(S.run(gp, S.case([30, 21, 9, 40], [120, 33, 150, 5], 40, 21))))
        print(tag, "score boundary_9x256", digest(g9.score(g9(ids, tm), mask, targets, nt)))
        for name in sorted(ST.CASES):
            print(tag, "score_text", name, digest(ST.run(g, ST._case(name)[0])), flush=True)


if __name__ == "__main__":
    main()
