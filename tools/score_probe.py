"""Teacher-forced scoring (GPT.score / ctts_gpt_score): what the scoring stage costs next to the prompt pass (report, not a gate).

Writes profiles/score_probe.jsonl: for 1 x (48 + 512), 8 x (56 + 256) and 32 x (48 + 512) rows (prompt + codes, every code a target) on fp32 and fp16
engines (synthetic weights at real size, 20 layers): the median of --reps timed calls after warm-up, with device events, of
  score     ctts_gpt_score (prompt pass + gather + final norm and code heads on every scored row + the log-softmax / argmax reduction),
  prefill   the prompt pass alone over the same rows (ctts_gpt_begin + ctts_gpt_prefill: the same layer stack),
and score - prefill = the scoring stage, against the target of <= 10 % of the prompt pass.  Also the device memory the first score call allocates.

    python tools/score_probe.py [--out profiles/score_probe.jsonl] [--reps 7]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chatttsplus_amd import _lib, synth                           # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs   # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
SHAPES = [(1, 48, 512), (8, 56, 256), (32, 48, 512)]


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    fn(); fn()                                                     # warm-up
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/score_probe.jsonl")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sd = synth.gpt_state_dict(synth.GPT_REAL, 1234)
    rows = []
    for wd in ("fp32", "fp16"):
        g = GPT(LLAMA, max_batch=32, max_seq_len=48 + 512 + 8, weight_dtype=wd)
        g.load_state_dict(sd)
        first = True
        for B, P, N in SHAPES:
            gen = torch.Generator().manual_seed(B * 1000 + P)
            ids = torch.randint(0, synth.GPT_REAL["num_text_tokens"], (B, P, 1), generator=gen).expand(-1, -1, 4).contiguous()
            mask = torch.ones(B, P, dtype=torch.long)
            codes = [torch.randint(0, 625, (N, 4), generator=gen) for _ in range(B)]
            si = score_inputs(ids, mask, mask.bool(), codes, 625, append_eos=False)
            T = int(si["ids"].shape[1])
            emb = g(si["ids"], si["text_mask"]).contiguous()
            msk = si["mask"].cuda().contiguous()
            tg = si["targets"].cuda().contiguous()
            nt = si["n_targets"].numpy().astype("int32")
            maxt = int(si["targets"].shape[1])
            lp = torch.empty(B, maxt, 4, device="cuda"); am = torch.empty(B, maxt, 4, dtype=torch.int32, device="cuda")
            st = g._stream()

            def score():
                _lib.check(g._lib.ctts_gpt_score(g._h, B, T, msk.data_ptr(), emb.data_ptr(), tg.data_ptr(), nt.ctypes.data_as(C.c_void_p), maxt,
                                                 lp.data_ptr(), am.data_ptr(), st), "score")
            scratch = None
            if first:
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                score(); torch.cuda.synchronize()
                scratch = free0 - torch.cuda.mem_get_info()[0]
                first = False
            sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, 1, 0, [], [], 4)
            oi = torch.empty(B, 1, 4, dtype=torch.int32, device="cuda"); fin = torch.zeros(B, dtype=torch.int32, device="cuda")
            end = torch.zeros(B, dtype=torch.int32, device="cuda")
            io = _lib.GenIO(ids=oi.data_ptr(), hiddens=None, finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)

            def prefill():
                _lib.check(g._lib.ctts_gpt_begin(g._h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
                _lib.check(g._lib.ctts_gpt_prefill(g._h, emb.data_ptr(), st), "prefill")
            t_score = timed(score, args.reps)
            t_pre = timed(prefill, args.reps)
            t_score2 = timed(score, args.reps)                     # interleaved: the first and second score medians bracket the prefill one
            ts = min(t_score, t_score2)
            stage = ts - t_pre
            row = dict(dtype=wd, B=B, prompt=P, codes=N, rows=B * T, scored_rows=int(nt.sum()), score_ms=round(ts, 4), score_ms_runs=[round(t_score, 4), round(t_score2, 4)],
                       prefill_ms=round(t_pre, 4), scoring_stage_ms=round(stage, 4), stage_share=round(stage / t_pre, 4), target_share=0.10,
                       meets_target=bool(stage <= 0.10 * t_pre), reps=args.reps)
            if scratch is not None:
                row["first_call_alloc_bytes"] = int(scratch)
            print(json.dumps(row), flush=True)
            rows.append(row)
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
