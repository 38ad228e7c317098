"""Per-utterance sampling knobs: what they cost on the decode step (report, not a gate).

Writes profiles/row_sampling_probe.jsonl: ms per decode step at 1, 8 and 32 rows for
  uniform   every row on the call's knobs (no per-row request: top-P 0.7, top-K 20, penalty 1.05),
  temps     a per-row request whose rows differ in temperature only (the call's top-P / top-K / penalty): the per-row table itself, no dearer values,
  mixed     every row its own temperature and one of 4 (top-P, top-K <= 64, penalty) patterns,
  pattern0..3  every row on ONE of those patterns (its own temperature): what the values cost without mixing; `dearest` = the slowest of them,
  serial1   (32 rows) one row with top-k disabled: that block takes the sampler's serial path and the step waits for it,
and the case that motivates the feature: 32 utterances with 32 temperatures as ONE batch-32 call against 32 batch-1 calls, in useful tokens/s.
A step's time is the difference of two generations (256 and 64 tokens, every row forced to its limit) over the 192 extra steps, so the prompt pass
and the set-up cancel.  fp32 engine, synthetic weights at real size (20 layers), device noise.

    python tools/row_sampling_probe.py [--out profiles/row_sampling_probe.jsonl] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chatttsplus_amd import synth                                  # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402
from chatttsplus_amd.pipeline import gen_logits                    # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
T_PROMPT = 48


PATTERNS = [dict(top_P=0.7, top_K=20, repetition_penalty=1.05), dict(top_P=0.9, top_K=3, repetition_penalty=1.0),
            dict(top_P=None, top_K=64, repetition_penalty=1.3), dict(top_P=0.5, top_K=40, repetition_penalty=1.05)]


def knobs(n, serial_row=None, pattern=None, temps_only=False):
    out = []
    for u in range(n):
        d = dict(temperature=0.1 + 0.04 * u)
        if not temps_only:
            d.update(PATTERNS[u % 4 if pattern is None else pattern])
        if u == serial_row:
            d["top_K"] = None
        out.append(d)
    return out


def run(g, emb, ids, B, new, per_row, temps=None):
    w, p = gen_logits(625, 0.7, 20, 1.05)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = list(g.generate(emb[:B], torch.from_numpy(ids[:B]), torch.tensor(temps if temps is not None else [0.3]), 625, max_new_token=new, min_new_token=new,
                          logits_warpers=w, logits_processors=p, noise="device", seed=7, utt_ids=list(range(B)), sampling_per_row=per_row))[-1]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sum(int(i.shape[0]) for i in out.ids)


def step_ms(g, emb, ids, B, per_row, reps):
    vals = []
    for _ in range(reps):
        a, _ = run(g, emb, ids, B, 256, per_row)
        b, _ = run(g, emb, ids, B, 64, per_row)
        vals.append((a - b) * 1e3 / 192)
    vals.sort()
    return vals[len(vals) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/row_sampling_probe.jsonl")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    g = GPT(LLAMA, max_batch=32, max_seq_len=T_PROMPT + 256 + 8, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    ids, _ = synth.prompt_ids(32, T_PROMPT, synth.GPT_REAL["num_text_tokens"], seed=5)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    run(g, emb, ids, 32, 16, None)                                 # warm-up: graphs, allocator
    rows = []
    for B in (1, 8, 32):
        cases = [("uniform", None), ("temps", knobs(B, temps_only=True)), ("mixed", knobs(B))] + [(f"pattern{p}", knobs(B, pattern=p)) for p in range(4)]
        cases += [("serial1", knobs(B, serial_row=B - 1))] if B == 32 else []
        res = {name: step_ms(g, emb, ids, B, pr, args.reps) for name, pr in cases}
        res["dearest"] = max(res[f"pattern{p}"] for p in range(4))
        for name, ms in res.items():
            rows.append(dict(probe="row_sampling", rows=B, case=name, ms_per_step=round(ms, 4), vs_uniform=round(ms / res["uniform"] - 1.0, 4),
                             vs_dearest=round(ms / res["dearest"] - 1.0, 4)))
            print(json.dumps(rows[-1]), flush=True)
    # 32 utterances with 32 temperatures: one batch-32 call vs 32 batch-1 calls (useful tokens / s, 128 tokens each)
    temps = [dict(temperature=0.1 + 0.04 * u) for u in range(32)]
    t32, n32 = run(g, emb, ids, 32, 128, temps)
    t1 = n1 = 0
    for u in range(32):
        dt, n = run(g, emb[u:u + 1], ids[u:u + 1], 1, 128, None, temps=[temps[u]["temperature"]])
        t1 += dt
        n1 += n
    rows.append(dict(probe="row_sampling", case="32_temperatures", one_call_tok_s=round(n32 / t32, 1), batch1_calls_tok_s=round(n1 / t1, 1),
                     speedup=round((n32 / t32) / (n1 / t1), 2)))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    g.close()


if __name__ == "__main__":
    main()
