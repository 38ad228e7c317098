"""Per-utterance LoRA: decode step time and prompt-pass time with the low-rank terms of the chosen targets on every row.

  python tools/lora_probe.py [--rows 1,8,32] [--tokens 384] [--dtype fp32] [--targets attn,all] [--modes none,fold,launch] [--prompt 32x512]
                             [--tag NAME] [--out profiles/mlp_lora_probe.jsonl]
  python tools/lora_probe.py --summary profiles/mlp_lora_probe.jsonl

--targets  attn = q/k/v/o, mlp = gate / up / down, all = the seven (a comma list: measured one after the other on the same engine)
--modes    none     no adapters (the engine's own choice of launches: the persistent launch at <= 8 rows)
           chain    no adapters, the launch chain at every row count (persistent_rows 0): the base line of the per-launch prices below 9 rows
           fold     adapters on every row, q/k/v/o terms from worker workgroups inside the QKV / o_proj launches (lora_fold 1; <= 8 rows and q/k/v/o only: "persist" below)
           launch   ... from two more launches per layer (lora_fold 0), launch chain at every row count
           persist  q/k/v/o adapters inside the persistent launch (<= 8 rows); with MLP targets the step takes the launch chain whatever this says
           MLP targets always cost two more launches per layer (lora.hip), in every mode.
--prompt   BxT: the prompt pass of B prompts of T tokens (ctts_gpt_begin of a 1-token generate), none and every --targets entry

Times are device-synchronised wall times; every shape is run once before it is timed (graphs captured, kernels loaded).  One invocation measures every
configuration ONCE and appends one JSON line per configuration to --out with its --tag; run the invocations to be compared alternately (A B A B A B: e.g. this build and,
through CTTS_HIP_LIB, the parent commit's library) and let --summary print the median and the spread (max - min) per tag and configuration.
Decode leg: ms = (t(tokens) - t(tokens / 4)) / (tokens - tokens / 4), ONE such difference per invocation: steps at contexts 48 + tokens / 4 .. 48 + tokens (mean ~300
keys at the default 384).  Prompt leg: ms = the best of three one-token generate() calls inside the invocation (prompt pass + one decode step + the call's host work).
(Until the MLP targets came the tool printed `ms_per_step`, the best of `--reps` differences, and `fold` forced persistent_lora 0: profiles/r04_lora_fold_probe.jsonl.)"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="32"); ap.add_argument("--tokens", type=int, default=384); ap.add_argument("--dtype", default="fp32")
ap.add_argument("--targets", default="attn"); ap.add_argument("--modes", default="none,fold,launch"); ap.add_argument("--prompt", default="")
ap.add_argument("--tag", default="this"); ap.add_argument("--out", default=""); ap.add_argument("--summary", default="")
a = ap.parse_args()

if a.summary:
    groups = {}
    for line in open(a.summary):
        d = json.loads(line)
        key = (d["tag"], d["leg"], d["dtype"], d["rows"], d.get("tokens", 0), d["targets"], d["mode"])
        groups.setdefault(key, []).append(d["ms"])
    print("| tag | leg | dtype | rows | targets | mode | runs | median ms | spread ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in sorted(groups, key=lambda k: (k[1], k[3], k[5], k[6], k[0])):
        v = groups[key]
        print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]}{'x' + str(key[4]) if key[1] == 'prompt' else ''} | {key[5]} | {key[6]} | {len(v)} | {statistics.median(v):.4f} | {max(v) - min(v):.4f} |")
    sys.exit(0)

import numpy as np, torch
from chatttsplus_amd import synth
from chatttsplus_amd.hip_models import GPT

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
SHAPES = dict(q_proj=(768, 768), k_proj=(768, 768), v_proj=(768, 768), o_proj=(768, 768), gate_proj=(3072, 768), up_proj=(3072, 768), down_proj=(768, 3072))
SETS = dict(attn=("q_proj", "k_proj", "v_proj", "o_proj"), mlp=("gate_proj", "up_proj", "down_proj"))
SETS["all"] = SETS["attn"] + SETS["mlp"]
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
SD = synth.gpt_state_dict(synth.GPT_REAL, 1234)


def emit(**d):
    d = dict(dict(tag=a.tag, dtype=a.dtype), **d)
    print(json.dumps(d), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(d) + "\n")


def load_adapters(g, targets):
    rl = np.random.Generator(np.random.Philox(key=31))
    for slot in range(4):
        g.load_adapter(slot, [(l, t, (rl.standard_normal((8, SHAPES[t][1])) * 0.02).astype(np.float32), (rl.standard_normal((SHAPES[t][0], 8)) * 0.02).astype(np.float32), 2.0)
                              for l in range(20) for t in SETS[targets]])


def timed(g, ids, mask, n):
    B, T = mask.shape
    emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    list(g.generate(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=n, min_new_token=n,
                    logits_warpers=LW, logits_processors=LP, return_hidden=False, noise="device", seed=7))
    torch.cuda.synchronize(); return time.perf_counter() - t0


for B in [int(r) for r in a.rows.split(",") if r]:
    g = GPT(LLAMA, max_batch=B, max_seq_len=48 + a.tokens + 32, weight_dtype=a.dtype)
    g.load_state_dict(SD)
    rows0 = g.get_option("persistent_rows")
    ids, mask = synth.prompt_ids(B, 48, 21178, 4321)
    for ti, targets in enumerate(a.targets.split(",")):
        load_adapters(g, targets)
        for mode in a.modes.split(","):
            if mode in ("none", "chain") and ti > 0:
                continue                                                  # adapter-free runs do not depend on what the slots hold
            g.set_row_adapters(None if mode in ("none", "chain") else [b % 4 for b in range(B)])
            g.set_option("lora_fold", {"launch": 0, "fold": 1, "notake": 2, "zeros": 3}.get(mode, 1))
            g.set_option("persistent_lora", 0 if mode == "launch" else 1)
            g.set_option("persistent_rows", 0 if mode == "chain" else rows0)
            lo, hi = a.tokens // 4, a.tokens
            timed(g, ids, mask, hi); timed(g, ids, mask, lo)              # every shape once before it is timed
            ms = (timed(g, ids, mask, hi) - timed(g, ids, mask, lo)) / (hi - lo) * 1e3
            emit(leg="decode", rows=B, tokens=a.tokens, targets="-" if mode in ("none", "chain") else targets, mode=mode, ms=round(ms, 5))
        for slot in range(4):
            g.load_adapter(slot, [])
    g.set_option("persistent_rows", rows0)
    g.set_row_adapters(None)
    g.close()

if a.prompt:
    B, T = (int(v) for v in a.prompt.split("x"))
    g = GPT(LLAMA, max_batch=B, max_seq_len=T + 16, weight_dtype=a.dtype)
    g.load_state_dict(SD)
    ids, mask = synth.prompt_ids(B, T, 21178, 4321)
    for targets in ["-"] + a.targets.split(","):
        if targets != "-":
            load_adapters(g, targets)
        g.set_row_adapters(None if targets == "-" else [b % 4 for b in range(B)])
        timed(g, ids, mask, 1); timed(g, ids, mask, 1)
        ms = min(timed(g, ids, mask, 1) for _ in range(3)) * 1e3           # prompt pass + one decode step + the call's host work
        emit(leg="prompt", rows=B, tokens=T, targets=targets, mode="none" if targets == "-" else "launch", ms=round(ms, 4))
    g.set_row_adapters(None)
    g.close()
