"""Shared prompt passes (ctts_gpt_share_prompts, kv_share.hip): what they save and what the replicate kernel costs (report, not a gate).

Writes profiles/share_prompt_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, 8 prompts x 4 candidates = 32 rows):
  prefill   begin + prefill, shared (8 prompt passes + one replicate launch) against unshared (32 prompt passes) at T = 100 and T = 400 (the length of
            a zero-shot speaker prompt): GPU time between two events, three alternating shared / unshared runs each, medians and spread (max - min)
  kernel    kv_share_kernel's mean duration and bytes/s at both lengths, from `rocprofv3 --kernel-trace --stats` runs of this program's --child mode
            (the program goes after `--`); bytes = groups x (1 + followers) x layers x 2 x heads x T x 256: every leader chunk is read once and
            written once per follower.  Next to it the device's measured float4 copy rate (6.29 TB/s); skipped with --no-trace or without rocprofv3
  request   the 8 x 4 x 512-token candidate request (infer(num_candidates=4), slice_size=32) end to end with share_prompt=True and False, alternating

    python tools/share_prompt_probe.py [--out profiles/share_prompt_probe.jsonl] [--no-trace] [--no-request]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import _lib, synth                           # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects   # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
PROMPTS, CANDS, MAX_NEW = 8, 4, 16
COPY_RATE = 6.29e12           # bytes/s, the device's measured float4 copy


def engine(max_seq):
    g = GPT(LLAMA, max_batch=PROMPTS * CANDS, max_seq_len=max_seq, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def prefill_ms(g, T, shared):
    """begin + prefill of 32 rows on 8 prompts of T tokens (left pads 0..7); GPU ms between two events"""
    B = PROMPTS * CANDS
    ids, mask = synth.prompt_ids(PROMPTS, T, synth.GPT_REAL["num_text_tokens"], 7, pad_left=list(range(PROMPTS)))
    pof = [p for p in range(PROMPTS) for _ in range(CANDS)]
    if not shared:
        ids, mask = ids[pof], mask[pof]
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[0], T, dtype=torch.bool)).contiguous()
    dev = g.device
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, MAX_NEW, 2, [], [], 4)
    out = torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    end = torch.zeros(B, dtype=torch.int32, device=dev)
    io = _lib.GenIO(ids=out.data_ptr(), hiddens=None, finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    lib, h, st = g._lib, g._h, g._stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    if shared:
        arr = np.ascontiguousarray(pof, dtype=np.int32)
        _lib.check(lib.ctts_gpt_share_prompts(h, B, arr.ctypes.data_as(C.c_void_p), PROMPTS), "share_prompts")
    _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    e1.record()
    torch.cuda.synchronize()
    return float(e0.elapsed_time(e1))


def child(T):
    """--child T: five shared begin + prefill calls; run under rocprofv3 by the parent"""
    g = engine(T + MAX_NEW + 16)
    for _ in range(5):
        prefill_ms(g, T, True)
    g.close()


def kernel_row(T):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", str(T)]
        subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "kv_share_kernel" in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    nbytes = PROMPTS * (1 + (CANDS - 1)) * LLAMA["num_hidden_layers"] * 2 * LLAMA["num_attention_heads"] * T * 64 * 4
                    return dict(kind="kernel", kernel="kv_share_kernel", T=T, groups=PROMPTS, followers=CANDS - 1, calls=int(row["Calls"]), mean_us=round(us, 3),
                                bytes=nbytes, bytes_per_s=round(nbytes / (us * 1e-6), 1), copy_rate_bytes_per_s=COPY_RATE,
                                fraction_of_copy_rate=round(nbytes / (us * 1e-6) / COPY_RATE, 4), bound_us=round(nbytes / COPY_RATE * 1e6, 3))
    return None


def request_rows():
    from chatttsplus_amd.hip_models import Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams
    g = engine(128 + 512)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 512 + 64, device="cuda:0", max_batch=32)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    rows = []
    with tempfile.TemporaryDirectory() as td:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(td), torch.device("cuda:0"))
        texts = synth.toy_texts(PROMPTS, 80, 100, seed=256)
        params = InferCodeParams(prompt="[speed_5]", max_new_token=512, min_new_token=4, show_tqdm=False, spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())

        def run(share):
            sink = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", noise_seed=4242, slice_size=32, _ids_sink=sink,
                                  num_candidates=CANDS, return_details=True, share_prompt=share))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return dt, sum(int(c.ids.shape[0]) for cs in out[0].candidates for c in cs), list(g.shared_prompts)

        run(True), run(False)                                           # warm-up: graphs captured
        for _ in range(3):
            for share in (True, False):
                dt, decoded, calls = run(share)
                rows.append(dict(kind="request", share_prompt=share, utterances=PROMPTS, candidates=CANDS, wall_ms=round(dt * 1e3, 2), decoded_tokens=decoded,
                                 shared_prompts=calls))
    g.close()
    for share in (True, False):
        w = [r["wall_ms"] for r in rows if r["share_prompt"] is share]
        rows.append(dict(kind="request_median", share_prompt=share, wall_ms=statistics.median(w), spread_ms=round(max(w) - min(w), 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/share_prompt_probe.jsonl")
    ap.add_argument("--child", type=int)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-request", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    rows = []
    for T in (100, 400):
        g = engine(T + MAX_NEW + 16)
        prefill_ms(g, T, True), prefill_ms(g, T, False)                 # warm-up
        runs = {True: [], False: []}
        for _ in range(3):
            for shared in (True, False):
                runs[shared].append(prefill_ms(g, T, shared))
        g.close()
        sh, un = statistics.median(runs[True]), statistics.median(runs[False])
        rows.append(dict(kind="prefill", T=T, prompts=PROMPTS, candidates=CANDS, shared_ms=round(sh, 4), unshared_ms=round(un, 4),
                         shared_runs=[round(v, 4) for v in runs[True]], unshared_runs=[round(v, 4) for v in runs[False]],
                         shared_spread_ms=round(max(runs[True]) - min(runs[True]), 4), unshared_spread_ms=round(max(runs[False]) - min(runs[False]), 4),
                         shared_over_unshared=round(sh / un, 4)))
        print(json.dumps(rows[-1]), flush=True)
    if not args.no_trace:
        for T in (100, 400):
            r = kernel_row(T)
            if r:
                rows.append(r)
                print(json.dumps(r), flush=True)
    if not args.no_request:
        for r in request_rows():
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
