"""Log-probs inside generate (ctts_gpt_set_logprob_out) and N-candidate ranking: what they cost (report, not a gate).

Writes profiles/gen_logprob_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine):
  step      ms per decode step with log-probs off and on at 1, 8 and 32 rows, context about 300 (prompt 44 + 256 generated tokens, then 64 timed graph
            steps, ctts_gpt_time_decode): three alternating off / on runs each, medians and spread (max - min)
  kernel    the sampler kernel's mean duration off and on at 32 rows, from two separate `rocprofv3 --kernel-trace --stats` runs of this program's
            --child mode (the program goes after `--`); skipped with --no-trace or when rocprofv3 is missing
  request   one 8-utterance x 4-candidate request (infer(num_candidates=4), 32 rows) against the same 8 utterances plain: wall time, useful tokens per
            second (the tokens of the 8 returned utterances), and how often candidate 0 -- the plain generation -- won
  accuracy  the worst differences of the sampler's log-probs against the float32 reference on the inputs of tests/test_gpu_gen_logprobs.py, test 1

    python tools/gen_logprob_probe.py [--out profiles/gen_logprob_probe.jsonl] [--no-trace]
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chatttsplus_amd import _lib, synth                           # noqa: E402
from chatttsplus_amd.hip_models import GPT                         # noqa: E402
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects   # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
PROMPT, WARM, TIMED = 44, 256, 64


def step_ms(g, B, on, timed=TIMED):
    """One call: prompt of PROMPT tokens, WARM generated tokens (context ~300), then `timed` graph steps timed by the engine."""
    max_new = WARM + timed + 8
    ids, mask = synth.prompt_ids(B, PROMPT, synth.GPT_REAL["num_text_tokens"], 7)
    emb = g(torch.from_numpy(ids), torch.ones(B, PROMPT, dtype=torch.bool)).contiguous()
    dev = g.device
    lw = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
    lp = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, max_new, max_new, lw, lp, 4)
    out = torch.empty(B, max_new, 4, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    end = torch.zeros(B, dtype=torch.int32, device=dev)
    lps = torch.empty(2, B, max_new, 4, device=dev)
    io = _lib.GenIO(ids=out.data_ptr(), hiddens=None, finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    lib, h, st = g._lib, g._h, g._stream()
    _lib.check(lib.ctts_gpt_begin(h, B, PROMPT, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    if on:
        _lib.check(lib.ctts_gpt_set_logprob_out(h, lps[0].data_ptr(), lps[1].data_ptr(), st), "set_logprob_out")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    _lib.check(lib.ctts_gpt_sample(h, st), "sample")
    _lib.check(lib.ctts_gpt_decode(h, WARM - 1, 1, st), "decode")
    ms = C.c_float(0)
    _lib.check(lib.ctts_gpt_time_decode(h, timed, C.byref(ms), st), "time_decode")
    torch.cuda.synchronize()
    return float(ms.value)


def engine(max_batch=32):
    g = GPT(LLAMA, max_batch=max_batch, max_seq_len=PROMPT + WARM + TIMED + 16, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def child(on):
    """--child: 32 rows, one call; run under rocprofv3 by the parent."""
    g = engine()
    step_ms(g, 32, on)
    g.close()


def sampler_mean_us(on):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "on" if on else "off"]
        subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "sampler_generate_kernel" in row["Name"]:
                    return dict(calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 3))
    return None


def request_rows():
    from chatttsplus_amd.hip_models import Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams
    g = GPT(LLAMA, max_batch=32, max_seq_len=128 + 512, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 512 + 64, device="cuda:0", max_batch=32)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    with tempfile.TemporaryDirectory() as td:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(td), torch.device("cuda:0"))
        texts = synth.toy_texts(8, 11, 91, seed=256)
        params = InferCodeParams(prompt="[speed_5]", max_new_token=512, min_new_token=4, show_tqdm=False, spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
        rows = []
        for name, kw in (("plain", {}), ("candidates_4", dict(num_candidates=4, return_details=True)), ("plain", {}), ("candidates_4", dict(num_candidates=4, return_details=True))):
            sink = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", noise_seed=4242, slice_size=32, _ids_sink=sink, **kw))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            tokens = sum(int(i.shape[0]) for _, i in sink)
            row = dict(kind="request", request=name, utterances=8, wall_ms=round(dt * 1e3, 2), useful_tokens=tokens, useful_tok_per_s=round(tokens / dt, 1))
            if kw:
                row["candidate_0_won"] = sum(1 for k in out[0].candidate if k == 0)
                row["chosen"] = list(out[0].candidate)
                row["decoded_tokens"] = sum(int(c.ids.shape[0]) for cs in out[0].candidates for c in cs)
            rows.append(row)
    g.close()
    return rows


def accuracy_rows():
    import numpy as np
    from oracle import ref_cpu
    from tests.test_gpu_gen_logprobs import SETS, reference, run_rows_lp
    from tests.test_gpu_sampler import _cfg
    rows = []
    for temp, top_p, top_k, rep, scale, min_new in SETS:
        rng = np.random.Generator(np.random.Philox(key=99))
        n = 128
        logits = (rng.standard_normal((n, 626)) * scale).astype(np.float32)
        history = rng.integers(0, 626, size=(n, 23), dtype=np.int64)
        history[:, -4:] = history[:, -5:-4]
        for r in range(n):
            logits[r, history[r, -1]] += 2.0 * scale
        q = (-np.log1p(-rng.random((n, 626)))).astype(np.float32).clip(min=1e-30)
        if min_new:
            logits[:, 625] += 3.0 * scale
        sp = ref_cpu.SamplerParams(temperature=[temp] * 4, top_p=top_p, top_k=top_k, repetition_penalty=rep, min_new_token=min_new)
        temps = torch.full((n, 1), temp, dtype=torch.float32)
        idx, lpr, lps = run_rows_lp(_cfg(np.float32(temp), top_p, top_k, rep, min_new), logits, history, q, 23)
        raw32, tol_raw, s32, tol_s, same = reference(logits, history, 23, sp, temps, idx)
        rows.append(dict(kind="accuracy", temperature=temp, top_P=top_p, top_K=top_k, repetition_penalty=rep, min_new_token=min_new, rows=n,
                         lp_raw_max_diff=float((lpr - raw32).abs().max()), lp_raw_tolerance=tol_raw, lp_sampled_max_diff=float((lps - s32)[same].abs().max()),
                         lp_sampled_tolerance=tol_s, rows_left_out=int((~same).sum())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gen_logprob_probe.jsonl")
    ap.add_argument("--child", choices=["off", "on"])
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-request", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.child == "on")
        return
    rows = []
    g = engine()
    for B in (1, 8, 32):
        step_ms(g, B, False, timed=16)                               # warm-up: graphs captured
        runs = {False: [], True: []}
        for _ in range(3):
            for on in (False, True):
                runs[on].append(step_ms(g, B, on))
        off, on = statistics.median(runs[False]), statistics.median(runs[True])
        rows.append(dict(kind="step", rows=B, context=PROMPT + WARM, timed_steps=TIMED, off_ms=round(off, 5), on_ms=round(on, 5),
                         off_runs=[round(v, 5) for v in runs[False]], on_runs=[round(v, 5) for v in runs[True]],
                         off_spread_ms=round(max(runs[False]) - min(runs[False]), 5), on_spread_ms=round(max(runs[True]) - min(runs[True]), 5),
                         on_minus_off_us=round((on - off) * 1e3, 3), on_over_off=round(on / off, 5)))
        print(json.dumps(rows[-1]), flush=True)
    g.close()
    if not args.no_trace:
        k_off, k_on = sampler_mean_us(False), sampler_mean_us(True)
        if k_off and k_on:
            rows.append(dict(kind="kernel", kernel="sampler_generate_kernel", rows=32, off=k_off, on=k_on, on_minus_off_us=round(k_on["mean_us"] - k_off["mean_us"], 3)))
            for r in rows:
                if r["kind"] == "step":
                    r["bound_us"] = k_off["mean_us"]                 # the feature may cost less than a second sampler launch
                    r["within_bound"] = bool(r["on_minus_off_us"] <= k_off["mean_us"])
            print(json.dumps(rows[-1]), flush=True)
    for r in accuracy_rows():
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
