"""What the batch-invariant mode (option "batch_invariant") costs, and what it buys.  One JSON line per measurement, both modes:
  step      ms per captured decode step vs rows (1 .. 64) at mean context ~309 (a 48-token prompt + 261 steps in, like tools/gpu_probe.py)
  prompt    the prompt pass (begin + prefill) at 32 x 512, 8 x 56 and 1 x 96 tokens
  request   the 256-utterance request of bench._request_256 through infer_sharded(continuous=True) at 32 / 16 / 8 rows x longest-first / arrival
            order: useful tok/s and how many utterances keep the token ids of the 32-row longest-first run
usage: python tools/invariant_probe.py [out.jsonl] [--skip-request] [--dtype fp16]
--dtype fp16: the same three probes on fp16 engines, default mode against option "schedule_invariant" (out.jsonl defaults to profiles/invariant_fp16_probe.jsonl).
The two engines live side by side in one process and alternate, three rounds: step and prompt lines carry the median and the spread (min, max) of the three."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from chatttsplus_amd import _lib, synth  # noqa: E402
from chatttsplus_amd.hip_models.gpt import GPT, sampler_cfg_from_objects  # noqa: E402

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
dev = torch.device("cuda:0")
DTYPE = sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "fp32"
out_path = next((a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--dtype"), None)
if out_path is None and DTYPE == "fp16":
    out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "invariant_fp16_probe.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def begin(g, B, T, N):
    ids, mask = synth.prompt_ids(B, T, 21178, 1)
    emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, N, N, LW, LP, 4)
    bufs = [torch.zeros(B, N, 4, dtype=torch.int32, device=dev), torch.zeros(B, N, 768, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
            torch.zeros(B, dtype=torch.int32, device=dev)]
    io = _lib.GenIO(ids=bufs[0].data_ptr(), hiddens=bufs[1].data_ptr(), finish=bufs[2].data_ptr(), end_idx=bufs[3].data_ptr(), noise=None, n_draws=0, seed=1)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    msk = torch.from_numpy(mask).to(dev).to(torch.int32)
    return emb, sc, io, st, msk, bufs


def step_times(g, mode, rows=(1, 2, 4, 8, 9, 16, 17, 24, 32, 33, 64), collect=None):
    lib, h = g._lib, g._h
    for B in rows:
        P, N = 48, 600
        emb, sc, io, st, msk, bufs = begin(g, B, P, N)
        _lib.check(lib.ctts_gpt_begin(h, B, P, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
        _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
        _lib.check(lib.ctts_gpt_sample(h, st), "sample")
        _lib.check(lib.ctts_gpt_decode(h, 160, 1, st), "warm")
        ms = C.c_float(0)
        _lib.check(lib.ctts_gpt_time_decode(h, 200, C.byref(ms), st), "time")          # steps 161 .. 360: mean context 48 + 261
        if collect is not None:
            collect.setdefault(("step", mode, B), []).append(ms.value)
            continue
        emit({"probe": "step", "mode": mode, "rows": B, "mean_ctx": 48 + 261, "ms_per_step": round(ms.value, 4)})


def prompt_times(g, mode, collect=None):
    lib, h = g._lib, g._h
    for B, T in ((32, 512), (8, 56), (1, 96)):
        emb, sc, io, st, msk, bufs = begin(g, B, T, 16)
        best = None
        for rep in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
            _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
            e1.record()
            torch.cuda.synchronize(dev)
            if rep:
                best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
        if collect is not None:
            collect.setdefault(("prompt", mode, (B, T)), []).append(best)
            continue
        emit({"probe": "prompt", "mode": mode, "B": B, "T": T, "ms": round(best, 3)})


def request(mode, options):
    from chatttsplus_amd.hip_models import Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams
    texts, limits, spk_index = bench._request_256(256)
    table = torch.from_numpy(np.stack([synth.speaker_vector(1234 + i) for i in range(4)]))
    params = InferCodeParams(prompt="[speed_5]", max_new_token=512, min_new_token=512, show_tqdm=False)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 512 + 64, device=str(dev), max_batch=32)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234)); syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    runs = {}
    for rows in (32, 16, 8):
        g = GPT(bench.LLAMA, max_batch=rows, max_seq_len=48 + 96 + 512 + 32, weight_dtype=DTYPE, device=str(dev), options=dict(options))
        g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
        with tempfile.TemporaryDirectory() as td:
            pipe = ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(td), dev)
            for order in ("longest_first", "input"):
                pipe.throughput_order = order
                walls = []
                for rep in range(2):                 # rep 0 captures the decode graphs
                    ids = []
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    pipe.infer_sharded(list(texts), speaker_index=spk_index, speaker_table=table, params_infer_code=params, noise_seed=4242, slice_size=rows,
                                       continuous=True, max_new_tokens_per_utterance=limits, ids_out=ids)
                    torch.cuda.synchronize(dev)
                    walls.append(time.perf_counter() - t0)
                runs[(rows, order)] = ([t.cpu() for t in ids], walls[-1])
        g.close()
    ref = runs[(32, "longest_first")][0]
    for (rows, order), (ids, wall) in runs.items():
        same = sum(bool(torch.equal(a, b)) for a, b in zip(ref, ids))
        emit({"probe": "request", "dtype": DTYPE, "mode": mode, "rows": rows, "order": order, "utterances": len(ids), "useful_tok_per_s": round(sum(limits) / wall, 1),
              "wall_s": round(wall, 3), "identical_to_32_rows_longest_first": same})


FP16_ROWS = (1, 2, 4, 5, 6, 8, 9, 16, 17, 32, 33, 56, 57, 64, 128)


def main_fp16():
    modes = (("default", {}), ("schedule_invariant", {"schedule_invariant": 1}))
    engines = {}
    for mode, options in modes:
        engines[mode] = GPT(bench.LLAMA, max_batch=128, max_seq_len=1024, weight_dtype="fp16", device=str(dev), options=dict(options))
        engines[mode].load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    got = {}
    for rnd in range(3):
        for mode, _ in modes:
            step_times(engines[mode], mode, FP16_ROWS, got)
            prompt_times(engines[mode], mode, got)
    for g in engines.values():
        g.close()
    for (probe, mode, what), v in got.items():
        v = sorted(v)
        rec = {"probe": probe, "dtype": "fp16", "mode": mode}
        rec.update({"rows": what, "mean_ctx": 48 + 261} if probe == "step" else {"B": what[0], "T": what[1]})
        rec.update({("ms_per_step" if probe == "step" else "ms"): round(v[1], 4), "min": round(v[0], 4), "max": round(v[2], 4), "rounds": 3})
        emit(rec)
    if "--skip-request" not in sys.argv:
        for mode, options in modes:
            request(mode, options)


def main():
    if DTYPE == "fp16":
        return main_fp16()
    for mode, options in (("default", {}), ("batch_invariant", {"batch_invariant": 1})):
        g = GPT(bench.LLAMA, max_batch=64, max_seq_len=1024, weight_dtype="fp32", device=str(dev), options=dict(options))
        g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
        step_times(g, mode)
        prompt_times(g, mode)
        g.close()
        if "--skip-request" not in sys.argv:
            request(mode, options)


if __name__ == "__main__":
    main()
