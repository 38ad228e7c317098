"""Text rows beside code rows (ctts_gpt_enable_text_rows; GPT.open_session(text_rows=...), ChatTTSPlusPipeline.open_session(refine=...)): what a mixed step costs and
what refining inside the session buys (report, not a gate).

Writes profiles/text_rows_probe.jsonl (synthetic weights at real size, 20 layers, fp32 engine, max_batch 32, toy tokenizer).
  (a) step    GPU ms per decode step (ctts_gpt_time_decode, 64 steps) at 1 / 8 / 32 rows with 0 and with 1 text row among them, alternating in one process, medians
              of three (spread = max - min).  The added cost is recorded next to a bound derived from the project's own numbers: the text head's weight bytes
              (21178 x 768 x 4) at the float4 copy rate README's shared-prompt paragraph states (6.29 TB/s), plus two launches at the per-launch price of
              profiles/mlp_lora_probe.jsonl (decode, all targets: ("launch" - "fold") / 40 launches at that row count).  The text sampler's own selection
              (one 21178-way row) is not part of that bound; no threshold is fixed.
  (b) latency submit-to-audio time of the session probe's arrival schedule (tools/session_probe.py, keyed by decode steps launched) with every utterance refined,
              in one refining SynthSession -- against what a service had to do before: drain and close the session, infer(refine_text_only=True) for the arrived
              texts, reopen, submit the refined texts.  Alternating, medians of three.
  dispatch    the two samplers, the code heads' launch and the text head's launch at 1 / 8 / 32 rows, per dispatch from `rocprofv3 --kernel-trace --stats` runs of this
              program's --child mode (the program goes after `--`); the text head is told from the code heads by its place in the step, not by its name (one
              kernel instantiation serves both); skipped with --no-trace or without rocprofv3

    python tools/text_rows_probe.py [--out profiles/text_rows_probe.jsonl] [--no-trace] [--no-latency]
"""
import argparse
import csv
import ctypes as C
import glob
import importlib.util
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

from chatttsplus_amd import _lib, synth                            # noqa: E402
from chatttsplus_amd.hip_models import GPT, Synth                  # noqa: E402
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects   # noqa: E402

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
ROWS, MAX_NEW, TXT_NEW, T = 32, 128, 48, 24
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
TEXT_HEAD_BYTES, COPY_TBS = 21178 * 768 * 4, 6.29


def engine(max_seq=T + MAX_NEW + 8):
    g = GPT(LLAMA, max_batch=ROWS, max_seq_len=max_seq, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return g


def per_launch_us():
    """{rows: us per launch} from profiles/mlp_lora_probe.jsonl: decode, adapters on all targets, the 40 launches "launch" mode runs more than "fold" """
    ms = {}
    for line in open(os.path.join(ROOT, "profiles", "mlp_lora_probe.jsonl")):
        r = json.loads(line)
        if r.get("leg") == "decode" and r.get("dtype") == "fp32" and r.get("targets") == "all" and r.get("mode") in ("launch", "fold"):
            ms[(r["rows"], r["mode"])] = r["ms"]                   # (the file's last such rows win)
    return {b: (ms[(b, "launch")] - ms[(b, "fold")]) * 1e3 / 40 for b in (1, 8, 32) if (b, "launch") in ms and (b, "fold") in ms}


def step_ms(g, B, n_text, steps=64):
    """B live rows, the first n_text of them text rows, none of which can end within the timed steps; ms per step of ctts_gpt_time_decode"""
    lib, h, dev = g._lib, g._h, g.device
    ids, mask = synth.prompt_ids(B, T, synth.GPT_REAL["num_text_tokens"], 7)
    emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool)).contiguous()
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, MAX_NEW, MAX_NEW - 1, LW, LP, 4)
    tsc = sampler_cfg_from_objects(torch.tensor([0.7]), 21177, MAX_NEW, MAX_NEW - 1, LW, [], 4, infer_text=True)
    out = dict(ids=torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev), tids=torch.empty(B, MAX_NEW, 4, dtype=torch.int32, device=dev),
               fin=torch.zeros(B, dtype=torch.int32, device=dev), end=torch.zeros(B, dtype=torch.int32, device=dev))
    io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=5)
    modes = np.ascontiguousarray([1 if b < n_text else 0 for b in range(B)], dtype=np.int32)
    if n_text:
        _lib.check(lib.ctts_gpt_set_row_modes(h, modes.ctypes.data_as(C.c_void_p), B), "set_row_modes")
    try:
        _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    finally:
        lib.ctts_gpt_set_row_modes(h, None, 0)
    if n_text:
        _lib.check(lib.ctts_gpt_enable_text_rows(h, C.byref(tsc), out["tids"].data_ptr(), st), "enable_text_rows")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    _lib.check(lib.ctts_gpt_sample(h, st), "sample")
    ms = C.c_float(0)
    _lib.check(lib.ctts_gpt_time_decode(h, steps, C.byref(ms), st), "time_decode")
    torch.cuda.synchronize()
    assert int(out["end"].min()) >= steps, "a row ended inside the timed steps"
    return float(ms.value)


def step_rows():
    g = engine()
    launch = per_launch_us()
    rows = []
    try:
        for B in (1, 8, 32):
            for n_text in (0, 1):
                step_ms(g, B, n_text, 16)                          # warm-up: graphs captured
            runs = {0: [], 1: []}
            for _ in range(3):
                for n_text in (0, 1):
                    runs[n_text].append(step_ms(g, B, n_text))
            med = {k: statistics.median(v) for k, v in runs.items()}
            head_us = TEXT_HEAD_BYTES / (COPY_TBS * 1e12) * 1e6
            rows.append(dict(kind="ms_per_step", rows=B, text_rows_0=round(med[0], 4), text_rows_0_spread=round(max(runs[0]) - min(runs[0]), 4),
                             text_rows_1=round(med[1], 4), text_rows_1_spread=round(max(runs[1]) - min(runs[1]), 4), added_us=round((med[1] - med[0]) * 1e3, 2),
                             bound_us=round(head_us + 2 * launch.get(B, float("nan")), 2), bound_text_head_us=round(head_us, 2),
                             bound_per_launch_us=round(launch.get(B, float("nan")), 2)))
    finally:
        g.close()
    return rows


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------------------
def _session_probe():
    spec = importlib.util.spec_from_file_location("session_probe", os.path.join(ROOT, "tools", "session_probe.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def pipeline(tmp):
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    g = engine(max_seq=96 + MAX_NEW + 8)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * MAX_NEW + 64, device="cuda:0", max_batch=ROWS)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    return g, ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(os.path.join(tmp, "tok")), torch.device("cuda:0"))


def serve(pipe, texts, arrivals, lims, way):
    """one pass over the schedule; submit-to-audio ms by utterance"""
    from chatttsplus_amd.pipeline import InferCodeParams, RefineTextParams
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, max_new_token=MAX_NEW, min_new_token=8, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
    refine = RefineTextParams(prompt="[oral_2]", max_new_token=TXT_NEW, min_new_token=4, show_tqdm=False)
    lat, t_sub, utt_of = {}, {}, {}
    pending = list(arrivals)
    base = 0                                                       # decode steps launched by the sessions closed so far
    ses = pipe.open_session(params, seed=11, rows=ROWS, refine=refine if way == "session" else None)

    def collect(results):
        for tk, wav, cancelled in results:
            torch.cuda.synchronize()
            lat[utt_of[tk]] = (time.perf_counter() - t_sub[utt_of[tk]]) * 1e3

    try:
        skipped = 0
        while pending or not ses.session.book.idle():
            now = base + ses.session.launched + skipped
            arrived = []
            while pending and pending[0][0] <= now:
                arrived.append(pending.pop(0)[1])
            for u in arrived:
                t_sub[u] = time.perf_counter()
            if arrived and way == "session":
                for u in arrived:
                    utt_of[ses.submit(texts[u], utt_id=u, max_new_token=lims[u])] = u
            elif arrived:                                          # before: the engine runs one mode at a time -- drain, close, refine, reopen, submit
                collect(ses.drain())
                base += ses.session.launched
                ses.close()
                refined = list(pipe.infer([texts[u] for u in arrived], refine_text_only=True, params_refine_text=refine, params_infer_code=params, noise="device", noise_seed=11,
                                          utt_ids=list(arrived), continuous=True))[0]
                ses = pipe.open_session(params, seed=11, rows=ROWS)
                utt_of = {}
                for u, t in zip(arrived, refined):
                    utt_of[ses.submit(t, utt_id=u, max_new_token=lims[u])] = u
            collect(ses.poll())
            if pending and ses.session.book.idle():
                skipped = pending[0][0] - base - ses.session.launched
    finally:
        ses.close()
    return lat


def latency_rows():
    sp = _session_probe()
    arrivals, lims = sp.schedule()
    n = len(arrivals)
    texts = synth.toy_texts(n, 8, 30, seed=68)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        g, pipe = pipeline(tmp)
        try:
            for way in ("session", "before"):
                serve(pipe, texts, arrivals, lims, way)            # warm-up
            runs = {"session": [], "before": []}
            for _ in range(3):
                for way in ("session", "before"):
                    runs[way].append(serve(pipe, texts, arrivals, lims, way))
        finally:
            g.close()
    for way in ("session", "before"):
        stats = [dict(mean=statistics.mean(lat.values()), median=statistics.median(lat.values()), max=max(lat.values()), first=lat[0]) for lat in runs[way]]
        row = dict(kind="submit_to_audio_ms", way=way, utterances=n)
        for k in stats[0]:
            vals = [s[k] for s in stats]
            row[k] = round(statistics.median(vals), 3)
            row[k + "_spread"] = round(max(vals) - min(vals), 3)
        rows.append(row)
    return rows


def child(B):
    """--child B: 32 steps at B rows with one text row and without, twice; run under rocprofv3 by the parent"""
    g = engine()
    for n_text in (0, 1, 0, 1):
        step_ms(g, B, n_text, 32)
    g.close()


def _stat(kind, B, name, us):
    return dict(kind=kind, rows=B, kernel=name[:160], calls=len(us), mean_us=round(statistics.mean(us), 3), min_us=round(min(us), 3), max_us=round(max(us), 3))


def kernel_rows(keep=None):
    """Per DISPATCH, from the kernel trace (the stats table cannot tell the text head from the code heads: both are one skinny_gemm_kernel instantiation under one
    name).  A mixed sample phase is the four consecutive dispatches code heads, text head, sampler_generate_kernel<true>, sampler_text_kernel: the text head is
    the dispatch right before the <true> sampler, the code heads the one before that; in an unmixed phase the code heads precede sampler_generate_kernel<false>
    (at <= 2 rows they are fused into the persistent launch: that dispatch is then the whole stack, and is left out)."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return []
    out = []
    for B in (1, 8, 32):
        with tempfile.TemporaryDirectory() as d:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", str(B)]
            subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if keep:
                os.makedirs(keep, exist_ok=True)
                for k, path in enumerate(paths):
                    shutil.copy(path, os.path.join(keep, f"rows{B}_{k}_kernel_trace.csv"))
            disp = []
            for path in paths:
                rd = csv.DictReader(open(path))
                cols = rd.fieldnames or []
                name_c = next((c for c in ("Kernel_Name", "Name") if c in cols), None)
                t0_c = next((c for c in ("Start_Timestamp", "Start") if c in cols), None)
                t1_c = next((c for c in ("End_Timestamp", "End") if c in cols), None)
                if not (name_c and t0_c and t1_c):
                    out.append(dict(kind="kernel_trace_error", rows=B, columns=cols))
                    continue
                disp += [(int(r[t0_c]), int(r[t1_c]), r[name_c]) for r in rd]
            disp.sort()
            acc = {}
            for k, (t0, t1, name) in enumerate(disp):
                us = (t1 - t0) / 1e3
                if "sampler_text_kernel" in name:
                    acc.setdefault(("text sampler (mixed step)", name), []).append(us)
                elif "sampler_generate_kernel<true>" in name:
                    acc.setdefault(("code sampler (mixed step)", name), []).append(us)
                    if k >= 2 and all("skinny_gemm" in disp[k - q][2] for q in (1, 2)):
                        acc.setdefault(("text head (mixed step)", disp[k - 1][2]), []).append((disp[k - 1][1] - disp[k - 1][0]) / 1e3)
                        acc.setdefault(("code heads (mixed step)", disp[k - 2][2]), []).append((disp[k - 2][1] - disp[k - 2][0]) / 1e3)
                        # what the sample phase of a mixed step occupies: first head's start to the text sampler's end
                        if k + 1 < len(disp) and "sampler_text_kernel" in disp[k + 1][2]:
                            acc.setdefault(("sample phase, heads to text sampler (mixed step)", "-"), []).append((disp[k + 1][1] - disp[k - 2][0]) / 1e3)
                elif "sampler_generate_kernel<false>" in name:
                    acc.setdefault(("code sampler (unmixed step)", name), []).append(us)
                    if k >= 1 and "skinny_gemm" in disp[k - 1][2]:
                        acc.setdefault(("code heads (unmixed step)", disp[k - 1][2]), []).append((disp[k - 1][1] - disp[k - 1][0]) / 1e3)
                        acc.setdefault(("sample phase, heads to code sampler (unmixed step)", "-"), []).append((t1 - disp[k - 1][0]) / 1e3)
            out += [_stat("dispatch: " + what, B, name, us) for (what, name), us in acc.items()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/text_rows_probe.jsonl")
    ap.add_argument("--child", type=int, default=0, metavar="ROWS")
    ap.add_argument("--keep-trace", metavar="DIR", help="copy the kernel-trace CSVs there")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    rows = [dict(note="fp32 20-layer engine, max_batch 32; (a) ctts_gpt_time_decode over 64 steps, 0 / 1 text row among 1 / 8 / 32 live rows, alternating, medians of "
                      "three, spread = max - min; bound = text head bytes at 6.29 TB/s + 2 launches at the per-launch price of profiles/mlp_lora_probe.jsonl; "
                      "(b) the session probe's arrival schedule, every utterance refined: one refining SynthSession vs drain + close + "
                      "infer(refine_text_only=True) + reopen + submit")]
    rows += step_rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    if not args.no_latency:
        for r in latency_rows():
            rows.append(r)
            print(json.dumps(r), flush=True)
    if not args.no_trace:
        for r in kernel_rows(args.keep_trace):
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
