"""Per-token log-probs written by the sampler during generate() (ctts_gpt_set_logprob_out, ctts_sampler_run_rows_lp; GPT.generate(return_logprobs=True);
ChatTTSPlusPipeline.infer(return_details / num_candidates)).  Synthetic weights at real widths, 4 decoder layers, as tests/test_gpu_score.py builds them.

The CPU reference of the processed distribution (`ref_probs`) follows oracle.ref_cpu.sample_step up to F.softmax(logits) with ref_cpu's own pieces and is
evaluated in float32 and in float64; a comparison's tolerance is 16 x the largest difference between those two evaluations on the same inputs (the factor
covers another expf and another reduction order), computed inside the test from the reference alone.

Worst differences observed on an MI355X (test 1, 8 sets x 128 rows; the tolerances computed for those sets in brackets):
    lp_raw      9.5e-7  (6.1e-6 .. 9.3e-6)
    lp_sampled  9.5e-7  (5.0e-6 .. 3.5e-5, the widest at temperature 3e-4, where the observed difference is 3.7e-9); 0 rows of 1024 left out
Step by step through the engine (test 2): lp_raw 9.5e-7 (9.0e-6), lp_sampled 9.5e-7 (1.0e-5).  Against the oracle model (test 3): 2.4e-6 on the fp32 engine
(bound 2e-4), 1.7e-3 on the fp16 engine (FP16_TOL = 4e-3); against GPT.score 3.3e-6 on fp32 (bound 2e-4: the decode-against-prompt-pass bound of
tests/test_gpu_score.py, which that file sets for fp32 engines) and 1.4e-3 on fp16, where decode and prompt pass round their activations and KV to fp16 along
different paths and each is only known to lie within FP16_TOL of the oracle: that comparison is held to FP16_TOL.  generate_many against batch 1: 3.3e-6
(bound 2e-5), 0 under batch_invariant.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs
from oracle import device_noise, ref_cpu
from tests.test_gpu_sampler import _cfg
from tests.test_gpu_score import CFG4, EOS, FP16_TOL, LLAMA4, engine, oracle_scores

pytestmark = pytest.mark.gpu

FILL = -7777.0
FACTOR = 16.0


# ---- the test-local reference ------------------------------------------------------------------------------------------------------------------
def ref_probs(logits, history, step, sp, temps, dtype):
    """ref_cpu.sample_step up to F.softmax(logits), in `dtype`: [rows, V] probabilities of the distribution the race draws from, and the kept set."""
    x = torch.as_tensor(logits).to(dtype) / torch.as_tensor(temps).to(dtype).view(-1, 1)                       # gpt.py:469
    hist = torch.as_tensor(history).to(torch.int64)
    if sp.repetition_penalty is not None and sp.repetition_penalty != 1 and hist.shape[1] > 0:
        x = ref_cpu.repetition_penalty(hist, x, sp.repetition_penalty, sp.max_input_ids, sp.past_window).to(dtype)
    if sp.top_p is not None:
        x = ref_cpu.top_p_warp(x, sp.top_p, sp.min_keep, stable=True)
    if sp.top_k is not None:
        x = ref_cpu.top_k_warp(x, sp.top_k, sp.min_keep)
    if step < sp.min_new_token:
        x = x.clone()
        x[:, sp.eos_token] = -torch.inf                                                                        # gpt.py:477-478
    return F.softmax(x, dim=-1), x > -torch.inf


def reference(logits, history, step, sp, temps, idx):
    """For the ids `idx`: (lp_raw32, tol_raw, lp_sampled32, tol_sampled, rows to compare lp_sampled on).  The tolerances are FACTOR x the largest
    float32-vs-float64 difference of the reference itself; a row is left out of the lp_sampled comparison only if the two evaluations keep different sets."""
    lg = torch.as_tensor(logits)
    ix = torch.as_tensor(idx).to(torch.int64).view(-1, 1)
    raw32 = torch.log_softmax(lg.float(), -1).gather(1, ix)[:, 0]
    raw64 = torch.log_softmax(lg.double(), -1).gather(1, ix)[:, 0]
    p32, kept32 = ref_probs(logits, history, step, sp, temps, torch.float32)
    p64, kept64 = ref_probs(logits, history, step, sp, temps, torch.float64)
    same = (kept32 == kept64).all(1)
    s32 = torch.log(p32.gather(1, ix)[:, 0])
    s64 = torch.log(p64.gather(1, ix)[:, 0])
    tol_raw = FACTOR * float((raw32.double() - raw64).abs().max())
    d = (s32.double() - s64)[same]
    tol_s = FACTOR * float(d[torch.isfinite(d)].abs().max()) if bool(torch.isfinite(d).any()) else 0.0
    return raw32, tol_raw, s32, tol_s, same


def knob_of(sc):
    k = _lib.RowSampling()
    for i in range(4):
        k.temperature[i] = sc.temperature[i]
    k.top_p_threshold, k.top_k, k.min_tokens_to_keep, k.use_penalty = sc.top_p_threshold, sc.top_k, sc.min_tokens_to_keep, sc.use_penalty
    for i in range(17):
        k.penalty_table[i] = sc.penalty_table[i]
    k.past_window, k.min_new_token, k.reserved = sc.past_window, sc.min_new_token, 0
    return k


def run_rows_lp(sc, logits, history, q, step, want=(True, True)):
    lib = _lib.load()
    dev = torch.device("cuda")
    rows, V = logits.shape
    lg, qq = torch.from_numpy(logits).to(dev), torch.from_numpy(q).to(dev)
    hs = torch.from_numpy(history.astype(np.int32)).to(dev).contiguous()
    idx = torch.zeros(rows, dtype=torch.int32, device=dev)
    lpr = torch.full((rows,), FILL, device=dev)
    lps = torch.full((rows,), FILL, device=dev)
    arr = (_lib.RowSampling * (rows // 4))(*[knob_of(sc)] * (rows // 4))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ctts_sampler_run_rows_lp(C.byref(sc), arr, lg.data_ptr(), hs.data_ptr(), history.shape[1], qq.data_ptr(), rows, V, int(step), idx.data_ptr(),
                                            lpr.data_ptr() if want[0] else None, lps.data_ptr() if want[1] else None, st), "sampler_run_rows_lp")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), lpr.cpu(), lps.cpu()


# ---- 1. the sampler alone, on identical logits -----------------------------------------------------------------------------------------------
SETS = [(0.3, 0.7, 20, 1.05, 0.55, 0), (0.0003, 0.7, 20, 1.05, 0.55, 0), (1.0, 0.9, 50, 1.3, 2.0, 0), (0.7, 0.3, 3, 1.0, 4.0, 0),
        (1.0, 0.99, 200, 1.0, 0.5, 0), (1.0, None, None, 1.1, 0.5, 0), (0.5, 0.5, None, 1.0, 0.3, 0),
        (0.3, 0.7, 20, 1.05, 0.55, 30)]           # min_new_token above the step (23): EOS, planted as the likely winner, is out of the race


@pytest.mark.parametrize("temp,top_p,top_k,rep,scale,min_new", SETS)
def test_sampler_logprobs_vs_reference(temp, top_p, top_k, rep, scale, min_new):
    rng = np.random.Generator(np.random.Philox(key=99))            # the input recipe of test_sampler_random_rows_vs_oracle
    rows = 128
    logits = (rng.standard_normal((rows, 626)) * scale).astype(np.float32)
    history = rng.integers(0, 626, size=(rows, 23), dtype=np.int64)
    history[:, -4:] = history[:, -5:-4]
    for r in range(rows):
        logits[r, history[r, -1]] += 2.0 * scale
    q = (-np.log1p(-rng.random((rows, 626)))).astype(np.float32).clip(min=1e-30)
    if min_new:
        logits[:, 625] += 3.0 * scale
    sp = ref_cpu.SamplerParams(temperature=[temp] * 4, top_p=top_p, top_k=top_k, repetition_penalty=rep, min_new_token=min_new)
    temps = torch.full((rows, 1), temp, dtype=torch.float32)
    ref_idx = ref_cpu.sample_step(torch.from_numpy(logits), torch.from_numpy(history), torch.from_numpy(q), 23, sp, temps).numpy()
    sc = _cfg(np.float32(temp), top_p, top_k, rep, min_new)
    idx, lpr, lps = run_rows_lp(sc, logits, history, q, 23)
    assert np.array_equal(idx, ref_idx.astype(np.int32)), f"{(idx != ref_idx).sum()} of {rows} ids differ"
    if min_new:
        assert not (idx == 625).any()
    raw32, tol_raw, s32, tol_s, same = reference(logits, history, 23, sp, temps, idx)
    d_raw = float((lpr - raw32).abs().max())
    d_s = float((lps - s32)[same].abs().max())
    print(f"set {(temp, top_p, top_k, rep, min_new)}: lp_raw max diff {d_raw:.3e} (tol {tol_raw:.3e}); lp_sampled max diff {d_s:.3e} (tol {tol_s:.3e}); "
          f"{int((~same).sum())} of {rows} rows left out")
    assert int((~same).sum()) <= 0.02 * rows
    assert torch.isfinite(lpr).all() and torch.isfinite(lps[same]).all()
    assert d_raw <= tol_raw
    assert d_s <= tol_s
    # either output alone: the same values, the other buffer untouched
    i2, r2, s2 = run_rows_lp(sc, logits, history, q, 23, want=(True, False))
    assert np.array_equal(i2, idx) and torch.equal(r2, lpr) and bool((s2 == FILL).all())
    i3, r3, s3 = run_rows_lp(sc, logits, history, q, 23, want=(False, True))
    assert np.array_equal(i3, idx) and torch.equal(s3, lps) and bool((r3 == FILL).all())


# ---- the engine, driven through the C ABI --------------------------------------------------------------------------------------------------------
class Call:
    """begin [+ set_logprob_out] + prefill on engine g; sample() / decode(n) advance it.  lp: "on", "null" (both pointers NULL) or None (no set call)."""

    def __init__(self, g, B, T, max_new, seed, lp="on", pad_left=None, temperature=0.3, min_new=2, warpers=True, rep=1.05, prompt_seed=71, knobs=None):
        self.g, self.B = g, B
        ids, mask = synth.prompt_ids(B, T, CFG4["num_text_tokens"], prompt_seed, pad_left=pad_left or [0] * B)
        emb = g(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool)).contiguous()
        dev = g.device
        lw = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()] if warpers else []
        lp_ = [type("R", (), dict(penalty=rep, past_window=16, max_input_ids=625))()] if rep != 1 else []
        self.sc = sampler_cfg_from_objects(torch.tensor([temperature] * 4), EOS, max_new, min_new, lw, lp_, 4)
        self.ids = torch.full((B, max_new, 4), -1, dtype=torch.int32, device=dev)
        self.hid = torch.zeros(B, max_new, 768, device=dev)
        self.fin = torch.zeros(B, dtype=torch.int32, device=dev)
        self.end = torch.zeros(B, dtype=torch.int32, device=dev)
        self.lpr = torch.full((B, max_new, 4), FILL, device=dev)
        self.lps = torch.full((B, max_new, 4), FILL, device=dev)
        io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr(), finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(), noise=None, n_draws=0,
                        seed=seed)
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
        lib, h = g._lib, g._h
        if knobs is not None:
            _lib.check(lib.ctts_gpt_set_row_sampling(h, knobs, B), "set_row_sampling")
        try:
            _lib.check(lib.ctts_gpt_begin(h, B, T, self.msk.data_ptr(), C.byref(self.sc), C.byref(io), self.st), "begin")
        finally:
            if knobs is not None:
                lib.ctts_gpt_set_row_sampling(h, None, 0)
        if lp == "on":
            _lib.check(lib.ctts_gpt_set_logprob_out(h, self.lpr.data_ptr(), self.lps.data_ptr(), self.st), "set_logprob_out")
        elif lp == "null":
            _lib.check(lib.ctts_gpt_set_logprob_out(h, None, None, self.st), "set_logprob_out")
        _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), self.st), "prefill")

    def sample(self):
        _lib.check(self.g._lib.ctts_gpt_sample(self.g._h, self.st), "sample")

    def decode(self, n, graph=0):
        _lib.check(self.g._lib.ctts_gpt_decode(self.g._h, n, graph, self.st), "decode")

    def state(self):
        torch.cuda.synchronize()
        return self.ids.cpu(), self.hid.cpu(), self.fin.cpu().tolist(), self.end.cpu().tolist()


def _walk(g, B, T, max_new, seed, pad_left, sp, temperature, warpers, rep, min_new):
    """Steps a call one token at a time; after every step the stored lp_raw / lp_sampled of the rows that were live equal the reference on that step's
    logits (history = the ids so far).  Returns the Call and the worst differences."""
    c = Call(g, B, T, max_new, seed, pad_left=pad_left, temperature=temperature, min_new=min_new, warpers=warpers, rep=rep)
    temps = torch.full((B * 4, 1), temperature, dtype=torch.float32)
    live = [True] * B
    worst = [0.0, 0.0, 0.0, 0.0]
    for step in range(max_new):
        c.sample() if step == 0 else c.decode(1)
        torch.cuda.synchronize()
        logits = g.last_logits(B).cpu().reshape(B * 4, 626)
        ids = c.ids.cpu()
        idx = ids[:, step].reshape(-1).to(torch.int64)
        history = ids[:, :step].permute(0, 2, 1).reshape(B * 4, step).to(torch.int64)
        sel = torch.tensor([live[b] for b in range(B) for _ in range(4)])
        if not bool(sel.any()):
            break
        raw32, tol_raw, s32, tol_s, same = reference(logits[sel], history[sel], step, sp, temps[sel], idx[sel])
        lpr = c.lpr[:, step].cpu().reshape(-1)[sel]
        lps = c.lps[:, step].cpu().reshape(-1)[sel]
        d_raw, d_s = float((lpr - raw32).abs().max()), float((lps - s32)[same].abs().max()) if bool(same.any()) else 0.0
        assert d_raw <= tol_raw, f"step {step}: lp_raw differs by {d_raw} (tolerance {tol_raw})"
        assert d_s <= tol_s, f"step {step}: lp_sampled differs by {d_s} (tolerance {tol_s})"
        assert int((~same).sum()) <= max(1, int(0.02 * int(sel.sum())))
        worst = [max(worst[0], d_raw), max(worst[1], tol_raw), max(worst[2], d_s), max(worst[3], tol_s)]
        fin, end = c.fin.cpu().tolist(), c.end.cpu().tolist()
        for b in range(B):
            if live[b] and (fin[b] or end[b] >= max_new):
                live[b] = False
    return c, worst


def test_engine_step_by_step():
    g = engine(max_seq=512)
    sp = ref_cpu.SamplerParams(temperature=[0.3] * 4, top_p=0.7, top_k=20, repetition_penalty=1.05, min_new_token=2)
    c, worst = _walk(g, 2, 12, 24, 11, [0, 3], sp, 0.3, True, 1.05, 2)
    print(f"step by step, default knobs: lp_raw {worst[0]:.3e} (tol {worst[1]:.3e}), lp_sampled {worst[2]:.3e} (tol {worst[3]:.3e})")
    ids, _, fin, end = c.state()
    for b in range(2):
        n = end[b] + (1 if fin[b] else 0)
        assert bool((c.lpr[b, :n].cpu() != FILL).all()) and bool((c.lpr[b, n:].cpu() == FILL).all())


EOS_SEED = 5       # picked on the GPU: under this seed row 0 samples EOS well inside the 400 steps (asserted below)


def test_engine_eos_step_is_written_at_end_idx():
    """Temperature 1, top-P / top-K / penalty off: under the near-uniform synthetic heads a row samples EOS on one of its 4 codebooks about once in 160
    steps.  The step that samples EOS is written at end_idx, entries beyond it keep the caller's fill."""
    g = engine(max_seq=512)
    sp = ref_cpu.SamplerParams(temperature=[1.0] * 4, top_p=None, top_k=None, repetition_penalty=1.0, min_new_token=0)
    max_new = 400
    c, worst = _walk(g, 2, 12, max_new, EOS_SEED, [0, 3], sp, 1.0, False, 1.0, 0)
    print(f"step by step, temperature 1: lp_raw {worst[0]:.3e} (tol {worst[1]:.3e}), lp_sampled {worst[2]:.3e} (tol {worst[3]:.3e})")
    ids, _, fin, end = c.state()
    print(f"finish {fin} end_idx {end}")
    assert any(fin), "no row ended by EOS under this seed: the case no longer covers the EOS step"
    lpr, lps = c.lpr.cpu(), c.lps.cpu()
    for b in range(2):
        e = end[b]
        if fin[b]:
            assert e < max_new and bool((ids[b, e] == EOS).any()), "finish reports EOS but the step at end_idx holds none"
            assert bool((lpr[b, :e + 1] != FILL).all()) and bool((lps[b, :e + 1] != FILL).all())        # the EOS step is written, at end_idx
            assert bool((lpr[b, e + 1:] == FILL).all()) and bool((lps[b, e + 1:] == FILL).all())        # beyond it: the caller's fill
            assert bool((ids[b, e + 1:] == -1).all())
        else:
            assert e == max_new and bool((lpr[b] != FILL).all())


# ---- 3. against the oracle model ---------------------------------------------------------------------------------------------------------------
def _generate(g, B, T, pad_left, max_new, seed, min_new=4, prompt_seed=72, **kw):
    ids, mask = synth.prompt_ids(B, T, CFG4["num_text_tokens"], prompt_seed, pad_left=pad_left)
    tm = torch.ones(B, T, dtype=torch.bool)
    lw = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
    lp = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
    outs = list(g.generate(g(torch.from_numpy(ids), tm), torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS, attention_mask=torch.from_numpy(mask),
                           max_new_token=max_new, min_new_token=min_new, logits_warpers=lw, logits_processors=lp, return_hidden=True, noise="device", seed=seed,
                           **kw))
    return outs, torch.from_numpy(ids), torch.from_numpy(mask), tm


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_generate_logprobs_vs_oracle_and_score(dtype):
    g = engine(dtype)
    outs, ids, mask, tm = _generate(g, 3, 14, [0, 3, 6], 20, 17, return_logprobs=True)
    out = outs[-1]
    assert len(out.logprobs) == 3 and len(out.sampled_logprobs) == 3 and len(out.final_logprobs) == 3
    codes = [i.cpu() for i in out.ids]
    si = score_inputs(ids, mask, tm, codes, EOS, append_eos=False)
    ref = oracle_scores(si)
    res = g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
    tol = 2e-4 if dtype == "fp32" else FP16_TOL
    for b in range(3):
        lp = out.logprobs[b].cpu()
        assert lp.shape == codes[b].shape == out.sampled_logprobs[b].shape
        d_o = float((lp - ref[b][0]).abs().max())
        d_s = float((lp - res.logprob[b]).abs().max())
        print(f"{dtype} sequence {b}: |logprobs - oracle| {d_o:.3e}, |logprobs - GPT.score| {d_s:.3e}")
        assert d_o <= tol
        assert d_s <= (2e-4 if dtype == "fp32" else FP16_TOL)
        assert bool((out.sampled_logprobs[b] <= 0).all()) and bool(torch.isfinite(out.sampled_logprobs[b]).all())
        assert (out.final_logprobs[b] is None) or tuple(out.final_logprobs[b].shape) == (2, 4)


# ---- 4. nothing changes when off, nothing feeds back when on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 8, 12])
def test_off_on_null_bit_identical(B, graph):
    """1 row and 2 rows: the persistent launch with the heads inside; 8 rows: its two-item form; 12 rows: the launch chain.  The call with log-probs comes
    first and the ones without follow on the same engine, so with graphs the same captured graphs serve all three."""
    g = engine(max_batch=16)
    runs = {}
    for mode in ("on", None, "null"):
        c = Call(g, B, 10, 28, 23, lp=mode, pad_left=[b % 4 for b in range(B)], min_new=3)
        c.sample()
        c.decode(27, graph)
        runs[mode] = c.state()
        if mode == "on":
            n = [e + (1 if f else 0) for f, e in zip(runs[mode][2], runs[mode][3])]
            assert all(bool((c.lpr[b, :n[b]].cpu() != FILL).all()) and bool((c.lps[b, n[b]:].cpu() == FILL).all()) for b in range(B))
        else:
            assert bool((c.lpr == FILL).all()) and bool((c.lps == FILL).all())
    for mode in ("on", "null"):
        for k, name in enumerate(("ids", "hiddens", "finish", "end_idx")):
            a, b = runs[mode][k], runs[None][k]
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b, f"{name} differ between no request and {mode}"


# ---- 5. serving paths ------------------------------------------------------------------------------------------------------------------------------
N_UTT, ROWS, T_MAX, SEED5 = 10, 4, 14, 777
HOT = dict(temperature=1e4, top_P=None, top_K=None, repetition_penalty=1.0, min_new_token=0)      # (near-)uniform draws: the winner is the smallest noise


@functools.lru_cache(maxsize=None)
def _restart_uid():
    """An utterance id whose step-0 draw is EOS on some codebook at attempt 0 (ensure_non_empty restarts it) and on none at attempt 1, by a clear margin
    of the device noise (oracle/device_noise.py), under the HOT knobs."""
    for uid in range(1000, 3000):
        first = [device_noise.exp_noise(SEED5, uid, vq, 0, 0, 626) for vq in range(4)]
        again = [device_noise.exp_noise(SEED5, uid, vq, 0, 1, 626) for vq in range(4)]
        clear = all(np.sort(q)[1] > 1.05 * np.sort(q)[0] for q in first + again)
        if clear and any(int(q.argmin()) == EOS for q in first) and not any(int(q.argmin()) == EOS for q in again):
            return uid
    raise AssertionError("no such id")


def _request():
    rng = np.random.Generator(np.random.Philox(key=515))
    lens = [int(x) for x in rng.integers(6, T_MAX + 1, size=N_UTT)]
    lims = [int(x) for x in rng.integers(6, 25, size=N_UTT)]
    ids, mask = synth.prompt_ids(N_UTT, T_MAX, CFG4["num_text_tokens"], seed=515, pad_left=[T_MAX - x for x in lens])
    uids = list(range(N_UTT))
    uids[6] = _restart_uid()
    per = [None] * N_UTT
    per[6] = dict(HOT)
    return lens, lims, ids, mask, uids, per


def _many(g, progress=False):
    lens, lims, ids, mask, uids, per = _request()
    emb = g(torch.from_numpy(ids), torch.ones(N_UTT, T_MAX, dtype=torch.bool))
    lw = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
    lp = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
    kw = dict(attention_mask=torch.from_numpy(mask), max_new_token=24, min_new_token=2, logits_warpers=lw, logits_processors=lp, return_hidden=True, seed=SEED5,
              utt_ids=uids, max_new_tokens_per_row=lims, sampling_per_row=per, return_logprobs=True)
    if not progress:
        return g.generate_many(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS, rows=ROWS, **kw)
    events = []
    gen = g.generate_many_iter(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS, rows=ROWS, progress=True, **kw)
    try:
        while True:
            events.append(next(gen))
    except StopIteration as stop:
        return stop.value, events


def _alone(g, u):
    lens, lims, ids, mask, uids, per = _request()
    T = lens[u]
    i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:])
    lw = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
    lp = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
    return list(g.generate(g(i1, torch.ones(1, T, dtype=torch.bool)), i1, torch.tensor([0.3] * 4), EOS, attention_mask=torch.from_numpy(mask[u:u + 1, T_MAX - T:]),
                           max_new_token=24, min_new_token=2, logits_warpers=lw, logits_processors=lp, return_hidden=True, noise="device", seed=SEED5,
                           utt_ids=[uids[u]], max_new_tokens_per_row=[lims[u]], sampling_per_row=[per[u]], return_logprobs=True))[-1]


@pytest.mark.parametrize("invariant", [False, True])
def test_generate_many_logprobs_equal_batch_1(invariant):
    g = engine(options=dict(batch_invariant=1) if invariant else None)
    out = _many(g)
    assert len(g.admissions) >= 1, "the request was meant to re-use rows"
    worst = 0.0
    for u in range(N_UTT):
        one = _alone(g, u)
        assert torch.equal(out.ids[u].cpu(), one.ids[0].cpu()), f"utterance {u}: token ids differ from its batch-1 run"
        assert out.ids[u].shape[0] >= 1 and not bool((out.ids[u] == EOS).any())
        for name in ("logprobs", "sampled_logprobs"):
            a, b = getattr(out, name)[u].cpu(), getattr(one, name)[0].cpu()
            assert a.shape == tuple(out.ids[u].shape)
            if invariant:
                assert torch.equal(a, b), f"utterance {u}: {name} not bit-identical under batch_invariant"
            else:
                d = float((a - b).abs().max())
                worst = max(worst, d)
                assert d <= 2e-5, f"utterance {u}: {name} differ by {d} from the batch-1 run"
        fa, fb = out.final_logprobs[u], one.final_logprobs[0]
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert float((fa.cpu() - fb.cpu()).abs().max()) <= (0.0 if invariant else 2e-5)
    print(f"generate_many vs batch 1 (invariant={invariant}): worst log-prob difference {worst:.3e}")


def test_streamed_partial_logprobs_are_prefixes():
    g = engine()
    outs, *_ = _generate(g, 2, 12, [0, 2], 24, 31, min_new=24, return_logprobs=True, stream=True, stream_batch=4)
    assert len(outs) >= 4
    final = outs[-1]
    for part in outs[:-1]:
        for b in range(2):
            n = part.ids[b].shape[0]
            assert part.logprobs[b].shape[0] == n and torch.equal(part.logprobs[b].cpu(), final.logprobs[b][:n].cpu())
            assert torch.equal(part.sampled_logprobs[b].cpu(), final.sampled_logprobs[b][:n].cpu())
    res, events = _many(g, progress=True)
    seen = 0
    for ev in events:
        items = ev[1] if isinstance(ev, tuple) and ev[0] == "progress" else ev
        for item in items:
            u, o = item[0], item[-1]
            n = o.ids[0].shape[0]
            assert torch.equal(o.ids[0].cpu(), res.ids[u][:n].cpu()) and torch.equal(o.logprobs[0].cpu(), res.logprobs[u][:n].cpu())
            assert torch.equal(o.sampled_logprobs[0].cpu(), res.sampled_logprobs[u][:n].cpu())
            seen += 1
    assert seen >= N_UTT


# ---- 6. candidates ---------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_candidates(tmp_path):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, InferDetails, select_candidate
    g = GPT(LLAMA4, max_batch=8, max_seq_len=160, weight_dtype="fp32", options=dict(batch_invariant=1))
    g.load_state_dict(synth.gpt_state_dict(CFG4, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    pipe = ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(str(tmp_path / "tok")), torch.device("cuda:0"))
    texts = synth.toy_texts(2, 8, 30, seed=67)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=32, min_new_token=4, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())

    def run(**kw):
        sink = []
        out = list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", noise_seed=4242, slice_size=8, _ids_sink=sink, **kw))
        return out, [i.cpu() for _, i in sorted(sink, key=lambda t: t[0])]

    try:
        plain, plain_ids = run()
        one, one_ids = run(num_candidates=1)
        assert all(torch.equal(a, b) for a, b in zip(plain_ids, one_ids))
        assert all(torch.equal(a, b) for wa, wb in zip(plain, one) for a, b in zip(wa, wb)), "num_candidates=1 is the plain call, bit for bit"
        out, win_ids = run(num_candidates=4, return_details=True)
        assert len(out) == 1 and isinstance(out[0], InferDetails)
        d = out[0]
        for u in range(2):
            cands = d.candidates[u]
            assert torch.equal(cands[0].ids.cpu(), plain_ids[u]), "candidate 0 is the plain generation"
            assert not all(torch.equal(c.ids.cpu(), cands[0].ids.cpu()) for c in cands[1:]), "the four candidates are all equal"
            assert d.candidate[u] == select_candidate(d.candidate_scores[u].tolist()) == int(d.candidate_scores[u].argmax())
            assert torch.equal(d.ids[u].cpu(), cands[d.candidate[u]].ids.cpu()) and torch.equal(win_ids[u], d.ids[u].cpu())
            assert d.mean_logprob[u] == pytest.approx(float(d.candidate_scores[u][d.candidate[u]]))
            assert d.wavs[u].shape[0] == 256 * (2 * d.ids[u].shape[0] - 1)
            served = texts[u] if texts[u].strip().endswith("[uv_break]") else texts[u] + " [uv_break]"      # what infer() hands the code pass (pipeline:414-416)
            sc = pipe.score([served] * 4, codes=[c.ids.cpu() for c in cands], params_infer_code=params, append_eos=False)
            for k in range(4):
                diff = abs(float(d.candidate_scores[u][k]) + float(sc.nll[k]))
                print(f"utterance {u} candidate {k}: score {float(d.candidate_scores[u][k]):.6f}, -nll {-float(sc.nll[k]):.6f}")
                assert diff <= 2e-4
        for u in range(2):
            if d.candidate[u] == 0:      # the plain generation won: its waveform is the plain call's
                a, b = d.wavs[u].cpu().numpy(), plain[0][u].cpu().numpy()
                assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-4
        picked, _ = run(num_candidates=4, return_details=True, select=lambda c: 2)
        assert picked[0].candidate == [2, 2] and all(torch.equal(picked[0].ids[u].cpu(), d.candidates[u][2].ids.cpu()) for u in range(2))
        # refusals, each with a message
        for kw, msg in ((dict(num_candidates=2, stream=True), "stream=False"), (dict(num_candidates=2, utt_ids=[0, 1 << 48]), r"not below 2\^48")):
            with pytest.raises(_lib.HipBackendError, match=msg):
                list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", **kw))
        with pytest.raises(_lib.HipBackendError, match="device noise"):
            list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="torch", num_candidates=2))
        with pytest.raises(_lib.HipBackendError, match="infer_sharded"):
            pipe.infer_sharded(list(texts), params_infer_code=params, num_candidates=2)
    finally:
        g.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_logprob_errors():
    g = engine()
    lib, h = g._lib, g._h
    c = Call(g, 2, 10, 8, 3, lp=None)
    buf = torch.zeros(2, 8, 4, device=g.device)
    c.sample()
    assert lib.ctts_gpt_set_logprob_out(h, buf.data_ptr(), buf.data_ptr(), c.st) != 0
    assert b"after the first" in lib.ctts_last_error()
    c.decode(7)
    torch.cuda.synchronize()
    # the refine-text pass returns none
    sc = sampler_cfg_from_objects(torch.tensor([0.7]), 21177, 8, 0, [], [], 4, infer_text=True)
    io = _lib.GenIO(ids=c.ids.data_ptr(), hiddens=None, finish=c.fin.data_ptr(), end_idx=c.end.data_ptr(), noise=None, n_draws=0, seed=1)
    _lib.check(lib.ctts_gpt_begin(h, 2, 10, c.msk.data_ptr(), C.byref(sc), C.byref(io), c.st), "begin")
    assert lib.ctts_gpt_set_logprob_out(h, buf.data_ptr(), None, c.st) != 0
    assert b"infer_text" in lib.ctts_last_error()
    ids, mask = synth.prompt_ids(1, 8, CFG4["num_text_tokens"], 72)
    with pytest.raises(_lib.HipBackendError, match="infer_text"):
        list(g.generate(g(torch.from_numpy(ids), torch.ones(1, 8, dtype=torch.bool)), torch.from_numpy(ids), torch.tensor([0.7]), 21177,
                        attention_mask=torch.from_numpy(mask), max_new_token=4, infer_text=True, return_logprobs=True))
    # every begin resets the request: a plain call after one with log-probs writes nothing
    c1 = Call(g, 2, 10, 8, 3, lp="on"); c1.sample(); c1.decode(7)
    c2 = Call(g, 2, 10, 8, 3, lp=None); c2.sample(); c2.decode(7)
    torch.cuda.synchronize()
    assert bool((c1.lpr[:, 0] != FILL).all()) and bool((c2.lpr == FILL).all()) and bool((c2.lps == FILL).all())
    assert torch.equal(c1.ids, c2.ids)
    # host noise works too: torch's generator and a caller's array
    ids, mask = synth.prompt_ids(2, 12, CFG4["num_text_tokens"], 72, pad_left=[0, 2])
    for noise in ("torch", torch.empty(8 + 4, 8, 626).exponential_(1)):
        torch.manual_seed(5)
        o = list(g.generate(g(torch.from_numpy(ids), torch.ones(2, 12, dtype=torch.bool)), torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS,
                            attention_mask=torch.from_numpy(mask), max_new_token=8, min_new_token=8, noise=noise, return_logprobs=True))[-1]
        assert all(lp.shape == (8, 4) and bool(torch.isfinite(lp).all()) and bool((lp < 0).all()) for lp in o.logprobs)
        assert all(bool((s <= 0).all()) for s in o.sampled_logprobs)
