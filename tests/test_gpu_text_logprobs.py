"""Log-probs of the refine-text pass on the GPU (ctts_gpt_set_text_logprob_out, ctts_sampler_run_text_lp; sampler_text_kernel<GUIDED>;
generate(return_text_logprobs=True), open_session(text_rows=..., return_text_logprobs=True)).  Synthetic weights at real widths (V = 21178, H = 768), 4 decoder
layers, the prompt pool of tests/test_gpu_session.py (prompts <= 14 tokens), max_new_token <= 12.

Tolerance of test 1 (u = 2^-24, the unit round-off of fp32).  The kernel forms lp_raw = (lg[id] - mx) - logf(s), s = sum_j expf(lg[j] - mx) over 21178 terms:
every thread adds its 21 terms in order, wave_sum adds 64 partials in 6 levels, 16 wave partials are added in order -- a reduction DEPTH of 21 + 6 + 16 = 43
additions, all terms positive, so the sum carries a relative error of at most 43 u; each term carries (|lg[j] - mx| + 2) u (the rounded difference in the exponent,
expf to 2 ulp), which the sum weights by p_j: DRIFT = sum_j p_j |lg[j] - mx| (evaluated in float64 from the reference's own values); logf adds 2 u, the numerator
|lg[id] - mx| u, the final subtraction |lp| u:
    tol_raw = (43 + 8 + DRIFT + |lg[id] - mx| + |lp_raw|) u        (8: expf and logf to 2 ulp each, with margin for the rounded row maximum's own terms)
lp_sampled = logf(expf(x[id] - m2) * inv2) runs the same reductions over the kept set (at most 43 deep), plus the division 1 / s2 and the product (2 u):
    tol_sampled = (43 + 8 + DRIFT_kept + |x[id] - m2| + |lp_sampled|) u
At the logits of this test (N(0, 9): |lg - mx| <= 27; the stand-in row's id 0 sits at -30) the tolerances come to 3.0e-6 .. 8.4e-6.  Worst differences measured
on an MI355X over the three parameter sets (each test prints its own): lp_raw 6.6e-7 (largest tolerance 8.4e-6), lp_sampled 2.9e-7 (largest tolerance 3.5e-6);
in the mixed batches of test 3, default mode, text rows against their batch-1 calls: 3.8e-6 at 9 rows, 1.2e-6 at 3 rows (bound 2e-5), 0 under batch_invariant."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import (TextGuide, gen_logits, guide_allowed, guide_eos_removable, guide_standin, guide_step, sampler_cfg_from_objects)
from oracle import ref_cpu
from tests.test_gpu_score import EOS, engine
from tests.test_gpu_session import FILL_F, FILL_I, INV, LP, LW, SEED, T_MAX, TEXT_EOS, Raw, _pool

pytestmark = pytest.mark.gpu

V = 21178
U = 2.0 ** -24
DEPTH = 21 + 6 + 16
NEW, TNEW, TXT_T, TXT_MIN = 12, 10, 0.7, 1       # code / text max_new_token of the generate states below
FREE5 = [7, 1023, 1024, 5000, TEXT_EOS - 1]
NEG_INF = -float("inf")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- 1. the hook against a float64 restatement -----------------------------------------------------------------------------------------------------------
def cpu_step(logits, q, T, top_p, top_k, min_keep, min_new, eos, t, guide=None):
    """One step of the text sampler restated on the CPU: the float32 id-selection path of tests/test_gpu_text_guide.py (oracle.ref_cpu's warpers, softmax, race)
    over the allowed set of `guide` = dict(src, cur, run, limit, free, max_run), or over the whole row.  -> (idx, cur, run, x): x = the float32 row the race drew
    from (temperature, guide mask, top-P, top-K, min_new_token applied; -inf outside the kept set)."""
    if guide is not None:
        n = len(guide["src"])
        args = (guide["cur"], guide["run"], t, guide["limit"], n, guide["max_run"])
        A = guide_allowed(*args, guide["src"], guide["free"], eos)
        x = torch.full((1, logits.numel()), NEG_INF)
        x[0, A] = logits[A]
    else:
        x = logits.clone()[None]
    x = x / torch.tensor(float(T), dtype=torch.float32)
    if top_p is not None:
        x = ref_cpu.top_p_warp(x, top_p, min_keep)
    if top_k is not None:
        x = ref_cpu.top_k_warp(x, top_k, 1)
    if t < min_new and (guide is None or guide_eos_removable(*args, guide["free"])):
        x = x.clone()
        x[0, eos] = NEG_INF
    ratio = torch.softmax(x, dim=-1)[0] / q
    if guide is None:
        return int(torch.argmax(ratio)), 0, 0, x[0]
    ratio = torch.where(ratio > 0, ratio, torch.zeros_like(ratio))
    idx = int(torch.argmax(ratio)) if float(ratio.max()) > 0 else guide_standin(guide["cur"], n, guide["src"], eos)
    cur, run, _ = guide_step(*args, idx, src=guide["src"], eos=eos)
    return idx, cur, run, x[0]


def reference_lp(row, idx):
    """float64 log_softmax(row)[idx] of a float32 row and the tolerance derived in the module docstring; (-inf, 0) where the row is -inf at idx"""
    r = row.double()
    if not bool(torch.isfinite(r[idx])):
        return NEG_INF, 0.0
    mx = r.max()
    p = torch.softmax(r, -1)
    fin = torch.isfinite(r)
    drift = float((p[fin] * (r[fin] - mx).abs()).sum())
    lp = float(torch.log_softmax(r, -1)[idx])
    return lp, (DEPTH + 8 + drift + float((r[idx] - mx).abs()) + abs(lp)) * U


def run_lp_hook(sc, logits, q, rows, guided, free=(), max_run=0, want=(True, True)):
    """rows: [dict(step, limit[, src, cur, run])] -> (idx, cur, run, lp_raw, lp_sampled); want = which of the two log-prob buffers are passed"""
    lib = _lib.load()
    R = len(rows)
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    step, lim = arr([r["step"] for r in rows]), arr([r["limit"] for r in rows])
    cat = off = cur = run = co = ro = fr = None
    if guided:
        cat = arr([i for r in rows for i in r["src"]])
        off = arr(np.cumsum([0] + [len(r["src"]) for r in rows]))
        cur, run = arr([r["cur"] for r in rows]), arr([r["run"] for r in rows])
        co, ro = np.zeros(R, np.int32), np.zeros(R, np.int32)
        fr = arr(list(free) or [0])
    idx = np.full(R, -5, np.int32)
    raw = np.full(R, FILL_F, np.float32) if want[0] else None
    smp = np.full(R, FILL_F, np.float32) if want[1] else None
    lg, qq = logits.to("cuda:0").contiguous(), q.to("cuda:0").contiguous()
    st = C.c_void_p(torch.cuda.current_stream(lg.device).cuda_stream)
    rc = lib.ctts_sampler_run_text_lp(C.byref(sc), lg.data_ptr(), qq.data_ptr(), R, V, _ptr(fr), len(free), max_run, _ptr(cat), _ptr(off), _ptr(cur), _ptr(run),
                                      _ptr(step), _ptr(lim), _ptr(idx), _ptr(co), _ptr(ro), _ptr(raw), _ptr(smp), st)
    assert rc == 0, lib.ctts_last_error().decode()
    return idx.tolist(), None if co is None else co.tolist(), None if ro is None else ro.tolist(), raw, smp


HOOK_MIN_NEW, HOOK_MAX_RUN = 5, 2


@pytest.mark.parametrize("temp,top_p,top_k", [(0.7, 0.7, 20), (3e-4, 0.7, 20), (0.7, None, 1)])
def test_hook_against_float64_restatement(temp, top_p, top_k):
    """Cases: unguided and guided rows; a guided row at cur == n (only EOS allowed); temperature 3e-4; top_k = 1; min_new_token removing EOS (EOS carries the largest
    logit at a step below min_new_token); rows whose every ratio is 0 (q = +inf): the stand-in fires -- element 0, outside the kept set, lp_sampled == -inf on the
    unguided row; src[cur] on the guided row, lp_sampled -inf where the warpers removed it, else its finite log-probability.  Measured maxima are printed."""
    w, _ = gen_logits(0, top_P=top_p, top_K=top_k, repetition_penalty=None)
    sc = sampler_cfg_from_objects(torch.tensor([temp]), TEXT_EOS, 64, HOOK_MIN_NEW, w, [], 4, infer_text=True)
    min_keep = 3 if top_p is not None else 1
    tg = torch.Generator().manual_seed(777)
    rng = np.random.Generator(np.random.Philox(key=778))
    # unguided rows: (step, what)
    un = [dict(step=9, limit=40), dict(step=0, limit=40), dict(step=2, limit=40, eos_top=True), dict(step=9, limit=40, eos_top=True), dict(step=9, limit=40, zero=True),
          dict(step=9, limit=40), dict(step=39, limit=40), dict(step=9, limit=40)]
    R = len(un)
    lg_u = torch.randn(R, V, generator=tg) * 3.0
    q_u = torch.empty(R, V).exponential_(generator=tg)
    for r, c in enumerate(un):
        if c.get("eos_top"):
            lg_u[r, TEXT_EOS] = 20.0
        if c.get("zero"):
            q_u[r] = float("inf")
            lg_u[r, 0] = -30.0                     # element 0 is far outside the kept set
    src = [int(i) for i in rng.integers(2100, 20000, size=6)]
    gd = [dict(src=src, cur=2, run=0, step=9, limit=40), dict(src=src, cur=2, run=1, step=2, limit=40), dict(src=src, cur=0, run=0, step=0, limit=7),
          dict(src=src[:3], cur=3, run=0, step=9, limit=40), dict(src=src[:3], cur=3, run=0, step=3, limit=40), dict(src=src[:3], cur=3, run=1, step=9, limit=10),
          dict(src=src[:3], cur=3, run=HOOK_MAX_RUN, step=3, limit=40), dict(src=src, cur=2, run=0, step=9, limit=40, zero=True),
          dict(src=src, cur=2, run=HOOK_MAX_RUN, step=9, limit=40, zero=True), dict(src=src, cur=1, run=0, step=9, limit=40)]
    G = len(gd)
    lg_g = torch.randn(G, V, generator=tg) * 3.0
    q_g = torch.empty(G, V).exponential_(generator=tg)
    for r, c in enumerate(gd):
        if c.get("zero"):
            q_g[r] = float("inf")
    worst = {"raw": 0.0, "smp": 0.0, "tol_raw": 0.0, "tol_smp": 0.0}

    def check(name, r, lg, x, idx, raw, smp, standin=False):
        want_raw, tol_raw = reference_lp(lg, idx)
        want_smp, tol_smp = reference_lp(x, idx)
        d_raw = abs(float(raw[r]) - want_raw)
        print(f"{name} row {r}: id {idx} lp_raw {float(raw[r]):.6f} (ref {want_raw:.6f}, diff {d_raw:.2e}, tol {tol_raw:.2e}) lp_sampled {float(smp[r]):.6f} (ref {want_smp:.6f})")
        assert d_raw <= tol_raw, f"{name} row {r}: lp_raw off by {d_raw} (tolerance {tol_raw})"
        worst["raw"], worst["tol_raw"] = max(worst["raw"], d_raw), max(worst["tol_raw"], tol_raw)
        if want_smp == NEG_INF:
            assert float(smp[r]) == NEG_INF, f"{name} row {r}: id {idx} lies outside the kept set, lp_sampled is {float(smp[r])}"
        elif standin and want_smp < -87.0:          # a stand-in whose fp32 probability underflows: -inf or the finite value
            assert float(smp[r]) == NEG_INF or abs(float(smp[r]) - want_smp) <= tol_smp
        else:
            d = abs(float(smp[r]) - want_smp)
            assert d <= tol_smp, f"{name} row {r}: lp_sampled off by {d} (tolerance {tol_smp})"
            worst["smp"], worst["tol_smp"] = max(worst["smp"], d), max(worst["tol_smp"], tol_smp)

    # unguided
    idx, _, _, raw, smp = run_lp_hook(sc, lg_u, q_u, un, False)
    for wt in ((False, False), (True, False), (False, True)):
        assert run_lp_hook(sc, lg_u, q_u, un, False, want=wt)[0] == idx, f"unguided ids change with the log-prob buffers {wt}"
    for r, c in enumerate(un):
        want_idx, _, _, x = cpu_step(lg_u[r], q_u[r], temp, top_p, sc.top_k, min_keep, HOOK_MIN_NEW, TEXT_EOS, c["step"])
        assert idx[r] == want_idx, f"unguided row {r}: id {idx[r]}, the restatement draws {want_idx}"
        check("unguided", r, lg_u[r], x, idx[r], raw, smp)
        if c.get("zero"):
            assert idx[r] == 0 and float(smp[r]) == NEG_INF and np.isfinite(raw[r])
        if c.get("eos_top"):
            assert (idx[r] != TEXT_EOS) == (c["step"] < HOOK_MIN_NEW), f"unguided row {r}: min_new_token"
    # guided
    idx, cur, run, raw, smp = run_lp_hook(sc, lg_g, q_g, gd, True, FREE5, HOOK_MAX_RUN)
    for wt in ((False, False), (True, False), (False, True)):
        assert run_lp_hook(sc, lg_g, q_g, gd, True, FREE5, HOOK_MAX_RUN, want=wt)[:3] == (idx, cur, run), f"guided ids / cursors change with the log-prob buffers {wt}"
    for r, c in enumerate(gd):
        guide = dict(src=c["src"], cur=c["cur"], run=c["run"], limit=c["limit"], free=FREE5, max_run=HOOK_MAX_RUN)
        want_idx, wc, wr, x = cpu_step(lg_g[r], q_g[r], temp, top_p, sc.top_k, min_keep, HOOK_MIN_NEW, TEXT_EOS, c["step"], guide)
        assert (idx[r], cur[r], run[r]) == (want_idx, wc, wr), f"guided row {r}"
        check("guided", r, lg_g[r], x, idx[r], raw, smp, standin=bool(c.get("zero")))
        if c.get("zero"):
            assert idx[r] == c["src"][c["cur"]]
        if c["cur"] == len(c["src"]) and (c["run"] >= HOOK_MAX_RUN or c["limit"] - c["step"] <= 1):
            assert idx[r] == TEXT_EOS and float(smp[r]) == 0.0, f"guided row {r}: EOS alone is allowed, p = 1"
    print(f"T={temp} top_p={top_p} top_k={top_k}: max |lp_raw - ref| {worst['raw']:.3e} (largest tol {worst['tol_raw']:.3e}); "
          f"max |lp_sampled - ref| {worst['smp']:.3e} (largest tol {worst['tol_smp']:.3e})")


def test_hook_guided_lp_raw_uses_the_full_row():
    """lp_raw of a guided row equals, within the bound above, the lp_raw an unguided row gives for the same logits and id: the guided row loads <= 65 logits for
    the race but reduces its whole row for lp_raw.  The id is the row's own source id, raised into the unguided row's top-K so that both rows can return it
    (the unguided row's noise is 1 everywhere, 1e-6 at the id)."""
    sc = sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, 64, 0, LW, [], 4, infer_text=True)
    ids = [0, 1023, 1024, 2047, 20479, TEXT_EOS - 1]
    tg = torch.Generator().manual_seed(31)
    lg = torch.randn(len(ids), V, generator=tg) * 3.0
    q = torch.ones(len(ids), V)
    for r, i in enumerate(ids):
        lg[r, i] += 16.0
        q[r, i] = 1e-6
    un, _, _, raw_u, _ = run_lp_hook(sc, lg, q, [dict(step=3, limit=40)] * len(ids), False)
    gd, _, _, raw_g, smp_g = run_lp_hook(sc, lg, q, [dict(src=[i], cur=0, run=0, step=3, limit=40) for i in ids], True, [], 0)
    assert un == ids and gd == ids
    for r, i in enumerate(ids):
        want, tol = reference_lp(lg[r], i)
        print(f"id {i}: guided lp_raw {raw_g[r]:.7f} unguided {raw_u[r]:.7f} float64 {want:.7f} (tol {tol:.2e})")
        assert abs(float(raw_g[r]) - float(raw_u[r])) <= tol and abs(float(raw_g[r]) - want) <= tol
        assert float(smp_g[r]) == 0.0              # the allowed set is {id}: p = 1


# ---- generate states through the C ABI ------------------------------------------------------------------------------------------------------------------------
def _guide_cursors(g, slots):
    """(cur, run) of the guide records at `slots` (debug_read "guide_tab": 4 + 64 header ints, then 1024 ints {n, -, cur, run, src..} per output slot)"""
    tab = np.zeros(68 + 1024 * 1024, dtype=np.int32)
    nb = C.c_size_t(0)
    st = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    _lib.check(g._lib.ctts_gpt_debug_read(g._h, b"guide_tab", tab.ctypes.data_as(C.c_void_p), tab.nbytes, C.byref(nb), st), "debug_read")
    return [(int(tab[68 + 1024 * s + 2]), int(tab[68 + 1024 * s + 3])) for s in slots]


def _src(u, n):
    rng = np.random.Generator(np.random.Philox(key=300 + u))
    return [int(i) for i in rng.integers(2100, 20000, size=n)]


class TextCall(Raw):
    """An infer_text generate state through the C ABI with max_new_token = TNEW; the log-prob arrays carry one slot more than the call has utterances"""

    def __init__(self, g, n_out):
        super().__init__(g, n_out, text=True)
        dev = g.device
        self.sc = sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, TNEW, TXT_MIN, LW, [], 4, infer_text=True)
        self.ids = torch.full((n_out, TNEW, 4), FILL_I, dtype=torch.int32, device=dev)
        self.tlp = torch.full((2, n_out + 1, TNEW), FILL_F, device=dev)

    def run(self, us, lims, srcs, want, graph):
        """want = (lp_raw?, lp_sampled?) or None: ctts_gpt_set_text_logprob_out is not called at all"""
        e, m = self._sel(us)
        uid = np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64)
        lim = np.ascontiguousarray(lims, dtype=np.int32)
        io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=None, finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(), noise=None, n_draws=0, seed=self.seed,
                        utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
        _lib.check(self.lib.ctts_gpt_begin(self.h, len(us), T_MAX, m.data_ptr(), C.byref(self.sc), C.byref(io), self.st), "begin")
        if srcs is not None:
            self.g._set_text_guide(self.st, TextGuide(FREE5, 2))
            self.g._set_guides(self.st, list(range(len(us))), srcs)
        if want is not None:
            _lib.check(self.lib.ctts_gpt_set_text_logprob_out(self.h, self.tlp[0].data_ptr() if want[0] else None, self.tlp[1].data_ptr() if want[1] else None, self.st),
                       "set_text_logprob_out")
        _lib.check(self.lib.ctts_gpt_prefill(self.h, e.data_ptr(), self.st), "prefill")
        _lib.check(self.lib.ctts_gpt_sample(self.h, self.st), "sample")
        self.decode(TNEW + 1, graph)
        torch.cuda.synchronize()
        assert self.progress()[1] == 1
        cursors = _guide_cursors(self.g, range(len(us))) if srcs is not None else None
        return self.ids.cpu(), self.fin.cpu(), self.end.cpu(), cursors, self.tlp.cpu()


# ---- 2. off, on and NULL bit-identical ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 9])
def test_text_calls_off_on_and_null_are_bit_identical(B, graph):
    g = engine("fp32", INV, max_batch=20)
    us = list(range(B))
    lims = [TNEW if u % 2 == 0 else 6 for u in us]
    for guided in (False, True):
        srcs = [_src(u, 3) if u % 3 != 2 else None for u in us] if guided else None
        off = TextCall(g, B).run(us, lims, srcs, None, graph)
        runs = {w: TextCall(g, B).run(us, lims, srcs, w, graph) for w in ((True, True), (True, False), (False, True))}
        for w, got in runs.items():
            for name, a, b in zip(("ids", "finish", "end_idx"), got[:3], off[:3]):
                assert torch.equal(a, b), f"B={B} graph={graph} guided={guided}: {name} differ with the buffers {w}"
            assert got[3] == off[3], f"B={B} graph={graph} guided={guided}: guide cursors differ with the buffers {w}"
        assert bool((off[4] == FILL_F).all()), "a call that never named the buffers wrote log-probs"
        both = runs[(True, True)][4]
        for k, w in ((0, (True, False)), (1, (False, True))):
            one = runs[w][4]
            assert torch.equal(one[k], both[k]) and bool((one[1 - k] == FILL_F).all()), f"one buffer NULL {w}: the other one differs or the NULL one was written"
        ids, fin, end = off[:3]
        for s in range(B):
            n, eos = int(end[s]), int(fin[s]) == 1
            m = n + 1 if eos else n                    # the step that sampled EOS is written at end_idx; a row that ended by its limit wrote n steps
            assert bool(torch.isfinite(both[0, s, :m]).all()) and bool((both[0, s, :m] <= 0).all()), f"slot {s}: lp_raw of its {m} steps"
            assert bool((both[1, s, :m] <= 0).all()) and not bool((both[:, s, :m] == FILL_F).any()), f"slot {s}: lp_sampled of its {m} steps"
            assert bool((both[:, s, m:] == FILL_F).all()), f"slot {s}: entries past end_idx were written"
            if eos:
                assert int(ids[s, n, 0]) == TEXT_EOS
            if guided and srcs[s] is not None:
                assert eos, "a guided row ends by EOS"
        assert bool((both[:, B] == FILL_F).all()), "something was written beyond [n_out][max_new_token]"


# ---- 3. text rows beside code rows ---------------------------------------------------------------------------------------------------------------------------
class LpMix(Raw):
    """A code-mode generate state (max_new_token NEW) with text rows enabled (max_new_token TNEW) and, on request, their log-prob arrays"""

    def __init__(self, g, n_out, seed=SEED):
        super().__init__(g, n_out, seed=seed)
        dev = g.device
        self.sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, NEW, 2, LW, LP, 4)
        self.tsc = sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, TNEW, TXT_MIN, LW, [], 4, infer_text=True)
        self.ids = torch.full((n_out, NEW, 4), FILL_I, dtype=torch.int32, device=dev)
        self.hid = torch.full((n_out, NEW, 768), FILL_F, device=dev)
        self.lp = torch.full((2, n_out, NEW, 4), FILL_F, device=dev)
        self.tids = torch.full((n_out, TNEW, 4), FILL_I, dtype=torch.int32, device=dev)
        self.tlp = torch.full((2, n_out + 1, TNEW), FILL_F, device=dev)

    def lim(self, u, mode):
        return min(self.lims[u], TNEW if mode else NEW)

    def begin(self, us, modes, text_lp=True, trim=False):
        e, m = self._sel(us)
        T = T_MAX
        if trim:
            T = self.lens[us[0]]
            e, m = e[:, T_MAX - T:].contiguous(), m[:, T_MAX - T:].contiguous()
            self.keep += [e, m]
        uid = np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64)
        lim = np.ascontiguousarray([self.lim(u, md) for u, md in zip(us, modes)], dtype=np.int32)
        md = np.ascontiguousarray(modes, dtype=np.int32)
        io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr(), finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(), noise=None, n_draws=0,
                        seed=self.seed, utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
        _lib.check(self.lib.ctts_gpt_set_row_modes(self.h, md.ctypes.data_as(C.c_void_p), len(us)), "set_row_modes")
        try:
            _lib.check(self.lib.ctts_gpt_begin(self.h, len(us), T, m.data_ptr(), C.byref(self.sc), C.byref(io), self.st), "begin")
        finally:
            self.lib.ctts_gpt_set_row_modes(self.h, None, 0)
        _lib.check(self.lib.ctts_gpt_enable_text_rows(self.h, C.byref(self.tsc), self.tids.data_ptr(), self.st), "enable_text_rows")
        _lib.check(self.lib.ctts_gpt_set_logprob_out(self.h, self.lp[0].data_ptr(), self.lp[1].data_ptr(), self.st), "set_logprob_out")
        if text_lp:
            _lib.check(self.lib.ctts_gpt_set_text_logprob_out(self.h, self.tlp[0].data_ptr(), self.tlp[1].data_ptr(), self.st), "set_text_logprob_out")
        _lib.check(self.lib.ctts_gpt_prefill(self.h, e.data_ptr(), self.st), "prefill")
        _lib.check(self.lib.ctts_gpt_sample(self.h, self.st), "sample")
        return self

    def admit(self, rows, us, outs, modes, atts=None):
        e, m = self._sel(us)
        arrs = [np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(modes, dtype=np.int32), np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64),
                np.ascontiguousarray([self.lim(u, md) for u, md in zip(us, modes)], dtype=np.int32), np.ascontiguousarray(outs, dtype=np.int32),
                np.ascontiguousarray(atts or [0] * len(us), dtype=np.int32)]
        self.keep += arrs
        p = [a.ctypes.data_as(C.c_void_p) for a in arrs]
        _lib.check(self.lib.ctts_gpt_admit_modes(self.h, len(us), p[0], p[1], self.st), "admit_modes")
        _lib.check(self.lib.ctts_gpt_admit(self.h, len(us), p[0], T_MAX, m.data_ptr(), e.data_ptr(), p[2], p[3], p[4], p[5], self.st), "admit")

    def text_out(self, o):
        """(ids [n], lp_raw [m], lp_sampled [m], n, finish): m = n + 1 where the row ended by EOS"""
        torch.cuda.synchronize()
        n, fin = int(self.end[o]), int(self.fin[o])
        m = n + 1 if fin == 1 else n
        return self.tids[o, :n, 0].cpu().to(torch.long), self.tlp[0, o, :m].cpu(), self.tlp[1, o, :m].cpu(), n, fin


_alone = {}


def alone_text(g, u, key, lim, seed=SEED):
    """utterance u through a batch-1 generate(infer_text=True, return_text_logprobs=True) on its trimmed prompt: (ids [n], lp_raw [m], lp_sampled [m])"""
    k = (key, u, lim, seed)
    if k not in _alone:
        lens, _, ids, mask, uids = _pool()
        T = lens[u]
        i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:])
        out = list(g.generate(g(i1, torch.ones(1, T, dtype=torch.bool)), i1, torch.tensor([TXT_T]), TEXT_EOS, attention_mask=torch.from_numpy(mask[u:u + 1, T_MAX - T:]),
                              max_new_token=TNEW, min_new_token=TXT_MIN, logits_warpers=LW, infer_text=True, noise="device", seed=seed, utt_ids=[uids[u]],
                              max_new_tokens_per_row=[lim], return_text_logprobs=True))[-1]
        n = out.ids[0].shape[0]
        assert out.logprobs[0].shape == (n,) and out.sampled_logprobs[0].shape == (n,)
        fl = out.final_logprobs[0]
        assert fl is None or fl.shape == (2,)
        raw, smp = out.logprobs[0].cpu(), out.sampled_logprobs[0].cpu()
        if fl is not None:
            raw, smp = torch.cat([raw, fl[0:1].cpu()]), torch.cat([smp, fl[1:2].cpu()])
        _alone[k] = (out.ids[0].cpu(), raw, smp)
    return _alone[k]


def _assert_text_matches_alone(got, one, exact, what):
    ids, raw, smp, n, _ = got
    assert torch.equal(ids, one[0]), f"{what}: ids differ from the batch-1 infer_text call"
    assert raw.shape == one[1].shape and smp.shape == one[2].shape, f"{what}: {raw.shape[0]} log-probs, batch 1 wrote {one[1].shape[0]}"
    if exact:
        assert torch.equal(raw, one[1]) and torch.equal(smp, one[2]), f"{what}: log-probs differ from the batch-1 call"
    else:
        fin = torch.isfinite(one[2])
        d = max(float((raw - one[1]).abs().max()), float((smp[fin] - one[2][fin]).abs().max()) if bool(fin.any()) else 0.0)
        print(f"{what}: |log-probs - batch 1| {d:.3e} (bound 2e-5)")
        assert d <= 2e-5 and torch.equal(torch.isfinite(smp), fin)


@pytest.mark.parametrize("mode", ["invariant", "default"])
@pytest.mark.parametrize("B", [3, 9])
def test_text_rows_beside_code_rows(B, mode):
    """2 text rows beside code rows at 3 rows (the persistent launch) and 9 rows (the launch chain): each text row's log-probs against its own batch-1 infer_text
    call -- bit for bit under batch_invariant, within 2e-5 (the batch-against-batch-1 bound of tests/test_gpu_gen_logprobs.py) in default mode, where the prompt
    keeps the pool's left padding.  The code rows' ids and log-probs are those of the same call without text log-probs."""
    g = engine("fp32", INV if mode == "invariant" else None, max_batch=20)
    us = list(range(B))
    modes = [0, 1, 1] if B == 3 else [0, 1, 0, 0, 1, 0, 0, 0, 0]
    c = LpMix(g, B).begin(us, modes)
    c.decode(NEW + 2)
    assert c.progress()[1] == 1
    plain = LpMix(g, B).begin(us, modes, text_lp=False)
    plain.decode(NEW + 2)
    assert plain.progress()[1] == 1
    assert bool((plain.tlp == FILL_F).all())
    for u, md in zip(us, modes):
        if md == 0:
            a, b = c.out(u), plain.out(u)
            assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:], f"code utterance {u} changes with the text rows' log-probs"
            assert bool((c.tlp[:, u] == FILL_F).all()), f"code slot {u}: text log-probs were written"
        else:
            assert torch.equal(c.tids[u], plain.tids[u])
            _assert_text_matches_alone(c.text_out(u), alone_text(g, u, mode, c.lim(u, 1)), mode == "invariant", f"{B} rows ({mode}), text utterance {u}")
            m = c.text_out(u)[1].shape[0]
            assert bool((c.tlp[:, u, m:] == FILL_F).all())
    assert bool((c.tlp[:, B] == FILL_F).all())


# ---- 4. session life cycle -------------------------------------------------------------------------------------------------------------------------------------
def test_log_probs_follow_their_utterance_through_compaction_cancel_and_readmission():
    """batch_invariant, sentinel fills.  (a) rows 0 (code), 1 (text), 2 (code) begin; the code rows end, the batch is compacted to the text row, grown again and text
    utterance 5 is admitted into the lane the compaction freed: both text utterances equal their batch-1 calls, log-probs included, each in its own slot.
    (b) a text row cancelled after 3 steps holds a prefix of its uncancelled log-probs and the fill behind it.  (c) an utterance re-admitted into its slot with
    attempt + 1 overwrites from step 0: its slot equals that of a state which seated it with attempt 1 from the start, and holds the fill behind its new end."""
    g = engine("fp32", INV, max_batch=20)
    # (a)
    c = LpMix(g, 6)
    c.lims = [3 if u in (0, 2) else x for u, x in enumerate(c.lims)]          # the code rows end after 3 tokens
    c.begin([0, 1, 2], [0, 1, 0])
    c.decode(4)
    c.compact([1])
    assert c.grow(1) == 0, c.lib.ctts_last_error().decode()
    c.admit([1], [5], [5], [1])
    c.decode(TNEW + 2)
    assert c.progress()[1] == 1
    for u in (1, 5):
        _assert_text_matches_alone(c.text_out(u), alone_text(g, u, "invariant", c.lim(u, 1)), True, f"(a) text utterance {u}")
        m = c.text_out(u)[1].shape[0]
        assert bool((c.tlp[:, u, m:] == FILL_F).all())
    for s in (0, 2, 3, 4, 6):
        assert bool((c.tlp[:, s] == FILL_F).all()), f"(a) slot {s} holds no text utterance, yet log-probs were written"
    full = c.text_out(1)
    # (b)
    c = LpMix(g, 3).begin([0, 1], [0, 1])
    c.decode(2)                                        # 3 steps sampled
    assert c.cancel([1]) == 0
    c.decode(NEW + 2)
    ids, raw, smp, n, fin = c.text_out(1)
    if full[3] > 3:
        assert n == 3 and fin == 0 and torch.equal(ids, full[0][:3]) and torch.equal(raw, full[1][:3]) and torch.equal(smp, full[2][:3]), "(b) the cancelled row is not a prefix"
    assert bool((c.tlp[:, 1, n + (1 if fin == 1 else 0):] == FILL_F).all()), "(b) a cancelled row kept writing log-probs"
    # (c)
    fresh = LpMix(g, 3).begin([0], [0])
    assert fresh.grow(1) == 0
    fresh.admit([1], [4], [1], [1], atts=[1])
    fresh.decode(NEW + 2)
    want = fresh.text_out(1)
    c = LpMix(g, 3).begin([0, 4], [0, 1])
    c.decode(TNEW + 1)
    first = c.text_out(1)
    assert first[3] >= 1
    c.admit([1], [4], [1], [1], atts=[1])
    c.decode(TNEW + 2)
    again = c.text_out(1)
    for name, a, b in zip(("ids", "lp_raw", "lp_sampled"), again[:3], want[:3]):
        assert torch.equal(a, b), f"(c) re-admitted with attempt 1: {name} differ from a state that seated it with attempt 1 from the start"
    m, m0 = again[1].shape[0], first[1].shape[0]
    if m0 > m:                                       # behind the new end the first attempt's values stand: the call clears nothing
        assert torch.equal(c.tlp[0, 1, m:m0].cpu(), first[1][m:m0])
    assert bool((c.tlp[:, 1, max(m, m0):] == FILL_F).all())


# ---- 7. errors by name -----------------------------------------------------------------------------------------------------------------------------------------
def test_errors_by_name():
    g = engine("fp32", INV, max_batch=20)
    lib, h = g._lib, g._h
    err = lambda: lib.ctts_last_error().decode()
    # a code call without text rows
    c = Raw(g, 2).begin([0, 1])
    buf = torch.zeros(2, 2, TNEW, device=g.device)
    assert lib.ctts_gpt_set_text_logprob_out(h, buf[0].data_ptr(), buf[1].data_ptr(), c.st) != 0 and "a code call without text rows" in err()
    c.decode(30)
    # after the first sample: an infer_text call, and a code call with text rows
    t = Raw(g, 2, text=True).begin([0, 1])
    assert lib.ctts_gpt_set_text_logprob_out(h, buf[0].data_ptr(), buf[1].data_ptr(), t.st) != 0 and "after the first" in err()
    # ... and the existing refusal is still in place: set_logprob_out after a text begin
    assert lib.ctts_gpt_set_logprob_out(h, buf[0].data_ptr(), buf[1].data_ptr(), t.st) != 0 and "infer_text" in err()
    t.decode(30)
    m = LpMix(g, 2).begin([0, 1], [0, 1], text_lp=False)
    assert lib.ctts_gpt_set_text_logprob_out(h, m.tlp[0].data_ptr(), m.tlp[1].data_ptr(), m.st) != 0 and "after the first" in err()
    m.decode(NEW + 2)
    # no generate state: scoring ended it
    from tests.test_gpu_score import case, run
    run(g, case([6], [3], 6, 5))
    assert lib.ctts_gpt_set_text_logprob_out(h, buf[0].data_ptr(), buf[1].data_ptr(), c.st) != 0 and "no generate state" in err()
    # hip_models: return_logprobs with infer_text keeps raising; return_text_logprobs in a code call without text rows is refused by name
    lens, _, ids, mask, _ = _pool()
    i1 = torch.from_numpy(ids[:1, T_MAX - lens[0]:])
    e1 = g(i1, torch.ones(1, lens[0], dtype=torch.bool))
    with pytest.raises(_lib.HipBackendError, match="infer_text"):
        list(g.generate(e1, i1, torch.tensor([TXT_T]), TEXT_EOS, max_new_token=4, logits_warpers=LW, infer_text=True, noise="device", seed=1, return_logprobs=True))
    with pytest.raises(_lib.HipBackendError, match="a code call without text rows"):
        list(g.generate(e1, i1, torch.tensor([0.3] * 4), EOS, max_new_token=4, logits_warpers=LW, noise="device", seed=1, return_text_logprobs=True))
    with pytest.raises(_lib.HipBackendError, match="a code call without text rows"):
        g.open_session(torch.tensor([0.3] * 4), EOS, NEW, logits_warpers=LW, return_text_logprobs=True)
    assert not g.busy


# ---- hip_models: a session's text utterances carry their log-probs ------------------------------------------------------------------------------------------
def test_open_session_text_results_carry_log_probs():
    """open_session(text_rows=..., return_text_logprobs=True): a text utterance's SessionResult carries [n] / [n] / [2] equal to its batch-1 call's (batch_invariant);
    a code utterance's result is what it is without the option (return_logprobs stays code-only: None here)."""
    g = engine("fp32", INV, max_batch=20)
    lens, lims, ids, mask, uids = _pool()
    text_rows = dict(temperature=TXT_T, top_P=0.7, top_K=20, eos_token=TEXT_EOS, max_new_token=TNEW, min_new_token=TXT_MIN)
    got = {}
    with g.open_session(torch.tensor([0.3] * 4), EOS, NEW, min_new_token=2, logits_warpers=LW, logits_processors=LP, seed=SEED, rows=4, text_rows=text_rows,
                        return_text_logprobs=True) as ses:
        tks = {}
        for u, md in ((0, "code"), (1, "text"), (4, "text")):
            T = lens[u]
            i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:])
            emb = g(i1, torch.ones(1, T, dtype=torch.bool))
            tks[ses.submit(emb[0], torch.ones(T, dtype=torch.int32), uids[u], limit=min(lims[u], TNEW if md == "text" else NEW), mode=md)] = (u, md)
        for r in ses.drain():
            got[tks[r.ticket][0]] = r
    assert got[0].mode == "code" and got[0].logprobs is None and got[0].final_logprobs is None
    for u in (1, 4):
        r, one = got[u], alone_text(g, u, "invariant", min(lims[u], TNEW))
        n = r.ids.shape[0]
        assert r.mode == "text" and r.logprobs.shape == (n,) and r.sampled_logprobs.shape == (n,)
        raw, smp = r.logprobs.cpu(), r.sampled_logprobs.cpu()
        if r.finished_by_eos:
            assert r.final_logprobs.shape == (2,)
            raw, smp = torch.cat([raw, r.final_logprobs[0:1].cpu()]), torch.cat([smp, r.final_logprobs[1:2].cpu()])
        assert torch.equal(r.ids.cpu(), one[0]) and torch.equal(raw, one[1]) and torch.equal(smp, one[2]), f"session text utterance {u}"
    assert not g.busy


# ---- the pipeline with the toy tokenizer: ranked refine candidates, score_text, details -----------------------------------------------------------------------
def test_pipeline_refine_candidates_and_score_text(tmp_path):
    """infer(refine_candidates=3): the refine pass serves every text three times under candidate_utt_id(u, k), the winner is the candidate with the highest mean
    raw log-prob ([Ebreak] step included) and pipe.score_text gives the winner's ids the log-probs the sampler wrote (2e-4, the decode-against-prompt-pass
    bound); with refine_guided every candidate holds the source tokens; infer(return_details=True) carries the plain refinement's log-probs."""
    from chatttsplus_amd import synth
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import (ChatTTSPlusPipeline, InferCodeParams, RefineTextParams, RefinedTexts, _decode_refined, candidate_utt_id, default_text_guide,
                                          refine_sources, select_candidate)
    from tests.test_gpu_score import CFG4, LLAMA4
    g = GPT(LLAMA4, max_batch=8, max_seq_len=200, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(synth.gpt_state_dict(CFG4, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    tok = synth.toy_tokenizer(str(tmp_path / "tok"))
    texts = synth.toy_texts(3, 5, 7, seed=68)
    refine = RefineTextParams(prompt="[oral_2]", max_new_token=12, min_new_token=2, show_tqdm=False)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=8, min_new_token=2, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
    seed, N = 4243, 3
    try:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, tok, torch.device("cuda:0"))
        norm = [pipe.normalizer(t, True, True, None) for t in texts]
        r = pipe._refine_text(norm, refine, continuous_rows=4, seed=seed, utt_ids=[0, 1, 2], n_cand=N)
        assert isinstance(r, RefinedTexts) and len(r.ids) == 3
        plain = pipe._refine_text(norm, refine, continuous_rows=4, seed=seed, utt_ids=[0, 1, 2])
        for u in range(3):
            sc = r.candidate_scores[u].tolist()
            assert r.candidate[u] == select_candidate(sc) and r.mean_logprob[u] == pytest.approx(max(sc))
            if r.candidate[u] == 0:                  # candidate 0 is the plain refinement
                assert torch.equal(r.ids[u].cpu(), plain.ids[u].cpu())
            one = pipe._refine_text([norm[u]], refine, continuous_rows=1, seed=seed, utt_ids=[candidate_utt_id(u, r.candidate[u])], want_logprobs=True)
            assert torch.equal(one.ids[0].cpu(), r.ids[u].cpu()) and torch.equal(one.logprobs[0], r.logprobs[u]), f"text {u}: the winner is not candidate {r.candidate[u]}'s own call"
        res = pipe.score_text(norm, [i.cpu() for i in r.ids], params_refine_text=refine)
        for u in range(3):
            m = r.logprobs[u].shape[0]               # (a refinement that ended by its limit has no [Ebreak] step: score_text's last entry is then extra)
            d = float((res.logprob[u][:m] - r.logprobs[u]).abs().max())
            print(f"text {u}: candidate {r.candidate[u]} of {r.candidate_scores[u].tolist()}, |score_text - sampler| {d:.3e}")
            assert d <= 2e-4
        kw = dict(params_refine_text=refine, params_infer_code=params, noise="device", noise_seed=seed, slice_size=4, utt_ids=[0, 1, 2])
        got = list(pipe.infer(list(texts), refine_text_only=True, refine_candidates=N, **kw))
        assert got == [_decode_refined(tok, r.ids)]
        # guided: every candidate holds the source tokens, the ranking chooses among the insertions
        free = set(default_text_guide(tok).free_ids)
        guided = list(pipe.infer(list(texts), refine_text_only=True, refine_candidates=N, refine_guided=True, **kw))[0]
        ids, att, _ = pipe._refine_prompt(norm, refine)
        for u, src in enumerate(refine_sources(tok, ids, att)):
            out_ids = tok._tokenizer(guided[u], add_special_tokens=False)["input_ids"]
            assert [i for i in out_ids if i not in free] == src, f"text {u}: the guided winner dropped or changed a source token"
        # return_details: the refine pass's log-probs beside the code pass's
        d = list(pipe.infer(list(texts), return_details=True, **kw))[0]
        assert len(d.refined_logprobs) == 3 and all(lp.dim() == 1 and lp.numel() >= 1 for lp in d.refined_logprobs)
        assert d.refined_mean_logprob == pytest.approx([float(lp.double().mean()) for lp in d.refined_logprobs])
        d = list(pipe.infer(list(texts), return_details=True, skip_refine_text=True, **kw))[0]
        assert d.refined_logprobs is None and d.refined_mean_logprob is None
        with pytest.raises(_lib.HipBackendError, match="refine_candidates > 1 needs stream=False"):
            list(pipe.infer(list(texts), stream=True, refine_candidates=2, **kw))
        assert not g.busy
    finally:
        g.close()
