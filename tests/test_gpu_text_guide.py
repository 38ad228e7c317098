"""Guided refine-text on the GPU (ctts_gpt_set_text_guide / ctts_gpt_set_guides / ctts_sampler_run_text_guided; sampler_text_kernel<true>): a guided text row's
ids are provably its source ids in order, with only ids of the free set inserted, ended by EOS.  Synthetic weights at real widths, 4 decoder layers, the prompt
pool of tests/test_gpu_session.py (set-up as in tests/test_gpu_text_rows.py).

1. the stand-alone hook (one step of the generate kernel itself) against a CPU restatement on identical logits and noise: ids and cursors equal, element for element;
2. text-mode calls at B = 1, 2, 3, guided and unguided rows mixed: the structural guarantees, batch-invariant equality with the batch-1 calls, graphs on / off;
3. token-for-token parity of a guided call with the CPU restatement over oracle.ref_cpu's forward;
4. guided text rows beside code rows at 2, 9 and 17 rows: begin / admit / grow + admit, a slot re-used guided -> unguided and back, a cancelled guided row,
   sentinel fills, code rows bit-identical to the schedule without guides;
5. the pipeline with the toy tokenizer: infer(refine_guided=True, continuous=True) and a refining SynthSession."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import (TextGuide, gen_logits, guide_allowed, guide_eos_removable, guide_standin, guide_step, sampler_cfg_from_objects)
from oracle import device_noise, ref_cpu
from tests.test_gpu_score import engine, oracle
from tests.test_gpu_session import FILL_I, INV, LW, SEED, T_MAX, TEXT_EOS, Raw, _alone, _assert_equals_alone, _pool
from tests.test_gpu_text_rows import SCHEDULES, TXT_MIN, TXT_NEW, TXT_T, Mix, _alone_text

pytestmark = pytest.mark.gpu

V = 21178
STRADDLE = [0, 1023, 1024, 2047, TEXT_EOS - 1]        # ownership in the kernel: thread j & 1023, bit j >> 10; the largest id that is not EOS
FREE5 = [7, 1023, 1024, 5000, TEXT_EOS - 1]


def _free64():
    rng = np.random.Generator(np.random.Philox(key=77))
    rest = [int(i) for i in rng.permutation(np.arange(3000, 20000))[:64 - len(STRADDLE)]]
    return STRADDLE + rest


# ---- the CPU restatement of one guided step: the unguided arithmetic (oracle.ref_cpu's warpers, softmax, exponential race) over the allowed set ------------------
def cpu_guided_step(logits, q, T, top_p, top_k, min_keep, min_new, eos, src, cur, run, t, limit, free, max_run):
    """-> (idx, cur, run, finished).  Elements outside A are -inf BEFORE the division by the temperature; min_new_token removes EOS only while another element of
    A remains; a NaN ratio counts as 0 and when every ratio is 0 the stand-in (src[cur], EOS once the source is out) is returned."""
    n = len(src)
    A = guide_allowed(cur, run, t, limit, n, max_run, src, free, eos)
    x = torch.full((1, logits.numel()), -float("inf"))
    x[0, A] = logits[A]
    x = x / torch.tensor(float(T), dtype=torch.float32)
    if top_p is not None:
        x = ref_cpu.top_p_warp(x, top_p, min_keep)
    if top_k is not None:
        x = ref_cpu.top_k_warp(x, top_k, 1)             # (top_k as the sampler receives it: already max(top_K, min_tokens_to_keep))
    if t < min_new and guide_eos_removable(cur, run, t, limit, n, max_run, free):
        x = x.clone()
        x[0, eos] = -float("inf")
    ratio = torch.softmax(x, dim=-1)[0] / q
    ratio = torch.where(ratio > 0, ratio, torch.zeros_like(ratio))
    idx = int(torch.argmax(ratio)) if float(ratio.max()) > 0 else guide_standin(cur, n, src, eos)
    return (idx,) + guide_step(cur, run, t, limit, n, max_run, idx, src=src, eos=eos)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_hook(g, sc, logits, q, free, max_run, rows):
    """rows: [dict(src, cur, run, step, limit)] -> (idx, cur, run) lists"""
    R = len(rows)
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    cat = arr([i for r in rows for i in r["src"]])
    off = arr(np.cumsum([0] + [len(r["src"]) for r in rows]))
    cur, run, step, lim = (arr([r[k] for r in rows]) for k in ("cur", "run", "step", "limit"))
    fr = arr(free if free else [0])
    idx, co, ro = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    lg, qq = logits.to(g.device).contiguous(), q.to(g.device).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    rc = g._lib.ctts_sampler_run_text_guided(C.byref(sc), lg.data_ptr(), qq.data_ptr(), R, V, _ptr(fr), len(free), max_run, _ptr(cat), _ptr(off), _ptr(cur), _ptr(run),
                                             _ptr(step), _ptr(lim), _ptr(idx), _ptr(co), _ptr(ro), st)
    return rc, idx.tolist(), co.tolist(), ro.tolist()


MIN_NEW_HOOK, MAX_RUN_HOOK = 5, 2


def _hook_rows(free, rng):
    """the scenarios of one free set: (name, row); sources over plain ids and, where there is one, a free id at the cursor"""
    plain = [int(i) for i in rng.integers(2100, 20000, size=8)]
    inside = plain[:2] + [free[len(free) // 2]] + plain[3:] if free else None
    out = []
    for name, src in (("outside", plain), ("inside", inside)):
        if src is None:
            continue
        n = len(src)
        out += [(f"{name}: slack many, min_new active", dict(src=src, cur=2, run=0, step=2, limit=40)),
                (f"{name}: slack many", dict(src=src, cur=2, run=1, step=9, limit=40)),
                (f"{name}: slack 1", dict(src=src, cur=2, run=0, step=9, limit=9 + (n - 2) + 1 + 1)),
                (f"{name}: slack 0", dict(src=src, cur=2, run=0, step=9, limit=9 + (n - 2) + 1)),
                (f"{name}: run == max_run", dict(src=src, cur=2, run=MAX_RUN_HOOK, step=9, limit=40)),
                (f"{name}: first step", dict(src=src, cur=0, run=0, step=0, limit=n + 1))]
    short = plain[:3]
    out += [("cur == n, steps left", dict(src=short, cur=3, run=0, step=9, limit=40)),
            ("cur == n, last step", dict(src=short, cur=3, run=1, step=9, limit=10)),
            ("cur == n, min_new active, another element left", dict(src=short, cur=3, run=0, step=3, limit=40)),
            ("cur == n, min_new active, EOS alone (last step)", dict(src=short, cur=3, run=0, step=3, limit=4)),
            ("cur == n, min_new active, EOS alone (run == max_run)", dict(src=short, cur=3, run=MAX_RUN_HOOK, step=3, limit=40))]
    return out


# ---- 1. the stand-alone hook against the CPU restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [1, 20])
@pytest.mark.parametrize("top_p", [0.7, None])
def test_hook_equals_cpu_restatement(top_p, top_k):
    g = engine("fp32", INV, max_batch=20)
    w, _ = gen_logits(0, top_P=top_p, top_K=top_k, repetition_penalty=None)
    sc = sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, 64, MIN_NEW_HOOK, w, [], 4, infer_text=True)
    rng = np.random.Generator(np.random.Philox(key=4242))
    for free in ([], [1023], STRADDLE, _free64()):
        cases = []
        for rep in range(2):
            cases += _hook_rows(free, rng)
        # degenerate rows: every logit -inf / NaN -> every ratio NaN -> the stand-in (src[cur], EOS once the source is out), never id 0
        deg = [("all -inf", dict(src=[4000, 4001], cur=1, run=0, step=9, limit=40)), ("all NaN", dict(src=[4000, 4001], cur=2, run=0, step=9, limit=40))]
        cases += deg
        R = len(cases)
        tg = torch.Generator().manual_seed(1000 + len(free))
        logits = torch.randn(R, V, generator=tg) * 3.0
        logits[R - 2] = -float("inf")
        logits[R - 1] = float("nan")
        q = torch.empty(R, V).exponential_(generator=tg)
        rc, idx, cur, run = run_hook(g, sc, logits, q, free, MAX_RUN_HOOK, [c for _, c in cases])
        assert rc == 0, g._lib.ctts_last_error().decode()
        drew_free = 0
        for r, (name, c) in enumerate(cases):
            want = cpu_guided_step(logits[r], q[r], TXT_T, top_p, sc.top_k, 3 if top_p is not None else 1, MIN_NEW_HOOK, TEXT_EOS, c["src"], c["cur"], c["run"], c["step"],
                                   c["limit"], free, MAX_RUN_HOOK)
            print(f"free {len(free):2d} {name}: device idx {idx[r]} cur {cur[r]} run {run[r]}; cpu {want}")
            assert (idx[r], cur[r], run[r]) == want[:3], f"free set of {len(free)}, {name}"
            drew_free += idx[r] in free and idx[r] != c["src"][min(c["cur"], len(c["src"]) - 1)]
        assert idx[R - 2] == 4001 and idx[R - 1] == TEXT_EOS
        if len(free) >= 5 and top_k > 3:
            assert drew_free > 0, "no case drew a free id: the free path went untested"


def test_hook_refusals():
    g = engine("fp32", INV, max_batch=20)
    sc = sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, 64, 0, LW, [], 4, infer_text=True)
    lg, q = torch.zeros(1, V), torch.ones(1, V)
    ok = dict(src=[5, 6], cur=0, run=0, step=0, limit=8)
    for free, max_run, row, msg in (([TEXT_EOS], 2, ok, "is the EOS token"), ([V], 2, ok, "outside 0.."), (list(range(65)), 2, ok, "at most 64"), ([3, 3], 2, ok, "listed twice"),
                                    ([3], -1, ok, "max_run"), ([3], 2, dict(ok, src=[]), "n == 0"), ([3], 2, dict(ok, limit=2), "needs 3 tokens"),
                                    ([3], 2, dict(ok, src=[5, TEXT_EOS]), "source id"), ([3], 2, dict(ok, cur=3), "outside the guide")):
        rc, *_ = run_hook(g, sc, lg, q, free, max_run, [row])
        assert rc != 0 and msg in g._lib.ctts_last_error().decode(), (msg, g._lib.ctts_last_error().decode())


# ---- 2. text-mode calls ---------------------------------------------------------------------------------------------------------------------------------
def _src(u, n):
    """a source of n ids for utterance u: plain ids, with one free id of FREE5 inside when it is long enough (the precedence case)"""
    rng = np.random.Generator(np.random.Philox(key=300 + u))
    s = [int(i) for i in rng.integers(2100, 20000, size=n)]
    if n >= 4:
        s[2] = FREE5[1]
    return s


def _check_structure(ids, src, free, max_run, limit, what):
    """ids (EOS excluded) are src with free ids interleaved, no run longer than max_run, within the limit"""
    k, run = 0, 0
    for i in ids:
        if k < len(src) and i == src[k]:
            k, run = k + 1, 0
        else:
            assert i in free, f"{what}: id {i} is neither the next source id nor a free id ({ids} for {src})"
            run += 1
            assert run <= max_run, f"{what}: a run of {run} free ids"
    assert k == len(src), f"{what}: {k} of {len(src)} source ids ({ids} for {src})"
    assert len(ids) + 1 <= limit


def _gen_text(g, us, lims, tg, srcs, seed=SEED, graph=True):
    lens, _, ids, mask, uids = _pool()
    Tm = max(lens[u] for u in us)
    i1 = torch.from_numpy(ids[us][:, T_MAX - Tm:])
    m1 = torch.from_numpy(mask[us][:, T_MAX - Tm:])
    was = g.use_graph
    g.use_graph = graph
    try:
        out = list(g.generate(g(i1, torch.ones(len(us), Tm, dtype=torch.bool)), i1, torch.tensor([TXT_T]), TEXT_EOS, attention_mask=m1, max_new_token=TXT_NEW,
                              min_new_token=TXT_MIN, logits_warpers=LW, infer_text=True, noise="device", seed=seed, utt_ids=[uids[u] for u in us],
                              max_new_tokens_per_row=lims, text_guide=tg, guide_src=srcs))[-1]
    finally:
        g.use_graph = was
    return [i.cpu().tolist() for i in out.ids]


@pytest.mark.parametrize("max_run", [0, 1, 3])
def test_text_mode_calls_keep_every_source_token(max_run):
    g = engine("fp32", INV, max_batch=20)
    tg = TextGuide(FREE5, max_run)
    # (utterances, limits, source lengths; None = unguided): B = 1, 2, 3; lengths 1, 2, 7 and limit - 1 (zero slack)
    for us, lims, ns in (([4], [12], [7]), ([1, 2], [TXT_NEW, 9], [1, 8]), ([3, 5, 6], [14, TXT_NEW, TXT_NEW], [2, None, TXT_NEW - 1])):
        srcs = [None if n is None else _src(u, n) for u, n in zip(us, ns)]
        got = _gen_text(g, us, lims, tg, srcs)
        eager = _gen_text(g, us, lims, tg, srcs, graph=False)
        assert got == eager, "use_graph 0 / 1 give different ids"
        for b, (u, lim, s) in enumerate(zip(us, lims, srcs)):
            what = f"B={len(us)} utterance {u} max_run={max_run}"
            print(what, "src", s, "->", got[b])
            one = _gen_text(g, [u], [lim], tg, [s])[0]
            assert got[b] == one, f"{what}: differs from its batch-1 call"
            if s is None:
                assert got[b] == _alone_text(g, u, "inv", lim=lim).tolist(), f"{what}: the unguided row differs from its batch-1 unguided call"
                continue
            _check_structure(got[b], s, FREE5, max_run, lim, what)
            if max_run == 0 or len(s) + 1 == lim:
                assert got[b] == s, f"{what}: with no free run / zero slack the output is exactly the source"


def test_text_mode_finish_flags_and_free_tokens_appear():
    """through the C ABI: finish == 1 and end_idx within the limit for every guided row; over the rows some free id is drawn (the free path is live)"""
    g = engine("fp32", INV, max_batch=20)
    c = Raw(g, 4, text=True)
    us, ns = [0, 1, 2, 3], [3, 5, 1, 4]
    srcs = [_src(u, n) for u, n in zip(us, ns)]
    e, m = c._sel(us)
    uid = np.ascontiguousarray([c.uids[u] for u in us], dtype=np.uint64)
    lim = np.ascontiguousarray([16, 16, 16, 5], dtype=np.int32)
    io = _lib.GenIO(ids=c.ids.data_ptr(), hiddens=None, finish=c.fin.data_ptr(), end_idx=c.end.data_ptr(), noise=None, n_draws=0, seed=c.seed, utt_ids=uid.ctypes.data,
                    row_limits=lim.ctypes.data)
    _lib.check(c.lib.ctts_gpt_begin(c.h, 4, T_MAX, m.data_ptr(), C.byref(c.sc), C.byref(io), c.st), "begin")
    # refused by name before any launch: guides without the per-call part
    sl = np.ascontiguousarray([0], dtype=np.int32); cat = np.ascontiguousarray(srcs[0], dtype=np.int32); off = np.ascontiguousarray([0, 3], dtype=np.int32)
    assert c.lib.ctts_gpt_set_guides(c.h, 1, _ptr(sl), _ptr(cat), _ptr(off), c.st) != 0 and "without the per-call part" in c.lib.ctts_last_error().decode()
    g._set_text_guide(c.st, TextGuide(FREE5, 3))
    off2 = np.ascontiguousarray([0, 16], dtype=np.int32); cat2 = np.ascontiguousarray(list(range(100, 116)), dtype=np.int32)
    assert c.lib.ctts_gpt_set_guides(c.h, 1, _ptr(sl), _ptr(cat2), _ptr(off2), c.st) != 0 and "needs 17 tokens" in c.lib.ctts_last_error().decode()
    sl4 = np.ascontiguousarray([1024], dtype=np.int32)
    assert c.lib.ctts_gpt_set_guides(c.h, 1, _ptr(sl4), _ptr(cat), _ptr(off), c.st) != 0 and "output slot 1024" in c.lib.ctts_last_error().decode()
    g._set_guides(c.st, us, srcs)
    _lib.check(c.lib.ctts_gpt_prefill(c.h, e.data_ptr(), c.st), "prefill")
    _lib.check(c.lib.ctts_gpt_sample(c.h, c.st), "sample")
    c.decode(16)
    torch.cuda.synchronize()
    steps, alld = c.progress()
    assert alld == 1
    n_free = 0
    for o, s in enumerate(srcs):
        n = int(c.end[o])
        ids = c.ids[o, :n, 0].cpu().tolist()
        assert int(c.fin[o]) == 1 and n + 1 <= int(lim[o]), f"slot {o}: finish {int(c.fin[o])}, end_idx {n}, limit {int(lim[o])}"
        assert int(c.ids[o, n, 0]) == TEXT_EOS and bool((c.ids[o, n + 1:] == FILL_I).all())
        _check_structure(ids, s, FREE5, 3, int(lim[o]), f"slot {o}")
        n_free += len(ids) - len(s)
    assert srcs[3] == c.ids[3, :4, 0].cpu().tolist()            # zero slack: exactly the source
    assert n_free > 0, "no free id was drawn in four guided rows with max_run 3"
    # every begin switches the feature off: the next plain call is the unguided one
    assert _alone_text(g, 2, "inv-after-guide").tolist() == _alone_text(g, 2, "inv").tolist()


# ---- 3. token-for-token parity with the CPU restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [9191, 4711])
def test_guided_call_equals_cpu_restatement(seed):
    """default mode, fp32, batch 1: the oracle's forward, its warpers, the documented device noise (stream 4) and the pure-Python automaton give the device's ids"""
    g, o = engine("fp32"), oracle()
    u, n, lim, max_run = 2, 5, 12, 2
    tg, src = TextGuide(FREE5, max_run), _src(2, 5)
    got = _gen_text(g, [u], [lim], tg, [src], seed=seed)[0]
    lens, _, ids, mask, uids = _pool()
    T = lens[u]
    i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:]).long()
    emb = o.embed(i1, torch.ones(1, T, dtype=torch.bool))
    o.alloc_cache(1, T + lim)
    m = torch.ones(1, T + lim, dtype=torch.bool)
    cur = run = 0
    want, x, nxt = [], emb, None
    for t in range(lim):
        mm = m[:, :T + t]
        pos = mm.long().cumsum(-1) - 1
        x, p = (emb, pos) if t == 0 else (torch.nn.functional.embedding(torch.tensor([[nxt]]), o.sd["emb_text.weight"]), pos[:, -1:])
        logits = torch.nn.functional.linear(o.forward(x, mm, p)[:, -1], o.head_text)[0]
        q = torch.from_numpy(np.asarray(device_noise.exp_noise(seed, uids[u], 4, t, 0, V), dtype=np.float32))
        nxt, cur, run, fin = cpu_guided_step(logits, q, TXT_T, 0.7, 20, 3, TXT_MIN, TEXT_EOS, src, cur, run, t, lim, FREE5, max_run)
        if fin:
            break
        want.append(nxt)
    print("seed", seed, "device", got, "cpu", want)
    assert got == want


# ---- 4. guided text rows beside code rows ----------------------------------------------------------------------------------------------------------------
def _run_schedule(g, key, guided, cancel_at=None):
    """SCHEDULES[key] of tests/test_gpu_text_rows.py with a guide on its text rows (`guided`: utterance -> source, others unguided), then one more admission that
    re-uses output slots: a guided slot for an unguided utterance and the other way round"""
    c = Mix(g, 18)
    tg = TextGuide(FREE5, 2)
    mode_u, lims = {}, {}

    def guides(us, outs):
        if guided is not None:
            g._set_guides(c.st, outs, [guided.get(u) for u in us])

    for call in SCHEDULES[key]:
        if call[0] == "begin":
            _, us, modes, lm = call
            ll = [(x or c.lims[u]) if md == 0 else min(x or c.lims[u], TXT_NEW) for u, md, x in zip(us, modes, lm)]
            if guided is None:
                c.begin(us, modes, ll)
            else:                                   # Mix.begin with the guide between enable_text_rows and the first sample
                real = c.lib.ctts_gpt_prefill
                e, m = c._sel(us)
                uid = np.ascontiguousarray([c.uids[u] for u in us], dtype=np.uint64); lim = np.ascontiguousarray(ll, dtype=np.int32); md = np.ascontiguousarray(modes, dtype=np.int32)
                io = _lib.GenIO(ids=c.ids.data_ptr(), hiddens=c.hid.data_ptr(), finish=c.fin.data_ptr(), end_idx=c.end.data_ptr(), noise=None, n_draws=0, seed=c.seed,
                                utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
                _lib.check(c.lib.ctts_gpt_set_row_modes(c.h, _ptr(md), len(us)), "set_row_modes")
                try:
                    _lib.check(c.lib.ctts_gpt_begin(c.h, len(us), T_MAX, m.data_ptr(), C.byref(c.sc), C.byref(io), c.st), "begin")
                finally:
                    c.lib.ctts_gpt_set_row_modes(c.h, None, 0)
                _lib.check(c.lib.ctts_gpt_enable_text_rows(c.h, C.byref(c.tsc), c.tids.data_ptr(), c.st), "enable_text_rows")
                g._set_text_guide(c.st, tg)
                guides(us, us)
                _lib.check(c.lib.ctts_gpt_set_logprob_out(c.h, c.lp[0].data_ptr(), c.lp[1].data_ptr(), c.st), "set_logprob_out")
                _lib.check(real(c.h, e.data_ptr(), c.st), "prefill")
                _lib.check(c.lib.ctts_gpt_sample(c.h, c.st), "sample")
                c.mode_of.update({o: x for o, x in enumerate(modes)})
            mode_u.update(zip(us, modes)); lims.update(zip(us, ll))
        elif call[0] == "decode":
            c.decode(call[1])
        elif call[0] == "grow":
            assert c.grow(call[1]) == 0, c.lib.ctts_last_error().decode()
        else:
            _, rows, us, modes = call
            ll = [c.lims[u] if md == 0 else min(c.lims[u], TXT_NEW) for u, md in zip(us, modes)]
            guides(us, us)
            assert c.admit(rows, us, us, modes, ll) == 0, c.lib.ctts_last_error().decode()
            mode_u.update(zip(us, modes)); lims.update(zip(us, ll))
        if cancel_at is not None and call[0] == "decode":
            assert c.cancel([cancel_at]) == 0
            cancel_at = None
    c.decode(28)
    assert c.progress()[1] == 1
    return c, mode_u, lims


def _check_sentinels(c):
    """Mix.check_sentinels for rows that end by a sampled EOS: no utterance wrote into another's slot of any array, or beyond its own steps.  The step that samples
    EOS is written at index end_idx (as for code rows), so a text row that finished by EOS -- every guided one does -- holds EOS there and the fill behind it;
    Mix.check_sentinels expects the fill from end_idx on, which holds only for text rows that end by their limit."""
    from tests.test_gpu_session import FILL_F
    torch.cuda.synchronize()
    for o in range(c.ids.shape[0]):
        md = c.mode_of.get(o)
        n = int(c.end[o]) if md is not None else 0
        if md != 0:
            assert bool((c.ids[o] == FILL_I).all()) and bool((c.lp[:, o] == FILL_F).all()), f"slot {o} (mode {md}): code ids / log-probs were written"
        if md != 1:
            assert bool((c.tids[o] == FILL_I).all()), f"slot {o} (mode {md}): text ids were written"
        if md == 1:
            rep = c.tids[o, :n]
            assert bool((rep == rep[:, :1]).all()) and bool((rep != TEXT_EOS).all()), f"text slot {o}: its {n} tokens"
            m = n
            if int(c.fin[o]) == 1:
                assert bool((c.tids[o, n] == TEXT_EOS).all()), f"text slot {o}: finished by EOS, but index {n} does not hold it"
                m = n + 1
            assert bool((c.tids[o, m:] == FILL_I).all()), f"text slot {o}: ids beyond its {n} tokens"
        if md == 0:
            assert bool((c.ids[o, n + 1:] == FILL_I).all()), f"code slot {o}: ids beyond its {n} tokens"
        assert bool((c.hid[o, n + 1:] == FILL_F).all()), f"slot {o}: hidden rows beyond its {n} steps"
        if md is None:
            assert int(c.end[o]) == FILL_I and int(c.fin[o]) == FILL_I


@pytest.mark.parametrize("key", [(2, 1), (9, 2), (17, 3)])
def test_guided_text_rows_beside_code_rows(key):
    g = engine("fp32", INV, max_batch=20)
    text_us = [u for call in SCHEDULES[key] if call[0] != "decode" and call[0] != "grow"
               for u, md in zip(call[1] if call[0] == "begin" else call[2], call[2] if call[0] == "begin" else call[3]) if md == 1]
    guided = {u: _src(u, 3 + k) for k, u in enumerate(text_us)}
    c, mode_u, lims = _run_schedule(g, key, guided)
    _check_sentinels(c)
    plain, _, _ = _run_schedule(g, key, None)
    for u, md in mode_u.items():
        if md == 0:                                 # code rows: bit-identical to the same schedule without guides, and to their batch-1 call
            a, b = c.out(u), plain.out(u)
            assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:], f"code utterance {u} differs from the schedule without guides"
            _assert_equals_alone(a, _alone(g, u, "inv", lim=lims[u]), f"code utterance {u}")
        else:
            ids, n, fin = c.text_out(u)
            what = f"{key}: text utterance {u}"
            print(what, "src", guided[u], "->", ids[:, 0].tolist())
            assert fin == 1
            _check_structure(ids[:, 0].tolist(), guided[u], FREE5, 2, lims[u], what)
            one = _gen_text(g, [u], [lims[u]], TextGuide(FREE5, 2), [guided[u]])[0]
            assert ids[:, 0].tolist() == one, f"{what}: differs from its batch-1 guided call"


def test_a_reused_slot_gets_a_fresh_record_and_a_cancelled_row_is_a_prefix():
    """One output slot held first by a guided utterance, then by an unguided one (a stale cursor or a stale source would show), and the other way round; a guided
    row cancelled mid-way keeps a prefix of its uncancelled tokens."""
    g = engine("fp32", INV, max_batch=20)
    tg = TextGuide(FREE5, 2)
    srcs = {1: _src(1, 9), 4: _src(4, 4), 5: _src(5, 6)}

    def run(cancel):
        c = Mix(g, 6)
        real_begin = [0, 1, 2]                      # rows: code 0, text 1 (guided, 9 ids), text 2 (unguided)
        e, m = c._sel(real_begin)
        uid = np.ascontiguousarray([c.uids[u] for u in real_begin], dtype=np.uint64); lim = np.ascontiguousarray([6, TXT_NEW, 7], dtype=np.int32)
        md = np.ascontiguousarray([0, 1, 1], dtype=np.int32)
        io = _lib.GenIO(ids=c.ids.data_ptr(), hiddens=c.hid.data_ptr(), finish=c.fin.data_ptr(), end_idx=c.end.data_ptr(), noise=None, n_draws=0, seed=c.seed,
                        utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
        _lib.check(c.lib.ctts_gpt_set_row_modes(c.h, _ptr(md), 3), "set_row_modes")
        try:
            _lib.check(c.lib.ctts_gpt_begin(c.h, 3, T_MAX, m.data_ptr(), C.byref(c.sc), C.byref(io), c.st), "begin")
        finally:
            c.lib.ctts_gpt_set_row_modes(c.h, None, 0)
        _lib.check(c.lib.ctts_gpt_enable_text_rows(c.h, C.byref(c.tsc), c.tids.data_ptr(), c.st), "enable_text_rows")
        g._set_text_guide(c.st, tg)
        g._set_guides(c.st, [0, 1, 2], [None, srcs[1], None])
        _lib.check(c.lib.ctts_gpt_prefill(c.h, e.data_ptr(), c.st), "prefill")
        _lib.check(c.lib.ctts_gpt_sample(c.h, c.st), "sample")
        c.decode(4)
        if cancel:
            assert c.cancel([1]) == 0
        c.decode(TXT_NEW)
        first = [c.text_out(1), c.text_out(2)]
        first = [(a[:, 0].tolist(), n, f) for a, n, f in first]
        # the slots swap kinds: slot 1 (was guided) <- unguided utterance 4; slot 2 (was unguided) <- guided utterance 5
        c.tids[1:3] = FILL_I
        g._set_guides(c.st, [1, 2], [None, srcs[5]])
        assert c.admit([1, 2], [4, 5], [1, 2], [1, 1], [8, TXT_NEW]) == 0, c.lib.ctts_last_error().decode()
        c.decode(TXT_NEW + 1)
        second = [(a[:, 0].tolist(), n, f) for a, n, f in (c.text_out(1), c.text_out(2))]
        return first, second

    first, second = run(False)
    _check_structure(first[0][0], srcs[1], FREE5, 2, TXT_NEW, "slot 1, guided")
    assert first[0][2] == 1
    assert first[1][0] == _alone_text(g, 2, "inv", lim=7).tolist()
    assert second[0][0] == _alone_text(g, 4, "inv", lim=8).tolist(), "slot 1 re-used by an unguided utterance: a stale record"
    _check_structure(second[1][0], srcs[5], FREE5, 2, TXT_NEW, "slot 2 re-used by a guided utterance")
    assert second[1][2] == 1 and second[1][0] == _gen_text(g, [5], [TXT_NEW], tg, [srcs[5]])[0]
    cfirst, csecond = run(True)
    n = cfirst[0][1]
    assert cfirst[0][2] == 0 and 1 <= n < first[0][1] and cfirst[0][0] == first[0][0][:n], "the cancelled guided row's tokens are not a prefix of the uncancelled run"
    assert csecond == second


def test_engine_refusals():
    g = engine("fp32", INV, max_batch=20)
    c = Raw(g, 4)
    c.begin([0, 1])
    f = np.ascontiguousarray(FREE5, dtype=np.int32)
    assert c.lib.ctts_gpt_set_text_guide(c.h, _ptr(f), 5, 2, c.st) != 0 and "a guide on a code row" in c.lib.ctts_last_error().decode()
    c.decode(30)
    m = Mix(g, 4).begin([0, 1], [0, 1])
    bad = np.ascontiguousarray([TEXT_EOS], dtype=np.int32)
    assert m.lib.ctts_gpt_set_text_guide(m.h, _ptr(bad), 1, 2, m.st) != 0 and "is the EOS token" in m.lib.ctts_last_error().decode()
    g._set_text_guide(m.st, TextGuide(FREE5, 2))
    # a guide on a slot a code utterance is about to take, and a source that does not fit the admitted row's limit
    g._set_guides(m.st, [2], [_src(2, 5)])
    m.decode(24)
    assert m.admit([0], [2], [2], [0]) != 0 and "a guide on a code row" in m.lib.ctts_last_error().decode()
    assert m.admit([0], [2], [2], [1], [4]) != 0 and "needs 6 tokens" in m.lib.ctts_last_error().decode()
    assert m.admit([0], [2], [2], [1], [8]) == 0, m.lib.ctts_last_error().decode()
    m.decode(10)
    ids, n, fin = m.text_out(2)
    assert fin == 1
    _check_structure(ids[:, 0].tolist(), _src(2, 5), FREE5, 2, 8, "admitted after the refusals")


# ---- 5. the pipeline with the toy tokenizer ---------------------------------------------------------------------------------------------------------------
def test_pipeline_guided_refine(tmp_path):
    """infer(refine_guided=True, continuous=True, noise="device") and a refining SynthSession(refine_guided=True): the refined text's tokens, minus the free set,
    are the input's; the two agree; refine_guided=False is today's output.  (The toy tokenizer knows its tags; its words share one id, so the count and the tags
    are what the comparison sees.)"""
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, RefineTextParams, default_text_guide, refine_sources
    from tests.test_gpu_score import CFG4, LLAMA4
    g = GPT(LLAMA4, max_batch=8, max_seq_len=200, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(synth.gpt_state_dict(CFG4, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    tok = synth.toy_tokenizer(str(tmp_path / "tok"))
    texts = synth.toy_texts(4, 16, 18, seed=68)       # (long enough that infer neither splits nor merges them)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=24, min_new_token=4, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
    refine = RefineTextParams(prompt="[oral_2]", max_new_token=22, min_new_token=2, show_tqdm=False)
    seed = 4243
    try:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, tok, torch.device("cuda:0"))
        free = set(default_text_guide(tok).free_ids)
        bt = tok._tokenizer
        kw = dict(params_refine_text=refine, params_infer_code=params, noise="device", noise_seed=seed, slice_size=2, continuous=True, utt_ids=list(range(4)),
                  skip_refine_text=False, refine_text_only=True)      # (more texts than slice_size: the continuous path, whose refine pass takes the request seed)
        today = list(pipe.infer(list(texts), **kw))
        assert list(pipe.infer(list(texts), refine_guided=False, **kw)) == today, "refine_guided=False changes the output"
        guided = list(pipe.infer(list(texts), refine_guided=True, **kw))
        assert len(guided) == 1 and len(guided[0]) == 4
        want = []
        for u, t in enumerate(texts):
            ids, att, _ = pipe._refine_prompt([pipe.normalizer(t, True, True, None)], refine)
            src = refine_sources(tok, ids, att)[0]
            got = bt(guided[0][u], add_special_tokens=False)["input_ids"]
            print(f"utterance {u}: {t!r} -> {guided[0][u]!r}")
            assert not (set(src) & free) and [i for i in got if i not in free] == src, f"utterance {u}: the refined tokens minus the free set are not the input's"
            want.append(src)
        assert guided != today
        with pytest.raises(_lib.HipBackendError, match="needs max_new_token >="):
            list(pipe.infer(list(texts), refine_guided=True, **dict(kw, params_refine_text=RefineTextParams(prompt="[oral_2]", max_new_token=2, show_tqdm=False))))
        got = {}
        with pipe.open_session(params, seed=seed, return_details=True, refine=refine, refine_guided=True) as ses:
            tk = [ses.submit(texts[u], utt_id=u) for u in range(2)]
            got.update({t: (d, c) for t, d, c in ses.poll()})
            tk += [ses.submit(texts[u], utt_id=u) for u in range(2, 4)]
            got.update({t: (d, c) for t, d, c in ses.drain()})
        for u in range(4):
            d, cancelled = got[tk[u]]
            assert not cancelled and d.refined_text == guided[0][u], f"utterance {u}: the session refined {d.refined_text!r}, infer {guided[0][u]!r}"
        with pytest.raises(_lib.HipBackendError, match="refine_guided needs refine="):
            pipe.open_session(params, refine_guided=True)
        assert not g.busy
    finally:
        g.close()
