"""Serving session: an elastic decode batch (ctts_gpt_grow), cancellation (ctts_gpt_cancel), GPT.open_session / DecodeSession and
ChatTTSPlusPipeline.open_session / SynthSession.  Synthetic weights at real widths, 4 decoder layers, as tests/test_gpu_score.py builds them.

Checked here: under batch_invariant an utterance seated in a grown row -- across the persistent-launch limit, the split-decode threshold and the second 16-row
group, in the lanes a compaction freed, in text mode -- equals its own batch-1 generate bit for bit; in default mode every row's log-probs agree with GPT.score of
its own ids within the project's bounds (2e-4 fp32, FP16_TOL fp16) and the tokens written before a grow are those of the plain call; a cancel changes nothing for
the other rows, freezes the cancelled row's outputs and counts a row once; the session's bookkeeping (growth, compaction, out-slot recycling, first-token-EOS
re-admission, cancel of queued and seated tickets); the pipeline session against infer(continuous=True); refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs
from tests.helpers import gen_case_inputs, load_golden
from tests.test_gpu_gen_logprobs import HOT, SEED5, _restart_uid
from tests.test_gpu_score import CFG4, EOS, FP16_TOL, engine

pytestmark = pytest.mark.gpu

INV = dict(batch_invariant=1)
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
SEED, T_MAX, MAX_NEW, MIN_NEW, N_POOL = 9191, 14, 24, 4, 18
FILL_I, FILL_F = -7, -123.0
TEXT_EOS = 21177


def _pool():
    """18 ragged prompts of 6..14 tokens, left padded to 14; token limits 6..24 (the first of every group of three is long)"""
    rng = np.random.Generator(np.random.Philox(key=9192))
    lens = [int(x) for x in rng.integers(6, T_MAX + 1, size=N_POOL)]
    lims = [24 if u % 3 == 0 else int(x) for u, x in enumerate(rng.integers(6, 25, size=N_POOL))]
    ids, mask = synth.prompt_ids(N_POOL, T_MAX, CFG4["num_text_tokens"], seed=9193, pad_left=[T_MAX - x for x in lens])
    return lens, lims, ids, mask, [500 + u for u in range(N_POOL)]


class Raw:
    """One generate state driven through the C ABI: output arrays with `n_out` slots, pre-filled with sentinels"""

    def __init__(self, g, n_out, seed=SEED, text=False, min_new=MIN_NEW):
        self.g, self.lib, self.h, self.text = g, g._lib, g._h, text
        dev = g.device
        self.lens, self.lims, self.pids, self.pmask, self.uids = _pool()
        self.emb = g(torch.from_numpy(self.pids), torch.ones(N_POOL, T_MAX, dtype=torch.bool)).contiguous()
        self.msk = torch.from_numpy(self.pmask).to(dev).to(torch.int32).contiguous()
        if text:
            self.sc = sampler_cfg_from_objects(torch.tensor([0.7]), TEXT_EOS, MAX_NEW, 1, LW, [], 4, infer_text=True)
        else:
            self.sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, MAX_NEW, min_new, LW, LP, 4)
        self.ids = torch.full((n_out, MAX_NEW, 4), FILL_I, dtype=torch.int32, device=dev)
        self.hid = torch.full((n_out, MAX_NEW, 768), FILL_F, device=dev)
        self.lp = torch.full((2, n_out, MAX_NEW, 4), FILL_F, device=dev)
        self.fin = torch.full((n_out,), FILL_I, dtype=torch.int32, device=dev)
        self.end = torch.full((n_out,), FILL_I, dtype=torch.int32, device=dev)
        self.seed = seed
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.keep = []                                 # host / device arrays of asynchronous calls stay alive until the state is read

    def _sel(self, us):
        ii = torch.as_tensor(us, dtype=torch.long, device=self.g.device)
        e, m = self.emb.index_select(0, ii).contiguous(), self.msk.index_select(0, ii).contiguous()
        self.keep += [e, m]
        return e, m

    def begin(self, us, lims=None):
        e, m = self._sel(us)
        uid = np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64)
        lim = np.ascontiguousarray(lims or [self.lims[u] for u in us], dtype=np.int32)
        io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr(), finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(), noise=None, n_draws=0,
                        seed=self.seed, utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
        _lib.check(self.lib.ctts_gpt_begin(self.h, len(us), T_MAX, m.data_ptr(), C.byref(self.sc), C.byref(io), self.st), "begin")
        if not self.text:
            _lib.check(self.lib.ctts_gpt_set_logprob_out(self.h, self.lp[0].data_ptr(), self.lp[1].data_ptr(), self.st), "set_logprob_out")
        _lib.check(self.lib.ctts_gpt_prefill(self.h, e.data_ptr(), self.st), "prefill")
        _lib.check(self.lib.ctts_gpt_sample(self.h, self.st), "sample")
        return self

    def decode(self, n, graph=1):
        _lib.check(self.lib.ctts_gpt_decode(self.h, n, graph, self.st), "decode")

    def grow(self, n):
        return self.lib.ctts_gpt_grow(self.h, n, self.st)

    def cancel(self, rows):
        arr = np.ascontiguousarray(rows, dtype=np.int32)
        self.keep.append(arr)
        return self.lib.ctts_gpt_cancel(self.h, len(rows), arr.ctypes.data_as(C.c_void_p), self.st)

    def compact(self, keep):
        arr = np.ascontiguousarray(keep, dtype=np.int32)
        _lib.check(self.lib.ctts_gpt_compact(self.h, arr.ctypes.data_as(C.c_void_p), len(keep), self.st), "compact")

    def admit(self, rows, us, outs, lims=None):
        e, m = self._sel(us)
        arrs = [np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64),
                np.ascontiguousarray(lims or [self.lims[u] for u in us], dtype=np.int32), np.ascontiguousarray(outs, dtype=np.int32)]
        self.keep += arrs
        p = [a.ctypes.data_as(C.c_void_p) for a in arrs]
        return self.lib.ctts_gpt_admit(self.h, len(us), p[0], T_MAX, m.data_ptr(), e.data_ptr(), p[1], p[2], p[3], None, self.st)

    def progress(self):
        steps, alld = C.c_int32(0), C.c_int32(0)
        _lib.check(self.lib.ctts_gpt_progress(self.h, C.byref(steps), C.byref(alld), self.st), "progress")
        return int(steps.value), int(alld.value)

    def out(self, o):
        """what the engine wrote for output slot o: (ids [n,4], hiddens, logprobs, sampled_logprobs, end_idx, finish)"""
        torch.cuda.synchronize()
        n = int(self.end[o])
        return self.ids[o, :n].cpu().to(torch.long), self.hid[o, :n].cpu(), self.lp[0, o, :n].cpu(), self.lp[1, o, :n].cpu(), n, int(self.fin[o])


def _engine_lanes(g, B):
    """KV lane of decode rows 0..B-1 as the engine holds them (RowMeta.seq of meta_dec; synchronises)"""
    meta = np.zeros((_lib.MAX_BATCH, 4), dtype=np.int32)
    nb = C.c_size_t(0)
    st = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    _lib.check(g._lib.ctts_gpt_debug_read(g._h, b"meta_dec", meta.ctypes.data_as(C.c_void_p), meta.nbytes, C.byref(nb), st), "debug_read")
    return meta[:B, 0].tolist()


_alone_cache = {}


def _alone(g, u, key, seed=SEED, lim=None, uid=None, sampling=None, min_new=MIN_NEW):
    """utterance u of the pool through a batch-1 generate() on its trimmed prompt"""
    k = (key, u, seed, lim, uid, min_new, None if sampling is None else tuple(sorted((a, str(b)) for a, b in sampling.items())))
    if k not in _alone_cache:
        lens, lims, ids, mask, uids = _pool()
        T = lens[u]
        i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:])
        out = list(g.generate(g(i1, torch.ones(1, T, dtype=torch.bool)), i1, torch.tensor([0.3] * 4), EOS, attention_mask=torch.from_numpy(mask[u:u + 1, T_MAX - T:]),
                              max_new_token=MAX_NEW, min_new_token=min_new, logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="device", seed=seed,
                              utt_ids=[uid if uid is not None else uids[u]], max_new_tokens_per_row=[lim or lims[u]], return_logprobs=True,
                              sampling_per_row=None if sampling is None else [sampling]))[-1]
        _alone_cache[k] = (out.ids[0].cpu(), out.hiddens[0].cpu(), out.logprobs[0].cpu(), out.sampled_logprobs[0].cpu())
    return _alone_cache[k]


def _assert_equals_alone(got, one, what):
    ids, hid, lp, ls, n, _ = got
    assert n == one[0].shape[0], f"{what}: end_idx {n}, batch 1 wrote {one[0].shape[0]} tokens"
    assert n >= 1
    for name, a, b in (("ids", ids, one[0]), ("hiddens", hid, one[1]), ("logprobs", lp, one[2]), ("sampled_logprobs", ls, one[3])):
        assert torch.equal(a, b), f"{what}: {name} differ from the batch-1 generate"


# ---- 1. grow under batch_invariant ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(2, 2), (7, 3), (15, 3)])
def test_grow_under_batch_invariant_equals_batch_1(B, n):
    """2 -> 4 rows; 7 -> 10: across the 8-row persistent limit and the 9-row split-decode threshold; 15 -> 18: into the second 16-row group"""
    g = engine("fp32", INV, max_batch=20)
    c = Raw(g, B + n).begin(list(range(B)))
    c.decode(3)
    assert c.grow(n) == 0, c.lib.ctts_last_error().decode()
    new = list(range(B, B + n))
    assert c.admit(new, new, new) == 0, c.lib.ctts_last_error().decode()
    c.decode(MAX_NEW + 2)
    steps, alld = c.progress()
    assert alld == 1
    for u in range(B + n):
        _assert_equals_alone(c.out(u), _alone(g, u, "inv20"), f"{B} -> {B + n} rows, utterance {u}")


# ---- 2. lanes after a compaction ------------------------------------------------------------------------------------------------------------------
def test_grown_rows_take_the_lanes_a_compaction_freed():
    """rows 0 and 2 end by their limit of 4 tokens and are compacted away: rows 0, 1 now hold lanes 1, 3, the free lanes are 0, 2, 4..  A grown row that took
    lane 2 = B, or lane 1 / 3, would write its K / V over a live utterance's."""
    g = engine("fp32", INV, max_batch=20)
    c = Raw(g, 7).begin([0, 1, 2, 3], lims=[4, 24, 4, 24])
    c.decode(4)
    c.compact([1, 3])
    assert c.grow(3) == 0, c.lib.ctts_last_error().decode()
    assert _engine_lanes(g, 5) == [1, 3, 0, 2, 4], "the grown rows did not take the lowest free lanes"
    assert c.admit([2, 3, 4], [4, 5, 6], [4, 5, 6]) == 0, c.lib.ctts_last_error().decode()
    assert _engine_lanes(g, 5) == [1, 3, 0, 2, 4]
    c.decode(MAX_NEW + 2)
    assert c.progress()[1] == 1
    for u, lim in ((1, 24), (3, 24), (4, None), (5, None), (6, None)):
        _assert_equals_alone(c.out(u), _alone(g, u, "inv20", lim=lim), f"utterance {u}")
    assert c.out(0)[4] == 4 and c.out(2)[4] == 4


# ---- 3. default mode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_default_mode_grown_rows_agree_with_score(dtype):
    """3 -> 6 -> 10 rows (persistent launch, its two-item form on fp32, the launch chain); row 9 runs four steps as a dead row before it is seated"""
    g = engine(dtype, max_batch=20)
    plain = Raw(g, 3).begin([0, 1, 2], lims=[24, 24, 24])
    plain.decode(4)
    torch.cuda.synchronize()
    before = plain.ids[:, :5].cpu()
    c = Raw(g, 10).begin([0, 1, 2], lims=[24, 24, 24])
    c.decode(4)
    assert c.grow(3) == 0 and c.admit([3, 4, 5], [3, 4, 5], [3, 4, 5]) == 0, c.lib.ctts_last_error().decode()
    c.decode(4)
    assert c.grow(4) == 0 and c.admit([6, 7, 8], [6, 7, 8], [6, 7, 8]) == 0, c.lib.ctts_last_error().decode()
    c.decode(4)
    assert c.admit([9], [9], [9]) == 0, c.lib.ctts_last_error().decode()
    c.decode(MAX_NEW + 2)
    assert c.progress()[1] == 1
    outs = [c.out(u) for u in range(10)]
    assert torch.equal(c.ids[:3, :5].cpu(), before), "the tokens written before the first grow differ from the plain 3-row call's"
    codes = [o[0] for o in outs]
    assert all(cd.shape[0] >= MIN_NEW for cd in codes)
    si = score_inputs(torch.from_numpy(c.pids[:10]), torch.from_numpy(c.pmask[:10]), torch.ones(10, T_MAX, dtype=torch.bool), codes, EOS, append_eos=False)
    res = g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
    tol = 2e-4 if dtype == "fp32" else FP16_TOL
    for u in range(10):
        d = float((outs[u][2] - res.logprob[u]).abs().max())
        print(f"{dtype} utterance {u} ({codes[u].shape[0]} tokens): |logprobs - GPT.score| {d:.3e} (bound {tol:.1e})")
        assert d <= tol


# ---- 4. cancel ------------------------------------------------------------------------------------------------------------------------------------------
def test_cancel_freezes_one_row_and_leaves_the_others_alone():
    g = engine()
    lims = [24, 24, 13, 3]

    def run(cancel):
        c = Raw(g, 4).begin([0, 1, 2, 3], lims=lims)
        c.decode(4)                                    # 5 steps: row 3 has finished by its limit
        if cancel:
            assert c.cancel([1, 3]) == 0, c.lib.ctts_last_error().decode()
        c.decode(3)
        if cancel:
            assert c.cancel([1]) == 0                  # again, later: not counted twice
        c.decode(MAX_NEW)
        assert c.progress()[1] == 1
        return c, [c.out(u) for u in range(4)]

    a, A = run(False)
    b, B = run(True)
    for u in (0, 2, 3):
        for k, name in enumerate(("ids", "hiddens", "logprobs", "sampled_logprobs")):
            assert torch.equal(A[u][k], B[u][k]), f"row {u}: {name} differ between the run with the cancel and the run without"
        assert A[u][4:] == B[u][4:]
    assert A[1][4] > 5 and A[3][4] == 3
    assert B[1][4] == 5 and B[1][5] == 0, f"cancelled row: end_idx {B[1][4]}, finish {B[1][5]}"
    assert torch.equal(B[1][0], A[1][0][:5]) and torch.equal(B[1][1], A[1][1][:5]) and torch.equal(B[1][2], A[1][2][:5])
    assert bool((b.ids[1, 5:] == FILL_I).all()) and bool((b.hid[1, 5:] == FILL_F).all()) and bool((b.lp[:, 1, 5:] == FILL_F).all()), \
        "the cancelled row wrote beyond the step it was cancelled at"


def test_cancel_of_every_live_row_ends_the_batch_and_the_row_serves_again():
    g = engine(options=INV)
    c = Raw(g, 5).begin([0, 1, 2, 3], lims=[24, 24, 24, 24])
    c.decode(4)
    assert c.progress() == (5, 0)
    assert c.cancel([0, 1, 2, 3]) == 0, c.lib.ctts_last_error().decode()
    assert c.progress() == (5, 1)
    c.decode(4)                                        # exits on the device: nothing is written
    assert c.progress() == (5, 1)
    torch.cuda.synchronize()
    ends = c.end.cpu().tolist()[:4]
    assert all(MIN_NEW <= e <= 5 for e in ends) and 5 in ends, ends
    assert all(f == 0 for f, e in zip(c.fin.cpu().tolist()[:4], ends) if e == 5)
    assert c.admit([1], [7], [4]) == 0, c.lib.ctts_last_error().decode()
    assert c.progress()[1] == 0
    c.decode(MAX_NEW + 1)
    assert c.progress()[1] == 1
    _assert_equals_alone(c.out(4), _alone(g, 7, "inv8"), "the utterance admitted into the cancelled row")
    assert c.end.cpu().tolist()[:4] == ends


# ---- 5. DecodeSession -------------------------------------------------------------------------------------------------------------------------------------
def test_decode_session_under_batch_invariant():
    g = engine(options=INV)
    lens, _, ids, mask, uids = _pool()
    uids = list(uids[:8])
    uids[4] = _restart_uid()                           # its first token is EOS at attempt 0 under the HOT knobs, not at attempt 1
    lims = [24, 24, 10, 24, 24, 6, 24, 24]
    per = [None] * 8
    per[4] = dict(HOT)
    emb = g(torch.from_numpy(ids[:8]), torch.ones(8, T_MAX, dtype=torch.bool))
    msk = torch.from_numpy(mask[:8])
    got = {}
    with g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, min_new_token=MIN_NEW, logits_warpers=LW, logits_processors=LP, return_hidden=True,
                        return_logprobs=True, seed=SEED5, rows=8, out_slots=5) as ses:
        with pytest.raises(_lib.HipBackendError, match="already running"):
            list(g.generate(emb[:1], torch.from_numpy(ids[:1]), torch.tensor([0.3] * 4), EOS, max_new_token=4))
        with pytest.raises(_lib.HipBackendError, match="session"):
            g.close()
        assert ses.step() == []                        # nothing queued, nothing live: nothing launched
        assert ses.launched == 0
        tk = [ses.submit(emb[u], msk[u], uids[u], limit=lims[u], sampling=per[u]) for u in range(3)]
        for _ in range(2):
            for r in ses.step():
                got[r.ticket] = r
            assert ses.book.lanes == _engine_lanes(g, 3) == [0, 1, 2]
        tk += [ses.submit(emb[u], msk[u], uids[u], limit=lims[u], sampling=per[u]) for u in range(3, 8)]
        assert ses.cancel(tk[7]) and ses.cancel(tk[1]) and not ses.cancel(tk[7])
        lanes_seen = set()
        while not ses.book.idle():
            for r in ses.step():
                assert r.ticket not in got
                got[r.ticket] = r
            # the host's mirror of the rows' KV lanes (SessionBook.lanes) is what the engine holds, through growth and compaction
            assert ses.book.lanes == _engine_lanes(g, len(ses.book.lanes)), f"lane mirror {ses.book.lanes} after {ses.batch_trace}"
            lanes_seen.add(tuple(ses.book.lanes))
        assert any(list(l) != list(range(len(l))) for l in lanes_seen), "the lanes never left the identity: the mirror was not put to the test"
        trace = list(ses.batch_trace)
        assert ses.step() == []
    assert not g.busy
    print(f"batch_trace {trace}")
    assert sorted(got) == tk
    sizes = [b for _, b in trace]
    assert sizes[0] == 3 and max(sizes) > 3, "the batch never grew"
    assert min(sizes[sizes.index(max(sizes)):]) < max(sizes), "no compaction after the growth"
    assert got[tk[7]].cancelled and got[tk[7]].ids.shape[0] == 0
    for u in (0, 2, 3, 4, 5, 6):
        r = got[tk[u]]
        one = _alone(g, u, "inv8", seed=SEED5, lim=lims[u], uid=uids[u], sampling=per[u])
        assert not r.cancelled and r.utt_id == uids[u]
        _assert_equals_alone((r.ids.cpu(), r.hiddens.cpu(), r.logprobs.cpu(), r.sampled_logprobs.cpu(), int(r.ids.shape[0]), 0), one, f"utterance {u}")
    assert got[tk[4]].attempt == 1, "the first-token-EOS utterance was not admitted again with its next attempt"
    assert all(got[tk[u]].attempt == 0 for u in (0, 2, 3, 5, 6))
    r, one = got[tk[1]], _alone(g, 1, "inv8", seed=SEED5, lim=lims[1], uid=uids[1])
    n = int(r.ids.shape[0])
    assert r.cancelled and 1 <= n < one[0].shape[0], f"the seated utterance wrote {n} of {one[0].shape[0]} tokens before its cancel"
    assert torch.equal(r.ids.cpu(), one[0][:n]) and torch.equal(r.hiddens.cpu(), one[1][:n]) and torch.equal(r.logprobs.cpu(), one[2][:n])


def _adapter(key, targets):
    rng = np.random.Generator(np.random.Philox(key=key))
    return [(l, t, (rng.standard_normal((8, 768 if t != "down_proj" else 3072)) * 0.05).astype(np.float32),
             (rng.standard_normal((3072 if t in ("gate_proj", "up_proj") else 768, 8)) * 0.05).astype(np.float32), 2.0) for l in range(4) for t in targets]


def test_decode_session_with_per_utterance_adapters():
    """Default mode (batch_invariant refuses per-utterance adapters): utterances with and without an adapter slot, seated at begin, in grown rows and in rows a
    finished utterance left (whose slot must not stick); the second adapter is loaded while two decode chunks are in flight.  Every utterance's log-probs agree
    with GPT.score of its own ids under its own adapter within 2e-4, the bound of the same comparison without adapters (test 3); scored under another utterance's
    slot they do not."""
    g = engine()
    lens, _, ids, mask, uids = _pool()
    slots = [0, -1, 0, 1, -1, 1, 0, -1]
    lims = [24, 6, 24, 24, 24, 8, 24, 24]
    emb = g(torch.from_numpy(ids[:8]), torch.ones(8, T_MAX, dtype=torch.bool))
    msk = torch.from_numpy(mask[:8])
    got = {}
    try:
        g.load_adapter(0, _adapter(91, ("q_proj", "k_proj", "v_proj", "o_proj")))
        with g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, min_new_token=MIN_NEW, logits_warpers=LW, logits_processors=LP, return_logprobs=True, seed=SEED,
                            rows=6) as ses:
            tk = [ses.submit(emb[u], msk[u], uids[u], limit=lims[u], adapter_slot=slots[u]) for u in range(3)]
            for _ in range(3):
                got.update({r.ticket: r for r in ses.step()})
            g.load_adapter(1, _adapter(92, ("q_proj", "v_proj", "gate_proj", "down_proj")))      # two chunks are enqueued
            tk += [ses.submit(emb[u], msk[u], uids[u], limit=lims[u], adapter_slot=slots[u]) for u in range(3, 8)]
            got.update({r.ticket: r for r in ses.drain()})
            trace = list(ses.batch_trace)
        print(f"batch_trace {trace}")
        assert max(b for _, b in trace) > 3 and sorted(got) == tk
        codes = [got[tk[u]].ids.cpu() for u in range(8)]
        assert all(c.shape[0] >= MIN_NEW for c in codes)
        si = score_inputs(torch.from_numpy(ids[:8]), torch.from_numpy(mask[:8]), torch.ones(8, T_MAX, dtype=torch.bool), codes, EOS, append_eos=False)

        def scored(sl):
            g.set_row_adapters(sl)
            try:
                return g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
            finally:
                g.set_row_adapters(None)
        own, other = scored(slots), scored([{0: 1, 1: -1, -1: 0}[s] for s in slots])
        for u in range(8):
            lp = got[tk[u]].logprobs.cpu()
            d, d_other = float((lp - own.logprob[u]).abs().max()), float((lp - other.logprob[u]).abs().max())
            print(f"utterance {u} (slot {slots[u]}, {codes[u].shape[0]} tokens): |logprobs - GPT.score| {d:.3e} under its own slot (bound 2.0e-04), {d_other:.3e} under another")
            assert d <= 2e-4
            assert d_other > 1e-3, f"utterance {u}: scoring under another slot changes nothing -- its adapter was not applied"
    finally:
        g.set_row_adapters(None)


# ---- 6. text mode ---------------------------------------------------------------------------------------------------------------------------------------
def test_text_mode_grow_equals_batch_1():
    g = engine(options=INV)
    c = Raw(g, 3, text=True).begin([0, 1], lims=[24, 24])
    c.decode(3)
    assert c.grow(1) == 0 and c.admit([2], [2], [2], lims=[24]) == 0, c.lib.ctts_last_error().decode()
    c.decode(MAX_NEW + 2)
    assert c.progress()[1] == 1
    for u in range(3):
        T = c.lens[u]
        i1 = torch.from_numpy(c.pids[u:u + 1, T_MAX - T:])
        one = list(g.generate(g(i1, torch.ones(1, T, dtype=torch.bool)), i1, torch.tensor([0.7]), TEXT_EOS, attention_mask=torch.from_numpy(c.pmask[u:u + 1, T_MAX - T:]),
                              max_new_token=MAX_NEW, min_new_token=1, logits_warpers=LW, infer_text=True, return_hidden=True, noise="device", seed=SEED,
                              utt_ids=[c.uids[u]]))[-1]
        ids, hid, _, _, n, _ = c.out(u)
        assert n == one.ids[0].shape[0] and n >= 1, f"text utterance {u}: {n} vs {one.ids[0].shape[0]} tokens"
        assert torch.equal(ids[:, 0], one.ids[0].cpu()) and torch.equal(hid, one.hiddens[0].cpu()), f"text utterance {u} differs from its batch-1 run"


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------------------------------------
def test_synth_session_matches_infer_continuous(tmp_path):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, InferDetails
    from tests.test_gpu_score import LLAMA4
    g = GPT(LLAMA4, max_batch=8, max_seq_len=160, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(synth.gpt_state_dict(CFG4, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    tok = synth.toy_tokenizer(str(tmp_path / "tok"))
    texts = synth.toy_texts(6, 8, 30, seed=68)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=24, min_new_token=4, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
    try:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, tok, torch.device("cuda:0"))
        ref = list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", noise_seed=4242, slice_size=4, continuous=True,
                              return_details=True))
        assert len(ref) == 1 and isinstance(ref[0], InferDetails)
        ref = ref[0]
        got = {}
        with pipe.open_session(params, seed=4242, return_details=True) as ses:
            tk = [ses.submit(texts[u], utt_id=u) for u in range(3)]
            for _ in range(2):
                got.update({t: (d, c) for t, d, c in ses.poll()})
            tk += [ses.submit(texts[u], utt_id=u) for u in range(3, 6)]
            got.update({t: (d, c) for t, d, c in ses.drain()})
            assert max(b for _, b in ses.batch_trace) > 3
        assert not g.busy
        for u in range(6):
            d, cancelled = got[tk[u]]
            assert not cancelled
            assert torch.equal(d.ids.cpu(), ref.ids[u].cpu()), f"utterance {u}: token ids differ from infer(continuous=True)"
            a, b = ref.wavs[u].cpu().numpy(), d.wav.cpu().numpy()
            assert a.shape == b.shape and a.shape[0] == 256 * (2 * d.ids.shape[0] - 1)
            rel = float(np.sqrt(np.mean((a - b) ** 2))) / float(np.sqrt(np.mean(a ** 2)))
            print(f"utterance {u}: wav rms difference {rel:.3e} relative (bound 1e-4)")
            assert rel <= 1e-4
        # out of scope inside a session: refused with a message, the engine stays free
        for kw, what in ((dict(num_candidates=4), "num_candidates"), (dict(noise="torch"), "caller-supplied noise"), (dict(stream=True), "streaming"),
                         (dict(sharded=True), "infer_sharded"), (dict(refine_text_only=True), "refine-text"), (dict(share_prompt=True), "shared prompt")):
            with pytest.raises(_lib.HipBackendError, match=what):
                pipe.open_session(params, **kw)
            assert not g.busy
        with pytest.raises(TypeError, match="unexpected keyword argument 'slice_size'"):
            pipe.open_session(params, slice_size=4)
        assert not g.busy
    finally:
        g.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_next_plain_call():
    """Every refusal of ctts_gpt_grow / ctts_gpt_cancel / open_session, each followed by a plain generate() of the reference-minted fixture's first slice
    (tests/golden gpt_real_device_noise: 20 layers, slices of 4)."""
    from chatttsplus_amd.hip_models import GPT
    from tests.test_gpu_gpt import LLAMA
    z, meta = load_golden("gpt_real_device_noise")
    sd, ids, mask, _ = gen_case_inputs(meta, synth.GPT_REAL)
    seed, uids, N = int(meta["noise_seed"]), [int(u) for u in meta["utt_ids"]], int(meta["max_new"])
    g = GPT(LLAMA, max_batch=4, max_seq_len=96, weight_dtype="fp32")
    g.load_state_dict(sd)
    lib, h, dev = g._lib, g._h, g.device
    ids_t, mask_t = torch.from_numpy(ids[:4]), torch.from_numpy(mask[:4])
    T = ids.shape[1]
    emb = g(ids_t, torch.ones(4, T, dtype=torch.bool)).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def plain(after):
        out = list(g.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, attention_mask=mask_t, max_new_token=N, min_new_token=int(meta["min_new"]), logits_warpers=LW,
                              logits_processors=LP, return_hidden=True, noise="device", seed=seed, utt_ids=uids[:4]))[-1]
        for b in range(4):
            n = int(z["lens"][b])
            assert out.ids[b].shape[0] == n and np.array_equal(out.ids[b].cpu().numpy(), z["ids"][b, :n].astype(np.int64)), f"after {after}: utterance {b}"

    def refused(rc, text, after):
        assert rc != 0 and text in lib.ctts_last_error().decode(), f"{after}: rc {rc}, message {lib.ctts_last_error().decode()!r}"
        torch.cuda.synchronize()
        plain(after)

    try:
        rows = np.ascontiguousarray([0, 1, 1, 5, -1], dtype=np.int32)
        p = rows.ctypes.data
        # no generate state: the engine has not begun anything yet (a finished generate() leaves its rows behind: that state is legal to grow)
        assert lib.ctts_gpt_grow(h, 1, st) != 0 and "grow: no generate state" in lib.ctts_last_error().decode()
        refused(lib.ctts_gpt_cancel(h, 1, C.c_void_p(p), st), "cancel: no generate state", "grow and cancel before any begin")
        out = dict(ids=torch.empty(4, 8, 4, dtype=torch.int32, device=dev), fin=torch.zeros(4, dtype=torch.int32, device=dev), end=torch.zeros(4, dtype=torch.int32, device=dev))
        sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, 8, 2, LW, LP, 4)
        msk = mask_t.to(dev).to(torch.int32).contiguous()

        def begin(noise=None):
            io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(),
                            noise=noise.data_ptr() if noise is not None else None, n_draws=2 if noise is not None else 0, seed=3)
            _lib.check(lib.ctts_gpt_begin(h, 2, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
            _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
            _lib.check(lib.ctts_gpt_sample(h, st), "sample")

        begin()
        refused(lib.ctts_gpt_grow(h, 0, st), "grow: n=0", "grow(0)")
        begin()
        refused(lib.ctts_gpt_grow(h, 3, st), "exceed max_batch=4", "grow past max_batch")
        begin()
        refused(lib.ctts_gpt_cancel(h, 1, C.c_void_p(p + 12), st), "cancel: row 5 of 2", "cancel of a row outside the batch")
        begin()
        refused(lib.ctts_gpt_cancel(h, 1, C.c_void_p(p + 16), st), "cancel: row -1 of 2", "cancel of a negative row")
        begin()
        refused(lib.ctts_gpt_cancel(h, 3, C.c_void_p(p), st), "cancel: row 1 named twice", "cancel naming a row twice")
        noise = torch.empty(2, 8, 626, device=dev).exponential_()
        begin(noise)
        refused(lib.ctts_gpt_grow(h, 1, st), "grow: device noise only", "grow with caller-supplied noise")
        # ... and the calls go through on the same state
        begin()
        assert lib.ctts_gpt_grow(h, 2, st) == 0 and lib.ctts_gpt_cancel(h, 2, C.c_void_p(p), st) == 0
        _lib.check(lib.ctts_gpt_decode(h, 4, 1, st), "decode")
        torch.cuda.synchronize()
        plain("a grow and a cancel that went through")
        # the host object: out of scope inside a session, a prompt that does not fit, an engine that is busy
        for kw, what in ((dict(prompt_of=[0, 0]), "shared prompt passes"), (dict(num_candidates=2), "num_candidates"), (dict(noise=noise), "caller-supplied noise"),
                         (dict(stream=True), "streaming windows"), (dict(sharded=True), "infer_sharded"), (dict(infer_text=True), "refine-text pass")):
            with pytest.raises(_lib.HipBackendError, match=what):
                g.open_session(torch.tensor([0.3] * 4), 625, N, **kw)
            assert not g.busy
        with pytest.raises(_lib.HipBackendError, match="rows=5 outside"):
            g.open_session(torch.tensor([0.3] * 4), 625, N, rows=5)
        plain("the refused open_session calls")
        ses = g.open_session(torch.tensor([0.3] * 4), 625, 80, seed=1)
        with pytest.raises(_lib.HipBackendError, match="exceed max_seq_len=96"):
            ses.submit(emb[0], mask_t[0], 1)           # 20 + 80 > 96
        with pytest.raises(_lib.HipBackendError, match="is live on this engine"):
            g.score(emb, mask_t, torch.zeros(4, 1, 4, dtype=torch.long), [1] * 4)
        with pytest.raises(_lib.HipBackendError, match="already running"):
            g.open_session(torch.tensor([0.3] * 4), 625, N)
        ses.close()
        with pytest.raises(_lib.HipBackendError, match="closed"):
            ses.step()
        plain("a session that refused its only prompt")
    finally:
        g.close()
