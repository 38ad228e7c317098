"""Text rows beside code rows in one decode batch (ctts_gpt_enable_text_rows / ctts_gpt_set_row_modes / ctts_gpt_admit_modes; RowState.mode), and what is built
on them: GPT.open_session(text_rows=...) / DecodeSession.submit(mode="text"), ChatTTSPlusPipeline.open_session(refine=...).  Synthetic weights at real widths,
4 decoder layers, the prompt pool of tests/test_gpu_session.py.

Checked here: under batch_invariant every text row -- seated by begin, admitted into a freed row, admitted into a grown row -- equals its batch-1
generate(infer_text=True) bit for bit and every code row its batch-1 generate (ids, hiddens, both log-probs), at 2, 3, 9 and 17 rows; sentinel fills show that no
utterance wrote into another's slot; in default mode a lone text row equals the text-mode call and the code rows' log-probs agree with GPT.score within the
project's bounds; the bookkeeping (row reports, cancel, "text_rows_live", all_done); the off path on the reference-minted golden; the two sessions; refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs
from tests.helpers import gen_case_inputs, load_golden
from tests.test_gpu_score import EOS, FP16_TOL, engine
from tests.test_gpu_session import (FILL_F, FILL_I, INV, LP, LW, MAX_NEW, MIN_NEW, SEED, T_MAX, TEXT_EOS, Raw, _alone, _assert_equals_alone, _engine_lanes, _pool)

pytestmark = pytest.mark.gpu

TXT_NEW = 20          # the text rows' max_new_token: below the code rows' 24, so the text ids array has a stride of its own
TXT_T, TXT_MIN = 0.7, 1


def _text_sc(max_new=TXT_NEW, **kw):
    return sampler_cfg_from_objects(torch.tensor([TXT_T]), TEXT_EOS, max_new, TXT_MIN, LW, kw.get("processors", []), 4, infer_text=True)


class Mix(Raw):
    """A code-mode generate state with text rows enabled: `tids` are the text rows' ids, slots shared with the code arrays"""

    def __init__(self, g, n_out, seed=SEED, hiddens=True):
        super().__init__(g, n_out, seed=seed)
        self.tsc = _text_sc()
        self.tids = torch.full((n_out, TXT_NEW, 4), FILL_I, dtype=torch.int32, device=g.device)
        self.hiddens = hiddens
        self.mode_of = {}                              # output slot -> mode of the utterance that holds it

    def opt(self, name):
        v = C.c_int(0)
        _lib.check(self.lib.ctts_gpt_get_option(self.h, name.encode(), C.byref(v)), "get_option")
        return int(v.value)

    def begin(self, us, modes=None, lims=None, enable=True, trim=False):
        """`trim` (one utterance): its prompt without the pool's left padding, as the batch-1 references run it"""
        modes = modes or [0] * len(us)
        e, m = self._sel(us)
        T = T_MAX
        if trim:
            assert len(us) == 1
            T = self.lens[us[0]]
            e, m = e[:, T_MAX - T:].contiguous(), m[:, T_MAX - T:].contiguous()
            self.keep += [e, m]
        uid = np.ascontiguousarray([self.uids[u] for u in us], dtype=np.uint64)
        lim = np.ascontiguousarray(lims or [self.lims[u] for u in us], dtype=np.int32)
        md = np.ascontiguousarray(modes, dtype=np.int32)
        io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr() if self.hiddens else None, finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(),
                        noise=None, n_draws=0, seed=self.seed, utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
        _lib.check(self.lib.ctts_gpt_set_row_modes(self.h, md.ctypes.data_as(C.c_void_p), len(us)), "set_row_modes")
        try:
            _lib.check(self.lib.ctts_gpt_begin(self.h, len(us), T, m.data_ptr(), C.byref(self.sc), C.byref(io), self.st), "begin")
        finally:
            self.lib.ctts_gpt_set_row_modes(self.h, None, 0)
        if enable:
            _lib.check(self.lib.ctts_gpt_enable_text_rows(self.h, C.byref(self.tsc), self.tids.data_ptr(), self.st), "enable_text_rows")
        _lib.check(self.lib.ctts_gpt_set_logprob_out(self.h, self.lp[0].data_ptr(), self.lp[1].data_ptr(), self.st), "set_logprob_out")
        _lib.check(self.lib.ctts_gpt_prefill(self.h, e.data_ptr(), self.st), "prefill")
        _lib.check(self.lib.ctts_gpt_sample(self.h, self.st), "sample")
        self.mode_of.update({o: md_ for o, md_ in enumerate(modes)})
        return self

    def admit(self, rows, us, outs, modes=None, lims=None):
        if modes is not None:
            arrs = [np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(modes, dtype=np.int32)]
            self.keep += arrs
            rc = self.lib.ctts_gpt_admit_modes(self.h, len(us), arrs[0].ctypes.data_as(C.c_void_p), arrs[1].ctypes.data_as(C.c_void_p), self.st)
            if rc:
                return rc
        rc = super().admit(rows, us, outs, lims=lims)
        if rc == 0:
            self.mode_of.update({o: md_ for o, md_ in zip(outs, modes or [0] * len(us))})
        return rc

    def text_out(self, o):
        torch.cuda.synchronize()
        n = int(self.end[o])
        return self.tids[o, :n].cpu().to(torch.long), n, int(self.fin[o])

    def check_sentinels(self):
        """no utterance wrote into another's slot of any array, or beyond its own steps (slots never seated keep every fill)"""
        torch.cuda.synchronize()
        for o in range(self.ids.shape[0]):
            md = self.mode_of.get(o)
            n = int(self.end[o]) if md is not None else 0
            if md != 0:
                assert bool((self.ids[o] == FILL_I).all()) and bool((self.lp[:, o] == FILL_F).all()), f"slot {o} (mode {md}): code ids / log-probs were written"
            if md != 1:
                assert bool((self.tids[o] == FILL_I).all()), f"slot {o} (mode {md}): text ids were written"
            if md == 1:
                rep = self.tids[o, :n]
                assert bool((rep == rep[:, :1]).all()) and bool((self.tids[o, n:] == FILL_I).all()), f"text slot {o}: ids beyond its {n} tokens"
            if md == 0:
                assert bool((self.ids[o, n + 1:] == FILL_I).all()), f"code slot {o}: ids beyond its {n} tokens"
            assert bool((self.hid[o, n + 1:] == FILL_F).all()), f"slot {o}: hidden rows beyond its {n} steps"
            if md is None:
                assert int(self.end[o]) == FILL_I and int(self.fin[o]) == FILL_I


_text_cache = {}


def _alone_text(g, u, key, seed=SEED, lim=None, max_new=TXT_NEW):
    """utterance u of the pool through a batch-1 generate(infer_text=True) on its trimmed prompt: ids [n]"""
    k = (key, u, seed, lim, max_new)
    if k not in _text_cache:
        lens, lims, ids, mask, uids = _pool()
        T = lens[u]
        i1 = torch.from_numpy(ids[u:u + 1, T_MAX - T:])
        out = list(g.generate(g(i1, torch.ones(1, T, dtype=torch.bool)), i1, torch.tensor([TXT_T]), TEXT_EOS, attention_mask=torch.from_numpy(mask[u:u + 1, T_MAX - T:]),
                              max_new_token=max_new, min_new_token=TXT_MIN, logits_warpers=LW, infer_text=True, noise="device", seed=seed, utt_ids=[uids[u]],
                              max_new_tokens_per_row=[min(lim or lims[u], max_new)]))[-1]
        _text_cache[k] = out.ids[0].cpu()
    return _text_cache[k]


def _assert_text_equals_alone(c, o, one, what):
    ids, n, _ = c.text_out(o)
    assert n == one.shape[0] and n >= 1, f"{what}: end_idx {n}, the batch-1 infer_text call wrote {one.shape[0]} tokens"
    assert torch.equal(ids[:, 0], one), f"{what}: ids differ from the batch-1 generate(infer_text=True)"


# every case: [(call, ...)] -- begin(us, modes, lims) | decode(n) | admit(rows, us, modes) | grow(n); utterance u writes output slot u
SCHEDULES = {
    (2, 1): [("begin", [0], [0], [3]), ("decode", 4), ("admit", [0], [1], [1]), ("grow", 1), ("admit", [1], [2], [0])],
    (3, 2): [("begin", [0, 1], [1, 0], [None, 3]), ("decode", 4), ("admit", [1], [2], [1]), ("grow", 1), ("admit", [2], [3], [0])],
    (9, 2): [("begin", list(range(7)), [0, 1, 0, 0, 0, 0, 0], [3] + [None] * 6), ("decode", 4), ("admit", [0], [7], [0]), ("grow", 2), ("admit", [7, 8], [8, 9], [1, 0])],
    (17, 3): [("begin", list(range(15)), [0, 1] + [0] * 13, [3] + [None] * 14), ("decode", 4), ("admit", [0], [15], [1]), ("grow", 2), ("admit", [15, 16], [16, 17], [1, 0])],
}


# ---- 1. batch-invariant equality through the C ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", sorted(SCHEDULES))
def test_text_rows_under_batch_invariant_equal_batch_1(B, n):
    """(2, 1): the 2-row case; (3, 2); (9, 2): across the 8 -> 9 row boundary; (17, 3): into the second 16-row group.  Text rows are seated by begin, by admit
    into a freed row and by grow + admit.  After every step the engine's rows (meta_dec: KV lanes) and its "text_rows_live" equal the host's mirror."""
    g = engine("fp32", INV, max_batch=20)
    c = Mix(g, 18)
    lims, mode_u, rows_mode, lanes = {}, {}, [], []

    def watch(steps):
        for _ in range(steps):
            c.decode(1)
            assert _engine_lanes(g, len(lanes)) == lanes, "meta_dec: the rows' KV lanes differ from the host mirror"
            assert c.opt("text_rows_live") == sum(rows_mode)

    for call in SCHEDULES[(B, n)]:
        if call[0] == "begin":
            _, us, modes, lm = call
            ll = [(x or c.lims[u]) if m == 0 else min(x or c.lims[u], TXT_NEW) for u, m, x in zip(us, modes, lm)]
            c.begin(us, modes, ll)
            lims.update(zip(us, ll)); mode_u.update(zip(us, modes))
            rows_mode, lanes = list(modes), list(range(len(us)))
        elif call[0] == "decode":
            watch(call[1])
        elif call[0] == "grow":
            assert c.grow(call[1]) == 0, c.lib.ctts_last_error().decode()
            rows_mode += [0] * call[1]
            lanes += list(range(len(lanes), len(lanes) + call[1]))      # (no compaction in these schedules: the lowest free lanes are B ..)
        else:
            _, rows, us, modes = call
            ll = [c.lims[u] if m == 0 else min(c.lims[u], TXT_NEW) for u, m in zip(us, modes)]
            assert c.admit(rows, us, us, modes, ll) == 0, c.lib.ctts_last_error().decode()
            lims.update(zip(us, ll)); mode_u.update(zip(us, modes))
            for r, m in zip(rows, modes):
                rows_mode[r] = m
            assert c.opt("text_rows_live") == sum(rows_mode)
    assert len(rows_mode) == B and sum(rows_mode) == n
    watch(2)
    c.decode(MAX_NEW + 2)
    assert c.progress()[1] == 1
    assert sum(mode_u.values()) >= n
    for u, m in sorted(mode_u.items()):
        if m == 1:
            _assert_text_equals_alone(c, u, _alone_text(g, u, "inv20", lim=lims[u]), f"{B} rows, text utterance {u}")
        else:
            _assert_equals_alone(c.out(u), _alone(g, u, "inv20", lim=lims[u]), f"{B} rows, code utterance {u}")
    c.check_sentinels()


# ---- 2. default mode ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_default_mode_lone_text_row_and_code_rows_against_score(dtype):
    """A lone text row of a text-rows-enabled code state runs the kernels of generate(infer_text=True) at batch 1 (the persistent launch without fused heads, the text
    head's launch, the text sampler): the same ids.  9 rows of which 2 are text rows (the launch chain): every code row's log-probs agree with GPT.score of its own ids within
    the bounds of test_default_mode_grown_rows_agree_with_score (2e-4 fp32, FP16_TOL fp16)."""
    g = engine(dtype, max_batch=20)
    c = Mix(g, 1).begin([1], [1], [TXT_NEW], trim=True)      # the very prompt of the batch-1 call: outside batch_invariant the left padding regroups sums
    assert c.opt("text_rows_live") == 1
    c.decode(MAX_NEW + 1)
    assert c.progress()[1] == 1
    _assert_text_equals_alone(c, 0, _alone_text(g, 1, f"def20-{dtype}", lim=TXT_NEW), f"{dtype}: the lone text row")
    modes = [0, 1, 0, 0, 1, 0, 0, 0, 0]
    c = Mix(g, 9).begin(list(range(3)), modes[:3], [24, TXT_NEW, 24])
    c.decode(4)
    assert c.grow(6) == 0 and c.admit(list(range(3, 9)), list(range(3, 9)), list(range(3, 9)), modes[3:], [24, TXT_NEW] + [24] * 4) == 0, c.lib.ctts_last_error().decode()
    c.decode(MAX_NEW + 2)
    assert c.progress()[1] == 1
    c.check_sentinels()
    code = [u for u in range(9) if modes[u] == 0]
    outs = {u: c.out(u) for u in code}
    codes = [outs[u][0] for u in code]
    assert all(cd.shape[0] >= MIN_NEW for cd in codes) and all(c.text_out(u)[1] >= 1 for u in (1, 4))
    si = score_inputs(torch.from_numpy(c.pids[code]), torch.from_numpy(c.pmask[code]), torch.ones(len(code), T_MAX, dtype=torch.bool), codes, EOS, append_eos=False)
    res = g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
    tol = 2e-4 if dtype == "fp32" else FP16_TOL
    for i, u in enumerate(code):
        d = float((outs[u][2] - res.logprob[i]).abs().max())
        print(f"{dtype} code utterance {u} ({codes[i].shape[0]} tokens) beside 2 text rows: |logprobs - GPT.score| {d:.3e} (bound {tol:.1e})")
        assert d <= tol


# ---- 3. bookkeeping -----------------------------------------------------------------------------------------------------------------------------------------
def _row_report(c, B):
    pin = torch.zeros(2 * B, dtype=torch.int32).pin_memory()
    _lib.check(c.lib.ctts_gpt_rows_enqueue(c.h, pin.data_ptr(), c.st), "rows_enqueue")
    torch.cuda.synchronize()
    return pin.view(-1, 2).tolist()


def test_text_row_bookkeeping():
    g = engine("fp32", INV, max_batch=20)

    def schedule(modes):
        """4 rows; row 2 is cancelled after 4 steps; after 7 steps row 2 is compacted away and row 1 (ended by its limit of 5) is handed to code utterance 4"""
        c = Mix(g, 5).begin([0, 1, 2, 3], modes, [24, 5, TXT_NEW, 24])
        c.decode(3)
        rep0 = _row_report(c, 4)
        assert c.cancel([2]) == 0, c.lib.ctts_last_error().decode()
        c.decode(3)
        rep1 = _row_report(c, 4)
        live1 = c.opt("text_rows_live")
        c.compact([0, 1, 3])
        live2 = c.opt("text_rows_live")
        assert c.admit([1], [4], [4], [0]) == 0, c.lib.ctts_last_error().decode()
        live3 = c.opt("text_rows_live")
        c.decode(MAX_NEW + 2)
        assert c.progress()[1] == 1
        return c, rep0, rep1, (live1, live2, live3)

    # (a) a text row that ends by its limit while code rows are live reports {fin, end}; a cancelled text row keeps a prefix of the uncancelled run
    c, rep0, rep1, live = schedule([0, 1, 1, 0])
    assert rep0 == [[0, 4]] * 4, rep0
    assert rep1[1] == [1, 5] and rep1[2] == [1, 4] and rep1[0][0] == 0 and rep1[3][0] == 0, rep1
    # (b) a finished text row counts until it is compacted away or its row is handed on; then the batch is an ordinary code batch
    assert live == (2, 1, 0), live
    full = _alone_text(g, 2, "inv20", lim=TXT_NEW)
    ids, n, fin = c.text_out(2)
    assert n == 4 and fin == 0 and full.shape[0] > 4 and torch.equal(ids[:, 0], full[:4]), "the cancelled text row's tokens are no prefix of the uncancelled run"
    _assert_text_equals_alone(c, 1, _alone_text(g, 1, "inv20", lim=5), "the text row that ended by its limit")
    c.check_sentinels()
    # ... whose code rows equal those of the same schedule run without text rows (utterances 1 and 2 as code rows), and their batch-1 runs
    p, _, _, plive = schedule([0, 0, 0, 0])
    assert plive == (0, 0, 0)
    for u in (0, 3, 4):
        a, b = c.out(u), p.out(u)
        for k, name in enumerate(("ids", "hiddens", "logprobs", "sampled_logprobs")):
            assert torch.equal(a[k], b[k]), f"code utterance {u}: {name} differ from the schedule without text rows"
        assert a[4:] == b[4:]
        _assert_equals_alone(a, _alone(g, u, "inv20", lim=24 if u != 4 else None), f"code utterance {u}")
    # (c) a batch whose last live rows are all text rows still reaches all_done
    c = Mix(g, 3).begin([0, 1, 2], [0, 1, 1], [4, TXT_NEW, 9])
    c.decode(5)
    assert c.progress()[1] == 0 and _row_report(c, 3)[0] == [1, 4]
    c.decode(TXT_NEW)
    steps, alld = c.progress()
    assert alld == 1 and steps <= TXT_NEW + 1
    _assert_text_equals_alone(c, 1, _alone_text(g, 1, "inv20", lim=TXT_NEW), "text row 1")
    _assert_text_equals_alone(c, 2, _alone_text(g, 2, "inv20", lim=9), "text row 2")
    c.check_sentinels()


# ---- 5. DecodeSession -------------------------------------------------------------------------------------------------------------------------------------
def test_decode_session_serves_text_and_code_utterances():
    """6 code and 3 text utterances submitted in mixed order while others decode, one cancel of each kind: every delivered utterance equals its batch-1 run"""
    g = engine("fp32", INV, max_batch=20)
    lens, lims, ids, mask, uids = _pool()
    kinds = ["code", "text", "code", "code", "text", "code", "code", "text", "code"]
    emb = g(torch.from_numpy(ids[:9]), torch.ones(9, T_MAX, dtype=torch.bool))
    msk = torch.from_numpy(mask[:9])
    got = {}
    with g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, min_new_token=MIN_NEW, logits_warpers=LW, logits_processors=LP, return_hidden=True, return_logprobs=True,
                        seed=SEED, rows=6, out_slots=7, text_rows=dict(temperature=TXT_T, top_P=0.7, top_K=20, eos_token=TEXT_EOS, max_new_token=TXT_NEW,
                                                                      min_new_token=TXT_MIN)) as ses:
        with pytest.raises(_lib.HipBackendError, match="text utterance keeps the session's text_rows values"):
            ses.submit(emb[1], msk[1], uids[1], mode="text", sampling=dict(temperature=0.5))
        tk = [ses.submit(emb[u], msk[u], uids[u], limit=24, mode=kinds[u]) for u in range(3)]
        for _ in range(2):
            got.update({r.ticket: r for r in ses.step()})
            assert ses.book.lanes == _engine_lanes(g, len(ses.book.lanes))
        tk += [ses.submit(emb[u], msk[u], uids[u], limit=24, mode=kinds[u]) for u in range(3, 9)]
        assert ses.cancel(tk[0]) and ses.cancel(tk[1])                 # a seated code utterance and a seated text utterance
        while not ses.book.idle():
            for r in ses.step():
                assert r.ticket not in got
                got[r.ticket] = r
            assert ses.book.lanes == _engine_lanes(g, len(ses.book.lanes)), f"lane mirror {ses.book.lanes} after {ses.batch_trace}"
        trace = list(ses.batch_trace)
    assert not g.busy and sorted(got) == tk
    print(f"batch_trace {trace}")
    assert max(b for _, b in trace) > 3, "the batch never grew"
    for u in range(2, 9):
        r = got[tk[u]]
        assert not r.cancelled and r.utt_id == uids[u] and r.mode == kinds[u]
        if kinds[u] == "text":
            one = _alone_text(g, u, "inv20", lim=TXT_NEW)
            assert r.ids.dim() == 1 and r.hiddens is None and r.logprobs is None and torch.equal(r.ids.cpu(), one), f"text utterance {u} differs from its batch-1 run"
        else:
            one = _alone(g, u, "inv20", lim=24)
            _assert_equals_alone((r.ids.cpu(), r.hiddens.cpu(), r.logprobs.cpu(), r.sampled_logprobs.cpu(), int(r.ids.shape[0]), 0), one, f"code utterance {u}")
    r, one = got[tk[0]], _alone(g, 0, "inv20", lim=24)
    n = int(r.ids.shape[0])
    assert r.cancelled and 1 <= n < one[0].shape[0] and torch.equal(r.ids.cpu(), one[0][:n]) and torch.equal(r.hiddens.cpu(), one[1][:n])
    r, one = got[tk[1]], _alone_text(g, 1, "inv20", lim=TXT_NEW)
    n = int(r.ids.shape[0])
    assert r.cancelled and r.mode == "text" and 1 <= n < one.shape[0] and torch.equal(r.ids.cpu(), one[:n]), "the cancelled text utterance is no prefix of its run"


# ---- 6. the pipeline: refine inside the session ---------------------------------------------------------------------------------------------------------
def test_synth_session_refines_inside_the_session(tmp_path):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, InferDetails, RefineTextParams
    from tests.test_gpu_score import CFG4, LLAMA4
    g = GPT(LLAMA4, max_batch=8, max_seq_len=200, weight_dtype="fp32", options=dict(INV))
    sd = synth.gpt_state_dict(CFG4, 1234)
    # The toy tokenizer keeps ids < [break_0] = 10 of a refined row, and a random 21178-way head all but never samples one: every refined text would be '' and
    # the comparison below empty.  The gains (weight-norm g) of the head's first 10 rows are raised 30-fold, so the text rows sample mostly those ids
    sd["head_text.parametrizations.weight.original0"] = sd["head_text.parametrizations.weight.original0"].copy()
    sd["head_text.parametrizations.weight.original0"][:10] *= 30.0
    g.load_state_dict(sd)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    tok = synth.toy_tokenizer(str(tmp_path / "tok"))
    texts = synth.toy_texts(6, 8, 30, seed=68)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=24, min_new_token=4, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())
    refine = RefineTextParams(prompt="[oral_2]", max_new_token=16, min_new_token=2, show_tqdm=False)
    seed = 4243
    try:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, tok, torch.device("cuda:0"))
        kw = dict(params_refine_text=refine, params_infer_code=params, noise="device", noise_seed=seed, slice_size=4, continuous=True, utt_ids=list(range(6)))
        ref_text = list(pipe.infer(list(texts), skip_refine_text=False, refine_text_only=True, **kw))
        assert len(ref_text) == 1 and len(ref_text[0]) == 6, "infer splits or merges these texts: not one utterance per text"
        ref = list(pipe.infer(list(texts), skip_refine_text=False, return_details=True, **kw))
        assert len(ref) == 1 and isinstance(ref[0], InferDetails) and len(ref[0].ids) == 6
        ref = ref[0]
        got = {}
        with pipe.open_session(params, seed=seed, return_details=True, refine=refine) as ses:
            tk = [ses.submit(texts[u], utt_id=u) for u in range(3)]
            for _ in range(2):
                got.update({t: (d, c) for t, d, c in ses.poll()})
            tk += [ses.submit(texts[u], utt_id=u) for u in range(3, 6)]
            got.update({t: (d, c) for t, d, c in ses.drain()})
            extra = ses.submit(texts[0], utt_id=77)
            assert ses.cancel(extra)                                   # still in its refine stage
            out = ses.drain()
            assert [(t, int(d.wav.shape[0]), c) for t, d, c in out] == [(extra, 0, True)]
        assert not g.busy and sorted(got) == tk
        for u in range(6):
            d, cancelled = got[tk[u]]
            assert not cancelled
            assert d.refined_text == ref_text[0][u], f"utterance {u}: refined text {d.refined_text!r}, infer gives {ref_text[0][u]!r}"
            assert torch.equal(d.ids.cpu(), ref.ids[u].cpu()), f"utterance {u}: code ids differ from infer(skip_refine_text=False, continuous=True)"
            a, b = ref.wavs[u].cpu().numpy(), d.wav.cpu().numpy()
            assert a.shape == b.shape
            rel = float(np.sqrt(np.mean((a - b) ** 2))) / float(np.sqrt(np.mean(a ** 2)))
            print(f"utterance {u}: refined {d.refined_text!r}, wav rms difference {rel:.3e} relative (bound 1e-4)")
            assert rel <= 1e-4
        refined = [got[tk[u]][0].refined_text for u in range(6)]
        assert len(set(refined)) > 1 and all(refined), f"the refined texts {refined} put nothing to the test"
        with pytest.raises(_lib.HipBackendError, match="refine-text"):
            pipe.open_session(params, refine_text_only=True)
        with pytest.raises(_lib.HipBackendError, match="must be 1..max_new_token=24"):
            pipe.open_session(params, refine=RefineTextParams(max_new_token=25))
        assert not g.busy
    finally:
        g.close()


# ---- 4 / 7. the off path and the refusals, on the reference-minted golden ---------------------------------------------------------------------------------------
def test_off_path_and_refusals_on_the_golden():
    """A state that never enables text rows: the first slice of the reference-minted fixture (tests/golden gpt_real_device_noise: 20 layers), bit for bit, with
    "text_rows_live" 0.  Then every refusal of the three calls and of open_session / submit, each followed by the same plain generate()."""
    from chatttsplus_amd.hip_models import GPT
    from tests.test_gpu_gpt import LLAMA
    from tests.test_gpu_score import CFG4, LLAMA4
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

    def live():
        v = C.c_int(-1)
        _lib.check(lib.ctts_gpt_get_option(h, b"text_rows_live", C.byref(v)), "get_option")
        return int(v.value)

    def plain(after):
        out = list(g.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, attention_mask=mask_t, max_new_token=N, min_new_token=int(meta["min_new"]), logits_warpers=LW,
                              logits_processors=LP, return_hidden=True, noise="device", seed=seed, utt_ids=uids[:4]))[-1]
        assert live() == 0
        for b in range(4):
            n = int(z["lens"][b])
            assert out.ids[b].shape[0] == n and np.array_equal(out.ids[b].cpu().numpy(), z["ids"][b, :n].astype(np.int64)), f"after {after}: utterance {b}"

    def refused(rc, text, after):
        assert rc != 0 and text in lib.ctts_last_error().decode(), f"{after}: rc {rc}, message {lib.ctts_last_error().decode()!r}"
        torch.cuda.synchronize()
        plain(after)

    try:
        plain("nothing: the off path")
        out = dict(ids=torch.empty(4, 8, 4, dtype=torch.int32, device=dev), fin=torch.zeros(4, dtype=torch.int32, device=dev), end=torch.zeros(4, dtype=torch.int32, device=dev),
                   tids=torch.empty(4, 8, 4, dtype=torch.int32, device=dev))
        sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, 8, 2, LW, LP, 4)
        sc_text = sampler_cfg_from_objects(torch.tensor([0.7]), TEXT_EOS, 8, 1, LW, [], 4, infer_text=True)
        msk = mask_t.to(dev).to(torch.int32).contiguous()
        keep = []

        def arr(v, dt=np.int32):
            a = np.ascontiguousarray(v, dtype=dt)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)

        def begin(modes=None, noise=None, cfg=None, knobs=None, share=None, prefill=True):
            io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(),
                            noise=noise.data_ptr() if noise is not None else None, n_draws=2 if noise is not None else 0, seed=3)
            if modes is not None:
                _lib.check(lib.ctts_gpt_set_row_modes(h, arr(modes), 2), "set_row_modes")
            if knobs is not None:
                _lib.check(lib.ctts_gpt_set_row_sampling(h, knobs, 2), "set_row_sampling")
            if share is not None:
                _lib.check(lib.ctts_gpt_share_prompts(h, 2, arr(share), 1), "share_prompts")
            try:
                rc = lib.ctts_gpt_begin(h, 2, T, msk.data_ptr(), C.byref(cfg or sc), C.byref(io), st)
            finally:
                lib.ctts_gpt_set_row_modes(h, None, 0)
                lib.ctts_gpt_set_row_sampling(h, None, 0)
            if rc == 0 and prefill:
                _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
            return rc

        def enable(cfg=None):
            return lib.ctts_gpt_enable_text_rows(h, C.byref(cfg or sc_text), out["tids"].data_ptr(), st)

        # a mode-1 row without enable_text_rows: seated by begin (sample and decode refuse), named for an admission
        assert begin([1, 0]) == 0 and live() == 1
        assert lib.ctts_gpt_decode(h, 1, 0, st) != 0 and "ctts_gpt_enable_text_rows has not been called" in lib.ctts_last_error().decode()
        refused(lib.ctts_gpt_sample(h, st), "ctts_gpt_enable_text_rows has not been called", "sample with a text row and no text block")
        assert begin() == 0 and lib.ctts_gpt_sample(h, st) == 0
        refused(lib.ctts_gpt_admit_modes(h, 1, arr([0]), arr([1]), st), "needs ctts_gpt_enable_text_rows first", "admit_modes(1) without enable_text_rows")
        assert begin() == 0
        refused(lib.ctts_gpt_admit_modes(h, 1, arr([0]), arr([2]), st), "mode 2 (0 = code, 1 = text)", "admit_modes with mode 2")
        refused(lib.ctts_gpt_set_row_modes(h, arr([0, 3]), 2), "mode 3 (0 = code, 1 = text)", "set_row_modes with mode 3")
        # use_penalty in text_sc; a text_sc that is not the refine pass's; text max_new_token beyond the code call's
        pen = sampler_cfg_from_objects(torch.tensor([0.7]), TEXT_EOS, 8, 1, LW, [], 4, infer_text=True)
        pen.use_penalty = 1
        assert begin() == 0
        refused(enable(pen), "use_penalty must be 0", "enable_text_rows with a repetition penalty")
        assert begin() == 0
        refused(enable(sc), "infer_text = 1", "enable_text_rows with code parameters")
        assert begin() == 0
        refused(enable(sampler_cfg_from_objects(torch.tensor([0.7]), TEXT_EOS, 9, 1, LW, [], 4, infer_text=True)), "must be 1..8, the code call's max_new_token",
                "text max_new_token 9 > 8")
        # caller-supplied noise
        noise = torch.empty(2, 8, 626, device=dev).exponential_()
        assert begin(noise=noise) == 0
        refused(enable(), "enable_text_rows: device noise only", "enable_text_rows with caller-supplied noise")
        refused(begin([0, 1], noise=noise), "need device noise", "begin seating a text row with caller-supplied noise")
        # a call whose own infer_text is 1
        assert begin(cfg=sc_text) == 0
        refused(enable(), "own infer_text is 1", "enable_text_rows in a text-mode call")
        refused(begin([1, 0], cfg=sc_text), "own infer_text is 1", "set_row_modes before a text-mode begin")
        # shared prompt passes with a text row
        refused(begin([0, 1], share=[0, 0]), "shared prompt passes (ctts_gpt_share_prompts) are for code rows", "share_prompts + a text row at begin")
        assert begin() == 0 and enable() == 0 and lib.ctts_gpt_sample(h, st) == 0
        _lib.check(lib.ctts_gpt_decode(h, 8, 0, st), "decode")
        _lib.check(lib.ctts_gpt_share_prompts(h, 2, arr([0, 0]), 1), "share_prompts")
        _lib.check(lib.ctts_gpt_admit_modes(h, 2, arr([0, 1]), arr([0, 1]), st), "admit_modes")
        refused(lib.ctts_gpt_admit(h, 2, arr([0, 1]), T, msk.data_ptr(), emb.data_ptr(), arr([7, 8], np.uint64), None, arr([2, 3]), None, st),
                "shared prompt passes (ctts_gpt_share_prompts) are for code rows", "share_prompts + a text row at admit")
        # restart while text rows are enabled
        assert begin() == 0 and enable() == 0 and lib.ctts_gpt_sample(h, st) == 0
        refused(lib.ctts_gpt_restart(h, st), "restart: text rows are enabled", "restart with text rows enabled")
        # per-row sampling knobs on a text row: at begin (an entry that differs from the call's values) and at admit
        from chatttsplus_amd.hip_models.gpt import row_sampling_from_values
        base, hot = row_sampling_from_values(sc, None, 4), row_sampling_from_values(sc, dict(temperature=0.9), 4)
        refused(begin([0, 1], knobs=(_lib.RowSampling * 2)(base, hot)), "carries per-row sampling knobs", "set_row_sampling on a text row")
        assert begin([0, 1], knobs=(_lib.RowSampling * 2)(hot, base)) == 0 and enable() == 0 and lib.ctts_gpt_sample(h, st) == 0      # (knobs on the code row: fine)
        _lib.check(lib.ctts_gpt_decode(h, 8, 0, st), "decode")
        _lib.check(lib.ctts_gpt_admit_sampling(h, 1, arr([1]), (_lib.RowSampling * 1)(hot), st), "admit_sampling")
        _lib.check(lib.ctts_gpt_admit_modes(h, 1, arr([1]), arr([1]), st), "admit_modes")
        refused(lib.ctts_gpt_admit(h, 1, arr([1]), T, msk.data_ptr(), emb.data_ptr(), arr([9], np.uint64), None, arr([2]), None, st), "carries per-row sampling knobs",
                "admit_sampling on a text row")
        # log-probs stay code-only but are not refused beside text rows; every begin switches the feature off again
        assert begin([0, 1]) == 0 and enable() == 0 and live() == 1
        assert begin() == 0 and live() == 0
        refused(lib.ctts_gpt_admit_modes(h, 1, arr([0]), arr([1]), st), "needs ctts_gpt_enable_text_rows first", "admit_modes after the next begin")
        # an engine without head_text
        g4 = GPT(LLAMA4, max_batch=4, max_seq_len=64, weight_dtype="fp32")
        try:
            g4.load_state_dict({k: v for k, v in synth.gpt_state_dict(CFG4, 1234).items() if not k.startswith("head_text")})
            e4 = torch.zeros(2, T, 768, device=dev)
            io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=3)
            _lib.check(lib.ctts_gpt_begin(g4._h, 2, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
            _lib.check(lib.ctts_gpt_prefill(g4._h, e4.data_ptr(), st), "prefill")
            refused(lib.ctts_gpt_enable_text_rows(g4._h, C.byref(sc_text), out["tids"].data_ptr(), st), "need head_text.* and emb_text.weight", "an engine without head_text")
            _lib.check(lib.ctts_gpt_set_row_modes(g4._h, arr([1, 0]), 2), "set_row_modes")
            rc = lib.ctts_gpt_begin(g4._h, 2, T, msk.data_ptr(), C.byref(sc), C.byref(io), st)
            lib.ctts_gpt_set_row_modes(g4._h, None, 0)
            refused(rc, "needs head_text.* and emb_text.weight", "a text row at begin on an engine without head_text")
        finally:
            g4.close()
        # the host objects
        with pytest.raises(_lib.HipBackendError, match="refine-text pass"):
            g.open_session(torch.tensor([0.3] * 4), 625, N, infer_text=True)
        with pytest.raises(_lib.HipBackendError, match=r"must be 1..max_new_token"):
            g.open_session(torch.tensor([0.3] * 4), 625, 8, text_rows=dict(eos_token=TEXT_EOS, max_new_token=9))
        with pytest.raises(_lib.HipBackendError, match="unknown key"):
            g.open_session(torch.tensor([0.3] * 4), 625, 8, text_rows=dict(eos_token=TEXT_EOS, max_new_token=8, repetition_penalty=1.2))
        assert not g.busy
        with g.open_session(torch.tensor([0.3] * 4), 625, 8, seed=1) as ses:
            with pytest.raises(_lib.HipBackendError, match='mode="text" needs a session opened with text_rows'):
                ses.submit(emb[0], mask_t[0], 1, mode="text")
        plain("the refused open_session / submit calls")
    finally:
        g.close()
