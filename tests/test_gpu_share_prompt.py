"""Shared prompt passes (ctts_gpt_share_prompts, kv_share.hip; GPT.generate / generate_many(prompt_of=...); infer(num_candidates=N, share_prompt=...)):
sequences that name one prompt run it through the prompt pass once, the others receive a copy of the leader's KV lane and pending decode input.
Synthetic weights at real widths, 4 decoder layers, as tests/test_gpu_score.py builds them.

Checked here: the followers' lanes equal their leaders' byte for byte and nothing else is written; the leaders' lanes are those of a plain call; under
batch_invariant a shared call equals the unshared one bit for bit (generate, generate_many with admissions, ensure_non_empty restarts, the pipeline); in
default mode (token flips between schedules are possible) every row's own log-probs agree with GPT.score of its ids within the project's bounds (2e-4 on
fp32, FP16_TOL on fp16: tests/test_gpu_gen_logprobs.py, tests/test_gpu_score.py); refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs
from tests import helpers
from tests.test_gpu_gen_logprobs import HOT, SEED5, _restart_uid
from tests.test_gpu_score import CFG4, EOS, FP16_TOL, LLAMA4, engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
INV = dict(batch_invariant=1)
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
POF = [1, 0, 1, 2, 0, 1]          # three prompts, non-adjacent and unsorted groups: sequences 0, 1 and 3 lead, 2, 4 and 5 follow


def _leaders(pof):
    first = {}
    for i, p in enumerate(pof):
        first.setdefault(p, i)
    return first


# ---- 1. lanes, bit for bit ---------------------------------------------------------------------------------------------------------------------
def _begin_prefill(g, ids, mask, prompt_of=None, max_new=8):
    """begin + prefill through the ABI (nothing is sampled); returns the KV cache as bytes [layer][k | v][lane][head][slot][64 elements] and x_dec [rows][768]"""
    lib, h, dev = g._lib, g._h, g.device
    P, T = mask.shape
    B = len(prompt_of) if prompt_of is not None else P
    emb = g(torch.from_numpy(ids), torch.ones(P, T, dtype=torch.bool)).contiguous()
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, max_new, 2, LW, LP, 4)
    out = dict(ids=torch.empty(B, max_new, 4, dtype=torch.int32, device=dev), fin=torch.zeros(B, dtype=torch.int32, device=dev),
               end=torch.zeros(B, dtype=torch.int32, device=dev))
    io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=3)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    msk = torch.from_numpy(mask).to(dev).to(torch.int32).contiguous()
    g._kv.fill_(SENTINEL)
    if prompt_of is not None:
        arr = np.ascontiguousarray(prompt_of, dtype=np.int32)
        _lib.check(lib.ctts_gpt_share_prompts(h, B, arr.ctypes.data_as(C.c_void_p), P), "share_prompts")
    _lib.check(lib.ctts_gpt_begin(h, B, T, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    x = np.zeros((_lib.MAX_BATCH, 768), dtype=np.float32)
    nb = C.c_size_t(0)
    _lib.check(lib.ctts_gpt_debug_read(h, b"x_dec", x.ctypes.data_as(C.c_void_p), x.nbytes, C.byref(nb), st), "debug_read")      # (synchronises)
    esz = 2 if g.dtype_code == _lib.DTYPE_F16 else 4
    n = 4 * 2 * g.max_batch * 12 * g.max_seq * 64 * esz
    kv = g._kv[:n].cpu().numpy().reshape(4, 2, g.max_batch, 12, g.max_seq, 64 * esz)
    return kv, x[:B].copy().view(np.uint8)


LANE_CASES = [("fp32", None, None, "3x37"), ("fp16", None, None, "3x37"), ("fp32", INV, None, "3x37"),
              ("fp32", None, None, "2x19"), ("fp16", None, None, "2x19"), ("fp32", INV, None, "2x19"),      # 38 prompt rows: below the 65-row split-GEMM threshold
              ("fp32", None, 64, "3x37")]                                                                   # 111 rows in passes of 64: prompts straddle the pass boundary


@pytest.mark.parametrize("dtype,options,pass_rows,shape", LANE_CASES)
def test_follower_lanes_equal_their_leaders(dtype, options, pass_rows, shape):
    g = engine(dtype, options=options, pass_rows=pass_rows)
    assert g.max_batch == 8
    if shape == "3x37":       # left pads 0 / 5 / 36: the last is a one-token prompt (under batch_invariant its prompt pass holds pad rows only)
        T, pads, pof = 37, [0, 5, 36], POF
    else:
        T, pads, pof = 19, [0, 7], [1, 0, 0, 1, 1]
    ids, mask = synth.prompt_ids(len(pads), T, CFG4["num_text_tokens"], 905, pad_left=pads)
    span = T - 1 if options else T         # batch_invariant: the last token runs through the first decode step
    kv, x = _begin_prefill(g, ids, mask, pof)
    lead = _leaders(pof)
    B = len(pof)
    assert kv[:, :, :B, :, :span].min() != SENTINEL or kv[:, :, :B, :, :span].max() != SENTINEL, "the prompt pass wrote nothing"
    for i, p in enumerate(pof):
        assert np.array_equal(kv[:, :, i, :, :span], kv[:, :, lead[p], :, :span]), f"lane {i} differs from its leader's lane {lead[p]} over the prompt span"
        assert np.array_equal(x[i], x[lead[p]]), f"decode input of row {i} differs from its leader's"
    # nothing else is written: slots at or beyond the prompt end of every lane, and the lanes the call does not name
    assert bool((kv[:, :, :, :, span:] == SENTINEL).all()), "a slot at or beyond the prompt end was written"
    assert bool((kv[:, :, B:] == SENTINEL).all()), "a lane outside the call was written"
    # the leaders' lanes and rows are those of a plain call of the same prompts
    kv0, x0 = _begin_prefill(g, ids, mask)
    for p, i in lead.items():
        assert np.array_equal(kv[:, :, i, :, :span], kv0[:, :, p, :, :span]), f"leader lane {i} differs from the plain call's lane {p}"
        assert np.array_equal(x[i], x0[p])
    assert bool((kv0[:, :, len(pads):] == SENTINEL).all())


# ---- 2. exact under batch_invariant ----------------------------------------------------------------------------------------------------------
def _gen_kw(**kw):
    base = dict(max_new_token=24, min_new_token=2, logits_warpers=LW, logits_processors=LP, return_hidden=True, return_logprobs=True)
    base.update(kw)
    return base


def _assert_same_outputs(a, b, what):
    assert len(a.ids) == len(b.ids)
    for r in range(len(a.ids)):
        assert a.ids[r].shape == b.ids[r].shape, f"{what} row {r}: end_idx differs ({a.ids[r].shape[0]} vs {b.ids[r].shape[0]})"
        for name in ("ids", "hiddens", "logprobs", "sampled_logprobs"):
            assert torch.equal(getattr(a, name)[r].cpu(), getattr(b, name)[r].cpu()), f"{what} row {r}: {name} differ"
        fa, fb = a.final_logprobs[r], b.final_logprobs[r]
        assert (fa is None) == (fb is None) and (fa is None or torch.equal(fa.cpu(), fb.cpu())), f"{what} row {r}: final_logprobs differ"


PER_ROW = [None, dict(temperature=0.7), dict(top_K=5, repetition_penalty=1.2), None, dict(temperature=1.0, top_P=0.9), dict(min_new_token=6)]
LIMITS = [24, 9, 17, 24, 5, 13]


def test_generate_shared_equals_unshared_bit_for_bit():
    g = engine(options=INV)
    ids, mask = synth.prompt_ids(3, 14, CFG4["num_text_tokens"], 906, pad_left=[0, 3, 13])
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    sel = torch.tensor(POF)
    kw = _gen_kw(attention_mask=None, noise="device", seed=41, utt_ids=[100 + i for i in range(6)], max_new_tokens_per_row=LIMITS, sampling_per_row=PER_ROW)
    shared = list(g.generate(g(ids_t, torch.ones(3, 14, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS, prompt_of=POF,
                             **dict(kw, attention_mask=mask_t)))[-1]
    assert g.shared_prompts == [(6, 3)]
    plain = list(g.generate(g(ids_t[sel], torch.ones(6, 14, dtype=torch.bool)), ids_t[sel], torch.tensor([0.3] * 4), EOS, **dict(kw, attention_mask=mask_t[sel])))[-1]
    assert g.shared_prompts == []
    assert len(shared.ids) == 6 and any(i.shape[0] > 2 for i in shared.ids)
    _assert_same_outputs(shared, plain, "generate")
    # knobs and limits differ inside a group: so do the tokens
    assert not torch.equal(shared.ids[0][:5].cpu(), shared.ids[2][:5].cpu())


# ---- 3. generate_many ----------------------------------------------------------------------------------------------------------------------------
def test_generate_many_groups_what_it_seats():
    g = engine(options=INV)
    ids, mask = synth.prompt_ids(3, 14, CFG4["num_text_tokens"], 907, pad_left=[0, 4, 8])
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    pof = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    sel = torch.tensor(pof)
    lims = [6, 20, 11, 24, 5, 16, 9, 24, 7]
    per = [None, dict(temperature=0.7), None, None, dict(top_K=5), None, dict(temperature=1.0, top_P=0.9), None, None]
    kw = _gen_kw(seed=43, utt_ids=[200 + i for i in range(9)], max_new_tokens_per_row=lims, sampling_per_row=per, rows=4)
    shared = g.generate_many(g(ids_t, torch.ones(3, 14, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS, attention_mask=mask_t, prompt_of=pof, **kw)
    calls, admissions = list(g.shared_prompts), list(g.admissions)
    print(f"generate_many: (rows, prompts) per begin / admit {calls}; admissions {admissions}")
    assert calls[0] == (4, 2), "begin seats candidates 0..2 of prompt 0 and candidate 0 of prompt 1"
    assert any(r > p for r, p in calls) and sum(r for r, _ in calls) >= 9
    assert len(admissions) >= 1 and len(calls) == 1 + len(admissions)
    plain = g.generate_many(g(ids_t[sel], torch.ones(9, 14, dtype=torch.bool)), ids_t[sel], torch.tensor([0.3] * 4), EOS, attention_mask=mask_t[sel], **kw)
    assert g.shared_prompts == []
    _assert_same_outputs(shared, plain, "generate_many")


# ---- 4. default mode: every row's log-probs against a re-scoring of its own ids --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_default_mode_rows_agree_with_score(dtype):
    g = engine(dtype)
    ids, mask = synth.prompt_ids(3, 14, CFG4["num_text_tokens"], 908, pad_left=[0, 3, 6])
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    sel = torch.tensor(POF)
    out = list(g.generate(g(ids_t, torch.ones(3, 14, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS, prompt_of=POF,
                          **_gen_kw(attention_mask=mask_t, max_new_token=20, min_new_token=4, noise="device", seed=47, utt_ids=[300 + i for i in range(6)],
                                    max_new_tokens_per_row=[20, 12, 20, 7, 20, 16])))[-1]
    assert g.shared_prompts == [(6, 3)]
    codes = [i.cpu() for i in out.ids]
    assert all(c.shape[0] >= 4 for c in codes)
    si = score_inputs(ids_t[sel], mask_t[sel], torch.ones(6, 14, dtype=torch.bool), codes, EOS, append_eos=False)
    res = g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
    tol = 2e-4 if dtype == "fp32" else FP16_TOL
    for b in range(6):
        d = float((out.logprobs[b].cpu() - res.logprob[b]).abs().max())
        print(f"{dtype} row {b} (prompt {POF[b]}, {'leader' if _leaders(POF)[POF[b]] == b else 'follower'}): |logprobs - GPT.score| {d:.3e} (bound {tol:.1e})")
        assert d <= tol


# ---- 5. ensure_non_empty with shared rows ------------------------------------------------------------------------------------------------------------
class _CountRestarts:
    """the library handle of one engine with ctts_gpt_restart counted"""

    def __init__(self, lib):
        self._lib, self.restarts = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ctts_gpt_restart":
            return fn

        def counted(*a):
            self.restarts += 1
            return fn(*a)
        return counted


def test_ensure_non_empty_restart_with_shared_rows():
    """EOS-boosted heads (helpers.gen_case_inputs).  Row 4 -- a follower -- draws near-uniformly (HOT) under an utterance id whose step-0 draw is EOS at
    attempt 0 and not at attempt 1 (tests/test_gpu_gen_logprobs.py _restart_uid); the other rows cannot end before their second token.  The whole batch restarts
    once (ctts_gpt_restart replays the last prompt token's layer pass from x_last / rope_dec0, filled for followers too) and finishes; equal to the unshared call."""
    from chatttsplus_amd.hip_models import GPT
    meta = dict(weight_seed=4321, eos_boost=2.2, B=3, T=12, pad_left=[0, 3, 5], prompt_seed=909)
    sd, ids, mask, _ = helpers.gen_case_inputs(meta, CFG4)
    g = GPT(LLAMA4, max_batch=8, max_seq_len=256, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(sd)
    lib = g._lib
    try:
        ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
        sel = torch.tensor(POF)
        uids = [400 + i for i in range(6)]
        uids[4] = _restart_uid()
        per = [dict(min_new_token=2) for _ in range(6)]
        per[4] = dict(HOT)
        kw = _gen_kw(min_new_token=0, noise="device", seed=SEED5, utt_ids=uids, sampling_per_row=per, ensure_non_empty=True)
        runs = []
        for pof in (POF, None):
            counter = g._lib = _CountRestarts(lib)
            i_t, m_t = (ids_t, mask_t) if pof is not None else (ids_t[sel], mask_t[sel])
            outs = list(g.generate(g(i_t, torch.ones(i_t.shape[0], 12, dtype=torch.bool)), i_t, torch.tensor([0.3] * 4), EOS, prompt_of=pof,
                                   **dict(kw, attention_mask=m_t)))
            assert outs, "ensure_non_empty gave up"
            assert counter.restarts == 1, f"{counter.restarts} restarts"
            runs.append(outs[-1])
        assert all(i.shape[0] >= 1 for i in runs[0].ids)
        _assert_same_outputs(runs[0], runs[1], "restart")
    finally:
        g._lib = lib
        g.close()


# ---- 6. pipeline -----------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_candidates_share_their_prompt(tmp_path):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, InferDetails
    sd = synth.gpt_state_dict(CFG4, 1234)
    g = GPT(LLAMA4, max_batch=8, max_seq_len=160, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(sd)
    g2 = GPT(LLAMA4, max_batch=8, max_seq_len=160, weight_dtype="fp32")
    g2.load_state_dict(sd)
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 32 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    tok = synth.toy_tokenizer(str(tmp_path / "tok"))
    texts = synth.toy_texts(2, 8, 30, seed=67)
    params = InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=24, min_new_token=4, show_tqdm=False,
                             spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float())

    def run(pipe, **kw):
        out = list(pipe.infer(list(texts), skip_refine_text=True, params_infer_code=params, noise="device", noise_seed=4242, slice_size=8, num_candidates=4,
                              return_details=True, **kw))
        assert len(out) == 1 and isinstance(out[0], InferDetails)
        return out[0]

    try:
        pipe = ChatTTSPlusPipeline.from_components(g, syn, tok, torch.device("cuda:0"))
        d = run(pipe)                                   # share_prompt=None on an invariant engine: shared
        assert g.shared_prompts == [(8, 2)]
        d0 = run(pipe, share_prompt=False)
        assert g.shared_prompts == []
        assert d.candidate == d0.candidate
        for u in range(2):
            assert len(d.candidates[u]) == 4
            for k in range(4):
                assert torch.equal(d.candidates[u][k].ids.cpu(), d0.candidates[u][k].ids.cpu()), f"utterance {u} candidate {k}: ids differ from the unshared run"
                assert torch.equal(d.candidates[u][k].logprobs, d0.candidates[u][k].logprobs)
            assert torch.equal(d.ids[u].cpu(), d0.ids[u].cpu())
            assert torch.equal(d.wavs[u].cpu(), d0.wavs[u].cpu())
        # a default-mode engine shares only when asked to
        pipe2 = ChatTTSPlusPipeline.from_components(g2, syn, tok, torch.device("cuda:0"))
        run(pipe2)
        assert g2.shared_prompts == []
        d2 = run(pipe2, share_prompt=True)
        assert g2.shared_prompts == [(8, 2)]
        assert all(len(d2.candidates[u]) == 4 and all(c.ids.shape[0] >= 4 for c in d2.candidates[u]) for u in range(2))
        assert all(d2.wavs[u].shape[0] == 256 * (2 * d2.ids[u].shape[0] - 1) for u in range(2))
    finally:
        g.close()
        g2.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_next_plain_call():
    g = engine()
    lib, h = g._lib, g._h
    ids, mask = synth.prompt_ids(3, 10, CFG4["num_text_tokens"], 910, pad_left=[0, 2, 4])
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)

    def plain():
        return list(g.generate(g(ids_t, torch.ones(3, 10, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS,
                               **_gen_kw(attention_mask=mask_t, max_new_token=12, noise="device", seed=53)))[-1]

    def shared(**kw):
        return list(g.generate(g(ids_t, torch.ones(3, 10, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS, prompt_of=POF,
                               **_gen_kw(attention_mask=mask_t, max_new_token=12, noise="device", seed=53, **kw)))

    before = plain()
    # sequences of one group with different adapter slots (0 and 2 share prompt 1)
    g.set_row_adapters([0, -1, 1, -1, -1, 0])
    try:
        with pytest.raises(_lib.HipBackendError, match=r"begin: sequences 0 and 2 share prompt 1 .*different adapter slots \(0, 1\)"):
            shared()
    finally:
        g.set_row_adapters(None)
    _assert_same_outputs(plain(), before, "after the adapter refusal")
    # infer_text: refused by the host before anything is enqueued, and by the engine
    with pytest.raises(_lib.HipBackendError, match="code mode only"):
        list(g.generate(g(ids_t, torch.ones(3, 10, dtype=torch.bool)), ids_t, torch.tensor([0.3] * 4), EOS, prompt_of=POF, infer_text=True, attention_mask=mask_t,
                        max_new_token=12, noise="device", seed=53))
    dev = g.device
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = dict(ids=torch.empty(6, 12, 4, dtype=torch.int32, device=dev), fin=torch.zeros(6, dtype=torch.int32, device=dev), end=torch.zeros(6, dtype=torch.int32, device=dev))
    io = _lib.GenIO(ids=out["ids"].data_ptr(), hiddens=None, finish=out["fin"].data_ptr(), end_idx=out["end"].data_ptr(), noise=None, n_draws=0, seed=3)
    msk = mask_t.to(dev).to(torch.int32).contiguous()
    arr = np.ascontiguousarray(POF, dtype=np.int32)
    sc_text = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, 12, 2, [], [], 4, infer_text=True)
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, 12, 2, LW, LP, 4)
    _lib.check(lib.ctts_gpt_share_prompts(h, 6, arr.ctypes.data_as(C.c_void_p), 3), "share_prompts")
    assert lib.ctts_gpt_begin(h, 6, 10, msk.data_ptr(), C.byref(sc_text), C.byref(io), st) != 0
    assert "code mode only" in lib.ctts_last_error().decode()
    # n differs from the call's
    _lib.check(lib.ctts_gpt_share_prompts(h, 6, arr.ctypes.data_as(C.c_void_p), 3), "share_prompts")
    assert lib.ctts_gpt_begin(h, 3, 10, msk.data_ptr(), C.byref(sc), C.byref(io), st) != 0
    assert "named the prompts of 6 sequences, this call has B=3" in lib.ctts_last_error().decode()
    # the request was consumed by the refused call: the same begin now goes through as a plain one
    _lib.check(lib.ctts_gpt_begin(h, 3, 10, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    # refused at once: an index out of range, a prompt named by no sequence
    bad = np.ascontiguousarray([0, 3, 1], dtype=np.int32)
    assert lib.ctts_gpt_share_prompts(h, 3, bad.ctypes.data_as(C.c_void_p), 3) != 0 and "outside 0..2" in lib.ctts_last_error().decode()
    bad = np.ascontiguousarray([0, 2, 2], dtype=np.int32)
    assert lib.ctts_gpt_share_prompts(h, 3, bad.ctypes.data_as(C.c_void_p), 3) != 0 and "prompt 1 is named by no sequence" in lib.ctts_last_error().decode()
    torch.cuda.synchronize()
    _assert_same_outputs(plain(), before, "after the refused calls")
    # ... and a shared call still works
    assert len(shared()[-1].ids) == 6
