"""The batch-invariance contract on fp16 engines (option "schedule_invariant", include/ctts_hip.h).

With the option on and device noise, an fp16 engine's hidden rows, token ids and log-probs of an utterance are a function of its own inputs only: served
alone, in slices of 2 .. 60 next to other prompts (other left padding; prompt passes of under 64, of 64 .. 1535 and of 1536 and more rows), through
finished-row compaction, begun or admitted, in arrival or longest-first order, across pass boundaries, in a growing session, behind a shared prompt pass --
bit for bit (torch.equal on ids AND hidden rows), not merely token for token.  Real widths (synth.GPT_REAL, 20 layers, synthetic weights): the kernels are
specialised to them.  One engine for the module; the yardstick is every utterance alone at batch 1, computed once."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from chatttsplus_amd import synth

pytestmark = pytest.mark.gpu

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
INV = {"schedule_invariant": 1}
INT_MAX = 0x7FFFFFFF

N_UTT, T_MAX, NEW_MAX, SEED = 60, 80, 16, 271828
MAX_BATCH, MAX_SEQ = 64, 128
_engines, _ref, _sd = {}, {}, []


def state_dict():
    if not _sd:
        _sd.append(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    return _sd[0]


def engine(dtype="fp16", options=INV, pass_rows=None, max_batch=MAX_BATCH):
    from chatttsplus_amd.hip_models import GPT
    key = (dtype, tuple(sorted(options.items())), pass_rows, max_batch)
    if key not in _engines:
        if pass_rows:
            os.environ["CTTS_PASS_ROWS"] = str(pass_rows)      # read once at finalize (as tests/test_gpu_score.py sets it)
        try:
            g = GPT(LLAMA, max_batch=max_batch, max_seq_len=MAX_SEQ, weight_dtype=dtype, options=dict(options))
            g.load_state_dict(state_dict())
        finally:
            os.environ.pop("CTTS_PASS_ROWS", None)
        _engines[key] = g
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    for g in _engines.values():
        g.close()
    _engines.clear()
    _ref.clear()


def _request():
    """N_UTT utterances: prompts U{8..80} tokens, limits U{6..16}; left-padded to T_MAX"""
    if "req" not in _ref:
        rng = np.random.Generator(np.random.Philox(key=1618))
        lens = [int(x) for x in rng.integers(8, T_MAX + 1, size=N_UTT)]
        lims = [int(x) for x in rng.integers(6, NEW_MAX + 1, size=N_UTT)]
        ids, mask = synth.prompt_ids(N_UTT, T_MAX, synth.GPT_REAL["num_text_tokens"], seed=77, pad_left=[T_MAX - n for n in lens])
        _ref["req"] = (lens, lims, ids, mask)
    return _ref["req"]


def _emb(g):
    lens, lims, ids, mask = _request()
    return lens, lims, ids, mask, g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))


def _generate(g, us, emb, ids, mask, lens, lims, trim=True, **kw):
    """the utterances `us` as ONE generate() call (left padding: to the longest of them, or the full T_MAX)"""
    T = max(lens[u] for u in us) if trim else T_MAX
    ii = torch.as_tensor(us, dtype=torch.long)
    out = list(g.generate(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(ids[us][:, T_MAX - T:]), torch.tensor([0.3] * 4), 625,
                          attention_mask=torch.from_numpy(mask[us][:, T_MAX - T:]), max_new_token=NEW_MAX, min_new_token=1, logits_warpers=LW,
                          logits_processors=LP, return_hidden=True, noise="device", seed=SEED, utt_ids=list(us), max_new_tokens_per_row=[lims[u] for u in us],
                          **kw))[-1]
    if kw.get("return_logprobs"):
        return {u: (out.ids[j].cpu(), out.hiddens[j].cpu(), out.logprobs[j].cpu(), out.sampled_logprobs[j].cpu()) for j, u in enumerate(us)}
    return {u: (out.ids[j].cpu(), out.hiddens[j].cpu()) for j, u in enumerate(us)}


def batch1_reference():
    """every utterance served alone (batch 1): the yardstick of the tests below.  Computed once, never modified."""
    if "b1" not in _ref:
        g = engine()
        lens, lims, ids, mask, emb = _emb(g)
        res = {}
        for u in range(N_UTT):
            res.update(_generate(g, [u], emb, ids, mask, lens, lims))
        _ref["b1"] = res
    return _ref["b1"]


def _same(ref, got, what):
    for u, t in got.items():
        (i, h), (ri, rh) = t[:2], ref[u][:2]
        assert torch.equal(i, ri), f"{what}: utterance {u} token ids differ from its batch-1 run"
        assert torch.equal(h, rh), f"{what}: utterance {u} hidden rows differ from its batch-1 run (max {float((h - rh).abs().max()) if h.shape == rh.shape else h.shape})"


def _plan(g, B):
    """the launch plan of a decode step at B rows: begin + prompt pass + first sample + one decode step, then GPT.decode_plan()"""
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects
    lens, lims, ids, mask, emb = _emb(g)
    dev, N = g.device, 4
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, N, N, LW, LP, 4)
    out_ids = torch.zeros(B, N, 4, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev); end = torch.zeros(B, dtype=torch.int32, device=dev)
    io = _lib.GenIO(ids=out_ids.data_ptr(), hiddens=None, finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    msk = torch.from_numpy(mask[:B]).to(dev).to(torch.int32).contiguous()
    embd = emb[:B].contiguous()
    _lib.check(g._lib.ctts_gpt_begin(g._h, B, T_MAX, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    _lib.check(g._lib.ctts_gpt_prefill(g._h, embd.data_ptr(), st), "prefill")
    _lib.check(g._lib.ctts_gpt_sample(g._h, st), "sample")
    _lib.check(g._lib.ctts_gpt_decode(g._h, 1, 0, st), "decode")
    torch.cuda.synchronize()
    return g.decode_plan()


# ---- 1. option surface ------------------------------------------------------------------------------------------------------------------------------------
def test_option_surface():
    """fails before the option exists: set_option answers "unknown option 'schedule_invariant'\""""
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models import GPT
    g = engine()
    assert g.get_option("schedule_invariant") == 1
    assert g.get_option("batch_invariant") == 1, "the contract reads under both names while it is on (share_prompt=None, sessions, generate_many rest on this)"
    # the pins read as the header says (fp16: the head / tail mechanisms read 0 = never)
    pins = {"persistent_rows": 0, "split_rows": 0, "down_splitk_rows": 1, "nbg2_rows": 0, "decode_splits": 1, "attn_wide_blocks": INT_MAX,
            "split_decode_rows": 0, "prefill_split_rows": 0, "valu_rows": 0, "split_nbg2_rows": 0, "prefill_splitk_rows": 0}
    for k, v in pins.items():
        assert g.get_option(k) == v, f"{k} reads {g.get_option(k)} under schedule_invariant, the header says {v}"
    g.set_option("schedule_invariant", 0)
    try:
        assert g.get_option("schedule_invariant") == 0 and g.get_option("batch_invariant") == 0
        assert g.get_option("split_rows") == 8 and g.get_option("nbg2_rows") == 57 and g.get_option("attn_wide_blocks") == 4096 and g.get_option("down_splitk_rows") == 9
    finally:
        g.set_option("schedule_invariant", 1)
    # "batch_invariant" stays refused on fp16, by a message that names both
    with pytest.raises(_lib.HipBackendError, match="batch_invariant.*schedule_invariant"):
        g.set_option("batch_invariant", 1)
    assert g.get_option("schedule_invariant") == 1
    # default 0 on either dtype; settable before finalize; a synonym of "batch_invariant" on fp32 engines
    for wd in ("fp16", "fp32"):
        d = GPT(LLAMA, max_batch=2, max_seq_len=64, weight_dtype=wd)
        try:
            assert d.get_option("schedule_invariant") == 0
            d.set_option("schedule_invariant", 5)
            assert d.get_option("schedule_invariant") == 1 and d.get_option("batch_invariant") == 1
            assert d.get_option("split_decode_rows") == (1 if wd == "fp32" else 0) and d.get_option("persistent_rows") == 0
            d.set_option("schedule_invariant", 0)
            assert d.get_option("batch_invariant") == 0
            if wd == "fp32":
                d.set_option("batch_invariant", 1)
                assert d.get_option("schedule_invariant") == 1
        finally:
            d.close()
    # per-utterance adapters: refused by the binding and by the engine itself, by a message naming the option
    with pytest.raises(_lib.HipBackendError, match="schedule_invariant"):
        g.set_row_adapters([0, -1])
    lens, lims, ids, mask, emb = _emb(g)
    arr = np.ascontiguousarray([0, -1], dtype=np.int32)
    _lib.check(g._lib.ctts_gpt_set_row_adapters(g._h, arr.ctypes.data_as(C.c_void_p), 2), "set_row_adapters")
    try:
        with pytest.raises(_lib.HipBackendError, match="schedule_invariant"):
            _generate(g, [0, 1], emb, ids, mask, lens, lims)
    finally:
        g.set_row_adapters(None)
    # caller-supplied noise: refused at begin
    with pytest.raises(_lib.HipBackendError, match="schedule_invariant"):
        list(g.generate(emb[:1, T_MAX - lens[0]:].contiguous(), torch.from_numpy(ids[:1, T_MAX - lens[0]:]), torch.tensor([0.3] * 4), 625, max_new_token=4,
                        logits_warpers=LW, logits_processors=LP, noise="torch"))
    _same(batch1_reference(), _generate(g, [0], emb, ids, mask, lens, lims), "after the refusals")          # the engine serves again
    # the decode plan at both sides of every fp16 row-count threshold: launch chain, 16-row chunks, S = 1 on 8-wave blocks, K sliced in the launch, no launch slices
    for B in (1, 5, 6, 9, 17, 57):
        p = _plan(g, B)
        assert p["B"] == B
        got = {k: p[k] for k in ("persist", "nbg", "S", "down_sk", "splitd", "xhm", "spd", "valu", "fuse_heads", "form_xh", "form_parts", "form_nbg", "wide_blocks")}
        assert got == dict(persist=0, nbg=1, S=1, down_sk=1, splitd=0, xhm=1, spd=0, valu=0, fuse_heads=0, form_xh=1, form_parts=0, form_nbg=1, wide_blocks=INT_MAX), (B, p)
        assert p["chunks"] == (B + 15) // 16


# ---- 2. row count and padding -----------------------------------------------------------------------------------------------------------------------------
def test_row_count_and_padding_invariance():
    """slices of 2 .. 60 utterances (both sides of the fp16 thresholds 5|6, 8|9, 16|17, 56|57; compaction crosses them again inside the larger ones), and the
    shortest prompt padded to the full width beside the five longest: hidden rows and ids equal the batch-1 run bit for bit"""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    rows = {}
    for size in (2, 5, 6, 8, 9, 16, 17, 33, 57, 60):
        got = {}
        for s0 in range(0, N_UTT, size):
            us = list(range(s0, min(s0 + size, N_UTT)))
            rows.setdefault(size, []).append(len(us) * (max(lens[u] for u in us) - 1))
            got.update(_generate(g, us, emb, ids, mask, lens, lims))
        _same(ref, got, f"slices of {size}")
    # the prompt passes spanned all three height bands of the default fp16 engine: under 64 rows, 64 .. 1535, 1536 and more
    assert any(lens[u] - 1 < 64 for u in range(N_UTT))          # (the batch-1 runs and the small slices)
    assert all(64 <= r < 1536 for r in rows[17][:3]), rows[17]
    assert rows[33][0] >= 1536 and rows[60][0] >= 1536, (rows[33], rows[60])
    shortest = min(range(N_UTT), key=lambda u: lens[u])
    longest = sorted(range(N_UTT), key=lambda u: -lens[u])[:5]
    _same(ref, _generate(g, [shortest] + longest, emb, ids, mask, lens, lims, trim=False), "short prompt beside the longest ones")
    assert lens[shortest] < 20 and max(lens) > 72


def test_attention_block_mates_do_not_matter():
    """The anchored prompt attention shares a 64-query block's key chunks among its queries: a chunk wholly outside a query's [first real key, own slot] must leave
    that query's running max, sum and accumulator bit-unchanged.  One utterance of 66 .. 78 tokens alone at batch 1, trimmed (no padding: queries 64.. of its
    second block all reach into the second chunk) and padded to the full width (pad queries in front extend the first block's chunks downwards; in the second
    block the queries below first key + 64 end before the chunk their block mates go on into)."""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    us = [u for u in range(N_UTT) if 66 <= lens[u] <= 78][:3]
    assert us, lens
    for u in us:
        _same(ref, _generate(g, [u], emb, ids, mask, lens, lims, trim=False), f"utterance {u} ({lens[u]} tokens) padded to {T_MAX}")


# ---- 3. pass boundaries -----------------------------------------------------------------------------------------------------------------------------------
def test_pass_boundaries_do_not_matter():
    ref = batch1_reference()
    g = engine(pass_rows=256)
    lens, lims, ids, mask, emb = _emb(g)
    us = list(range(17))
    assert len(us) * (max(lens[u] for u in us) - 1) > 2 * 256          # at least three passes, boundaries inside sequences
    _same(ref, _generate(g, us, emb, ids, mask, lens, lims), "17 utterances in prompt passes of 256 rows")


# ---- 4. generate_many -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,schedule", [(8, "fifo"), (32, "longest_first")])
def test_continuous_batching_and_compaction_invariance(rows, schedule):
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    g.schedule = schedule
    try:
        out = g.generate_many(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=NEW_MAX,
                              min_new_token=1, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=SEED, utt_ids=list(range(N_UTT)),
                              max_new_tokens_per_row=lims, rows=rows)
    finally:
        g.schedule = "fifo"
    assert g.admissions
    _same(ref, {u: (out.ids[u].cpu(), out.hiddens[u].cpu()) for u in range(N_UTT)}, f"generate_many on {rows} rows, {schedule}")


# ---- 5. session -------------------------------------------------------------------------------------------------------------------------------------------
def test_growing_session_equals_batch_1():
    """a DecodeSession whose batch grows 1 -> 6 -> 9 -> 17 and compacts back, one seated utterance cancelled on the way"""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    order = sorted(range(N_UTT), key=lambda u: -lims[u])[:17]          # the longest-running first: nobody ends before the batch has reached 17 rows
    assert all(lims[u] >= 13 for u in order[:9]), [lims[u] for u in order]
    msk = torch.from_numpy(mask)
    saved = g.compact_chunk
    g.compact_chunk = 4
    got, tk = {}, []

    def submit(us):
        return [ses.submit(emb[u, T_MAX - lens[u]:], msk[u, T_MAX - lens[u]:], u, limit=lims[u]) for u in us]

    def step():
        for r in ses.step():
            got[r.ticket] = r
    try:
        with g.open_session(torch.tensor([0.3] * 4), 625, NEW_MAX, min_new_token=1, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=SEED,
                            rows=17, out_slots=17) as ses:
            tk += submit(order[:1]); step(); step()
            tk += submit(order[1:6]); step()
            tk += submit(order[6:9]); step()
            tk += submit(order[9:17]); step()
            assert ses.cancel(tk[16])
            got.update({r.ticket: r for r in ses.drain()})
            trace = list(ses.batch_trace)
    finally:
        g.compact_chunk = saved
    print(f"batch_trace {trace}")
    sizes = [b for _, b in trace]
    assert [s for s in sizes if s in (6, 9, 17)][:3] == [6, 9, 17], sizes
    assert min(sizes[sizes.index(17):]) < 17, "no compaction after the growth"
    assert sorted(got) == sorted(tk)
    for j, u in enumerate(order[:16]):
        r = got[tk[j]]
        assert not r.cancelled and r.utt_id == u
        _same(ref, {u: (r.ids.cpu(), r.hiddens.cpu())}, "session")
    r, (ri, rh) = got[tk[16]], ref[order[16]][:2]
    n = int(r.ids.shape[0])
    assert r.cancelled and n <= ri.shape[0]
    assert torch.equal(r.ids.cpu(), ri[:n]) and torch.equal(r.hiddens.cpu(), rh[:n]), "the cancelled utterance's tokens so far differ from its batch-1 run"


def test_text_rows_beside_code_rows_in_a_session():
    """refine-text utterances as text rows of a code session (3 rows, grown to 6): every code row equals its batch-1 generate, every text row its batch-1
    generate(infer_text=True)"""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    msk = torch.from_numpy(mask)
    us, kinds = [30, 31, 32, 33, 34, 35], ["code", "text", "code", "text", "code", "text"]
    TXT = dict(temperature=0.7, top_P=0.7, top_K=20, eos_token=21177, max_new_token=12, min_new_token=1)
    got, tk = {}, []
    with g.open_session(torch.tensor([0.3] * 4), 625, NEW_MAX, min_new_token=1, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=SEED,
                        rows=6, out_slots=6, text_rows=TXT) as ses:
        for lo, hi in ((0, 3), (3, 6)):
            tk += [ses.submit(emb[u, T_MAX - lens[u]:], msk[u, T_MAX - lens[u]:], u, limit=lims[u] if k == "code" else None, mode=k) for u, k in zip(us[lo:hi], kinds[lo:hi])]
            for _ in range(2):
                got.update({r.ticket: r for r in ses.step()})
        got.update({r.ticket: r for r in ses.drain()})
    assert sorted(got) == sorted(tk)
    for t, u, k in zip(tk, us, kinds):
        r = got[t]
        assert r.mode == k and not r.cancelled
        if k == "code":
            _same(ref, {u: (r.ids.cpu(), r.hiddens.cpu())}, "code row beside text rows")
        else:
            i1 = torch.from_numpy(ids[u:u + 1, T_MAX - lens[u]:])
            one = list(g.generate(emb[u:u + 1, T_MAX - lens[u]:].contiguous(), i1, torch.tensor([0.7]), 21177, attention_mask=msk[u:u + 1, T_MAX - lens[u]:], max_new_token=12,
                                  min_new_token=1, logits_warpers=LW, infer_text=True, noise="device", seed=SEED, utt_ids=[u]))[-1].ids[0].cpu()
            assert one.shape[0] >= 1 and torch.equal(r.ids.cpu().flatten(), one.flatten()), f"text row {u}: ids differ from its batch-1 refine-text call"


# ---- 6. other paths ---------------------------------------------------------------------------------------------------------------------------------------
def test_refine_text_pass_invariance():
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)

    def run(sel):
        T = max(lens[u] for u in sel)
        ii = torch.as_tensor(sel, dtype=torch.long)
        out = list(g.generate(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(ids[sel][:, T_MAX - T:]), torch.tensor([0.7]), 21177,
                              attention_mask=torch.from_numpy(mask[sel][:, T_MAX - T:]), max_new_token=12, min_new_token=1, logits_warpers=LW,
                              infer_text=True, return_hidden=True, noise="device", seed=SEED, utt_ids=sel))[-1]
        return {u: (out.ids[j].cpu(), out.hiddens[j].cpu()) for j, u in enumerate(sel)}

    us = list(range(9))
    alone = {}
    for u in us:
        alone.update(run([u]))
    _same(alone, run(us), "refine-text pass, slice of 9")


def test_shared_prompt_pass_equals_unshared():
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    prompts = [3, 4, 5]
    T = max(lens[u] for u in prompts)
    pof = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    sel = torch.tensor([prompts[p] for p in pof])
    pi = torch.tensor(prompts)
    kw = dict(max_new_token=NEW_MAX, min_new_token=1, logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="device", seed=SEED,
              utt_ids=[900 + i for i in range(9)], max_new_tokens_per_row=[6, 16, 11, 16, 7, 12, 9, 16, 8])
    ids_t, mask_t = torch.from_numpy(ids)[:, T_MAX - T:], torch.from_numpy(mask)[:, T_MAX - T:]
    e = emb[:, T_MAX - T:]
    shared = list(g.generate(e[pi.cuda()].contiguous(), ids_t[pi], torch.tensor([0.3] * 4), 625, attention_mask=mask_t[pi], prompt_of=pof, **kw))[-1]
    assert g.shared_prompts == [(9, 3)]
    plain = list(g.generate(e[sel.cuda()].contiguous(), ids_t[sel], torch.tensor([0.3] * 4), 625, attention_mask=mask_t[sel], **kw))[-1]
    assert g.shared_prompts == []
    for j in range(9):
        assert torch.equal(shared.ids[j].cpu(), plain.ids[j].cpu()) and torch.equal(shared.hiddens[j].cpu(), plain.hiddens[j].cpu()), j
    assert not torch.equal(shared.ids[0][:4].cpu(), shared.ids[1][:4].cpu())          # (other utterance ids: other noise)


def test_score_alone_equals_padded_batch():
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    us = sorted(range(N_UTT), key=lambda u: lens[u])[10:50:9][:5]
    assert len(us) == 5 and len({lens[u] for u in us}) > 1
    n = 8
    rng = np.random.Generator(np.random.Philox(key=99))
    tg = torch.from_numpy(rng.integers(0, 626, size=(N_UTT, n, 4)).astype(np.int64))
    T = max(lens[u] for u in us)
    ii = torch.as_tensor(us, dtype=torch.long)
    both = g.score(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(mask[us][:, T_MAX - T:]), tg[ii], [n] * 5)
    for j, u in enumerate(us):
        one = g.score(emb[u:u + 1, T_MAX - lens[u]:].contiguous(), torch.from_numpy(mask[u:u + 1, T_MAX - lens[u]:]), tg[u:u + 1], [n])
        assert torch.equal(one.logprob[0], both.logprob[j]) and torch.equal(one.argmax[0], both.argmax[j]), f"utterance {u}: scored alone != in the padded batch of 5"
    _same(batch1_reference(), _generate(g, [0], emb, ids, mask, lens, lims), "generate after score")


def test_logprobs_are_equal_too():
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    us = list(range(20, 29))
    both = _generate(g, us, emb, ids, mask, lens, lims, return_logprobs=True)
    _same(batch1_reference(), both, "slice of 9 with log-probs")
    for u in us[::4]:
        one = _generate(g, [u], emb, ids, mask, lens, lims, return_logprobs=True)[u]
        assert torch.equal(one[2], both[u][2]) and torch.equal(one[3], both[u][3]), f"utterance {u}: log-probs differ from its batch-1 run"


# ---- 7. fidelity under the option -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,pad,N", [(1, 48, None, 64), (32, 24, [i % 17 for i in range(32)], 24)])
def test_mel_and_waveform_tolerance_under_the_option(B, T, pad, N):
    """the pinned stack against the CPU oracle (teacher forced): mel / waveform relative RMS within the project's stated fp16 bound"""
    from chatttsplus_amd.hip_models import Synth
    from oracle import ref_cpu
    from tests.test_gpu_fp16_parity import MEL_WAV_TOL, _rel_rms, teacher_forced_hiddens
    g, sd = engine(), state_dict()
    if "syn" not in _ref:
        s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=256, max_batch=32)
        dsd, vsd = synth.dvae_state_dict(synth.DVAE_REAL, 1234), synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
        s.load("dvae.", dsd); s.load("vocos.", vsd)
        _ref["syn"] = (s, dsd, vsd)
    s, dsd, vsd = _ref["syn"]
    ids, mask = synth.prompt_ids(B, T, synth.GPT_REAL["num_text_tokens"], 700 + B, pad_left=pad)
    o = ref_cpu.OracleGPT(sd, 12)
    emb = o.embed(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
    ref = o.generate(emb, torch.from_numpy(ids), ref_cpu.SamplerParams(min_new_token=N), attention_mask=torch.from_numpy(mask), max_new_token=N,
                     noise=ref_cpu.SeededNoise(9))
    hid = teacher_forced_hiddens(g, emb, mask, torch.stack(list(ref.ids), 0).to(torch.int32), N)
    wavs = s.decode_batch([hid[b] for b in range(B)])
    worst = dict(hid=0.0, mel=0.0, wav=0.0)
    for b in (range(B) if B <= 4 else range(0, B, 5)):
        mel_ref = ref_cpu.dvae_decode(dsd, ref.hiddens[b])
        wav_ref = ref_cpu.vocos_decode(vsd, mel_ref).numpy()
        worst["hid"] = max(worst["hid"], _rel_rms(hid[b].cpu().numpy(), ref.hiddens[b].numpy()))
        worst["mel"] = max(worst["mel"], _rel_rms(s.dvae_decode(hid[b]).cpu().numpy(), mel_ref.numpy()))
        worst["wav"] = max(worst["wav"], _rel_rms(wavs[b].cpu().numpy(), wav_ref))
    print(f"fp16 schedule_invariant parity B={B} N={N}: rel-RMS hidden {worst['hid']:.2e} mel {worst['mel']:.2e} wav {worst['wav']:.2e}")
    assert worst["mel"] <= MEL_WAV_TOL["fp16"] and worst["wav"] <= MEL_WAV_TOL["fp16"], worst


# ---- 8. off by default ------------------------------------------------------------------------------------------------------------------------------------
def test_off_by_default_the_plans_are_todays():
    """with the option at 0 an fp16 engine plans what tests/test_gpu_decode_plans.py expects of it at 1, 9 and 57 rows"""
    from tests.test_gpu_decode_plans import XH16, plan_mismatches
    g = engine(options={})
    assert g.get_option("schedule_invariant") == 0 and g.get_option("batch_invariant") == 0
    want = {1: dict(persist=1, valu=0, fuse_heads=1, form_logits=1, form_parts=0, form_xh=0, S=">2"),
            9: dict(nbg=1, chunks=1, down_sk=1, pf_kb=0, **XH16),
            57: dict(nbg=2, chunks=2, down_sk=0, pf_kb=">0", form_nbg=2, attn_wave8=1, **XH16)}
    for B, expect in want.items():
        p = _plan(g, B)
        assert p["B"] == B
        bad = plan_mismatches(p, expect)
        assert not bad, f"default fp16 engine at {B} rows: " + "; ".join(bad) + f" (plan {p})"
