"""Teacher-forced scoring of audio codes (ctts_gpt_score, include/ctts_hip.h; GPT.score; ChatTTSPlusPipeline.score).

Checked here: log-probabilities and argmaxes against the oracle's forward + code heads + log_softmax (fp32 and fp16 engines, short and long prompt
passes, several passes); agreement with the decode path's logits under forced ids; a sequence scores the same alone as inside a padded batch (bit for
bit under batch_invariant, also across pass boundaries); per-utterance adapters against a merged-adapter engine; errors, and generate() before and
after a score() call bit-identical; the pipeline's codes and wavs paths.  Synthetic weights at real widths, 4 decoder layers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects, score_inputs
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

CFG4 = dict(synth.GPT_REAL, num_hidden_layers=4)
LLAMA4 = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=4)
SEED = 4321
EOS = 625
_engines = {}


def _sd():
    if "sd" not in _engines:
        _engines["sd"] = synth.gpt_state_dict(CFG4, SEED)
    return _engines["sd"]


def engine(dtype="fp32", options=None, pass_rows=None, max_batch=8, max_seq=256):
    from chatttsplus_amd.hip_models import GPT
    key = (dtype, tuple(sorted((options or {}).items())), pass_rows, max_batch, max_seq)
    if key not in _engines:
        if pass_rows:
            os.environ["CTTS_PASS_ROWS"] = str(pass_rows)      # read once at finalize (as tests/test_gpu_gpt.py sets it)
        try:
            g = GPT(LLAMA4, max_batch=max_batch, max_seq_len=max_seq, weight_dtype=dtype, options=dict(options or {}))
            g.load_state_dict(_sd())
        finally:
            os.environ.pop("CTTS_PASS_ROWS", None)
        _engines[key] = g
    return _engines[key]


def oracle():
    if "oracle" not in _engines:
        _engines["oracle"] = ref_cpu.OracleGPT(_sd(), 12)
    return _engines["oracle"]


def case(plens, ncodes, T0, seed, append_eos=True):
    """Prompts of plens[b] text tokens (left padded to T0), ncodes[b] random codes each -> score_inputs' dict."""
    g = torch.Generator().manual_seed(seed)
    B = len(plens)
    ids = torch.zeros(B, T0, 4, dtype=torch.long)
    mask = torch.zeros(B, T0, dtype=torch.long)
    for b, n in enumerate(plens):
        ids[b, T0 - n:] = torch.randint(0, CFG4["num_text_tokens"], (n, 1), generator=g).expand(n, 4)
        mask[b, T0 - n:] = 1
    codes = [torch.randint(0, 625, (n, 4), generator=g) for n in ncodes]
    return score_inputs(ids, mask, mask.bool(), codes, EOS, append_eos=append_eos)


def run(g, si):
    emb = g(si["ids"], si["text_mask"])
    return g.score(emb, si["mask"], si["targets"], si["n_targets"])


def oracle_scores(si):
    """OracleGPT.forward over the whole sequences at positions cumsum(mask) - 1 (pads 1), code_logits on every row, log_softmax."""
    o = oracle()
    ids, mask = si["ids"], si["mask"].to(torch.long)
    B, T = mask.shape
    emb = o.embed(ids, si["text_mask"])
    pos = (mask.cumsum(1) - 1).masked_fill(mask == 0, 1)
    o.alloc_cache(B, T)
    with torch.no_grad():
        hid = o.forward(emb, mask, pos)
        lg = torch.stack([torch.nn.functional.linear(hid, w) for w in o.head_code], 2)     # [B, T, 4, V]
    out = []
    for b in range(B):
        n = int(si["n_targets"][b])
        rows = lg[b, T - n:]
        ls = torch.log_softmax(rows, -1)
        t = si["targets"][b, :n].to(torch.long)
        top2 = rows.topk(2, -1).values
        out.append((ls.gather(-1, t[..., None])[..., 0], rows.argmax(-1), top2[..., 0] - top2[..., 1]))
    return out


def check_vs_oracle(res, ref, tol):
    worst = 0.0
    for b, (lp, am, gap) in enumerate(ref):
        d = float((res.logprob[b] - lp).abs().max())
        worst = max(worst, d)
        assert d <= tol, f"sequence {b}: |dlogprob| {d} > {tol}"
        sure = gap > 1e-3
        assert torch.equal(res.argmax[b][sure], am[sure]), f"sequence {b}: argmax differs where the oracle's top-2 gap is > 1e-3"
    return worst


# ---- 1. against the oracle: both prompt-pass families, with and without EOS ------------------------------------------------------------
@pytest.mark.parametrize("append_eos", [True, False])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_score_vs_oracle_fp32(shape, append_eos):
    if shape == "short":        # 2 x 27 rows: < 65, the decode kernels' prompt pass
        si = case([12, 9], [5, 14], 12, 11, append_eos)
        assert int(si["mask"].numel()) < 65
    else:                       # 3 sequences, 5..40 codes, different left pads: >= 65 rows, the split GEMMs
        si = case([16, 12, 7], [5, 23, 40], 16, 12, append_eos)
        assert int(si["mask"].numel()) >= 65
    res = run(engine(), si)
    check_vs_oracle(res, oracle_scores(si), 2e-4)
    assert res.nll.shape == (len(res.logprob),) and 0.0 <= res.accuracy <= 1.0


# ---- 2. several passes -------------------------------------------------------------------------------------------------------------------
def test_score_several_passes():
    si = case([30, 21, 9, 40], [120, 33, 150, 5], 40, 21)
    assert int(si["mask"].numel()) > 2 * 256                    # 4 x 160 rows: three passes, sequences straddle the boundaries
    res = run(engine(pass_rows=256), si)
    check_vs_oracle(res, oracle_scores(si), 2e-4)


# ---- 3. agreement with the decode path -----------------------------------------------------------------------------------------------------
def test_score_matches_decode_logits_under_forced_ids():
    g = engine()
    B, N = 2, 10
    si = case([14, 10], [N, N], 14, 31, append_eos=False)
    T0 = 14
    codes = si["targets"].to(torch.int32)                         # [B, N, 4]
    res = run(g, si)
    # the same prompts through begin / prefill / sample, then the codes forced one by one
    ids = si["ids"][:, :T0]; mask = si["mask"][:, :T0]
    emb = g(ids, si["text_mask"][:, :T0]).contiguous()
    lib, h, dev = g._lib, g._h, g.device
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), EOS, N, N, [], [], 4)
    out_ids = torch.zeros(B, N, 4, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev); end = torch.zeros(B, dtype=torch.int32, device=dev)
    io = _lib.GenIO(ids=out_ids.data_ptr(), hiddens=None, finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    msk = mask.to(dev).to(torch.int32).contiguous()
    _lib.check(lib.ctts_gpt_begin(h, B, T0, msk.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
    _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")
    _lib.check(lib.ctts_gpt_sample(h, st), "sample")
    steps = [g.last_logits(B).cpu()]
    forced = codes.to(dev)
    for i in range(1, N):
        f = forced[:, i - 1].contiguous()
        _lib.check(lib.ctts_gpt_force_ids(h, f.data_ptr(), st), "force")
        _lib.check(lib.ctts_gpt_decode(h, 1, 0, st), "decode")
        steps.append(g.last_logits(B).cpu())
    lg = torch.stack(steps, 1)                                    # [B, N, 4, V]
    ls = torch.log_softmax(lg, -1).gather(-1, codes.to(torch.long)[..., None])[..., 0]
    for b in range(B):
        d = float((res.logprob[b] - ls[b]).abs().max())
        assert d <= 2e-4, f"sequence {b}: score vs decode logits {d}"


# ---- 4. padding independence -------------------------------------------------------------------------------------------------------------
def _alone_and_batched(g_alone, g_batch, si_batch, row):
    """Sequence `row` of si_batch scored alone (its own unpadded layout) and inside the batch."""
    n = int(si_batch["mask"][row].sum())
    one = {k: (v[row:row + 1, -n:] if k in ("ids", "mask", "text_mask") else v[row:row + 1]) for k, v in si_batch.items()}
    return run(g_alone, one), run(g_batch, si_batch)


def test_score_padding_independence_default():
    g = engine()
    si = case([16, 12, 7], [5, 23, 40], 16, 41)
    for row in range(3):
        a, bt = _alone_and_batched(g, g, si, row)
        assert float((a.logprob[0] - bt.logprob[row]).abs().max()) <= 2e-5, f"row {row}"


def test_score_batch_invariant_bit_identical():
    inv = engine(options={"batch_invariant": 1})
    inv_p = engine(options={"batch_invariant": 1}, pass_rows=256)
    x = case([11], [19], 11, 51)                                  # the sequence under test: 11 prompt rows, 19 codes
    ref = run(inv, x)
    xp, xc = x["ids"][0, :11], x["targets"][0, :19].to(torch.long)

    def mixed(B, row, seed):
        """x at `row` of a batch of B random sequences (other prompt lengths, hence other left pads)."""
        gg = torch.Generator().manual_seed(seed)
        plens = [int(torch.randint(3, 40, (1,), generator=gg)) for _ in range(B)]
        ncodes = [int(torch.randint(3, 90, (1,), generator=gg)) for _ in range(B)]
        plens[row] = 11
        T0 = max(plens)
        ids = torch.zeros(B, T0, 4, dtype=torch.long); mask = torch.zeros(B, T0, dtype=torch.long)
        codes = []
        for b in range(B):
            if b == row:
                src, cb = xp, xc
            else:
                src = torch.randint(0, CFG4["num_text_tokens"], (plens[b], 1), generator=gg).expand(-1, 4)
                cb = torch.randint(0, 625, (ncodes[b], 4), generator=gg)
            ids[b, T0 - plens[b]:] = src; mask[b, T0 - plens[b]:] = 1
            codes.append(cb)
        return score_inputs(ids, mask, mask.bool(), codes, EOS)

    for g, B, row, seed in ((inv, 3, 1, 52), (inv, 8, 5, 53), (inv_p, 8, 6, 54), (inv_p, 3, 0, 55)):
        si = mixed(B, row, seed)
        if g is inv_p and B == 8:
            assert int(si["mask"].numel()) > 2 * 256          # several passes
        res = run(g, si)
        assert torch.equal(res.logprob[row], ref.logprob[0]), f"B={B} row {row}: logprob not bit-identical"
        assert torch.equal(res.argmax[row], ref.argmax[0]), f"B={B} row {row}: argmax differs"


def boundary_case():
    """Nine unpadded sequences of 256 tokens with 2298 targets: more scored rows in ONE pass than a heads launch takes (SCORE_ROWS = 2048 in gpt_engine.hip), sequence 8
    straddling row 2048 of the gathered rows.  -> ids, mask, text_mask, targets, n_targets"""
    B, T = 9, 256
    n = [256] * 7 + [250, 256]
    assert sum(n) > 2048 and sum(n[:8]) < 2048
    gen = torch.Generator().manual_seed(57)
    ids = torch.randint(0, CFG4["num_text_tokens"], (B, T, 1), generator=gen).expand(-1, -1, 4).contiguous()
    targets = torch.randint(0, 625, (B, T, 4), generator=gen, dtype=torch.int32)
    return ids, torch.ones(B, T, dtype=torch.int32), torch.ones(B, T, dtype=torch.bool), targets, torch.tensor(n, dtype=torch.int32)


def test_score_chunk_boundary_schedule_independent():
    """boundary_case under batch_invariant: the nine scored together equal, bit for bit, the same sequences scored as eight and one"""
    ids, mask, tm, targets, nt = boundary_case()
    B, T = mask.shape
    assert (B, T) == (9, 256) and int(nt.sum()) > 2048
    g = engine(options={"batch_invariant": 1}, max_batch=B, max_seq=T)
    emb = g(ids, tm)
    whole = g.score(emb, mask, targets, nt)
    plan = g.prompt_plan()
    assert plan["passes"] == 1 and plan["rows_full"] >= B * T          # one pass holds all nine, so its 2298 scored rows take two heads launches
    parts = [g.score(emb[lo:hi], mask[lo:hi], targets[lo:hi], nt[lo:hi]) for lo, hi in ((0, 8), (8, 9))]
    for b in range(B):
        part, row = (parts[0], b) if b < 8 else (parts[1], 0)
        assert whole.logprob[b].shape == (int(nt[b]), 4)
        assert torch.equal(whole.logprob[b], part.logprob[row]), f"sequence {b}: logprob not bit-identical"
        assert torch.equal(whole.argmax[b], part.argmax[row]), f"sequence {b}: argmax differs"


# ---- 5. per-utterance adapters -------------------------------------------------------------------------------------------------------------
def test_score_adapters_vs_merged():
    rng = np.random.Generator(np.random.Philox(key=83))
    ad = []
    for l in range(4):
        for t in ("q_proj", "k_proj", "v_proj", "o_proj"):
            ad.append((l, t, (rng.standard_normal((8, 768)) * 0.05).astype(np.float32), (rng.standard_normal((768, 8)) * 0.05).astype(np.float32), 2.0))
    base = engine()
    merged = base.with_lora(ad)
    try:
        base.load_adapter(0, ad)
        si = case([16, 12, 7], [5, 23, 40], 16, 61)
        plain = run(base, si)
        mrg = run(merged, si)
        base.set_row_adapters([0, -1, 0])
        try:
            mixed = run(base, si)
        finally:
            base.set_row_adapters(None)
        for b, slot in enumerate([0, -1, 0]):
            ref, tol = (mrg, 2e-4) if slot >= 0 else (plain, 2e-5)
            d = float((mixed.logprob[b] - ref.logprob[b]).abs().max())
            assert d <= tol, f"row {b} (slot {slot}): {d}"
        assert float((mixed.logprob[0] - plain.logprob[0]).abs().max()) > 1e-3, "the adapter changed nothing"
    finally:
        merged.close()
        base.set_row_adapters(None)


# ---- 6. fp16 engine against the oracle -----------------------------------------------------------------------------------------------------
FP16_TOL = 4e-3


def test_score_fp16_vs_oracle():
    """fp16 weights and KV: the largest |dlogprob| against the fp32 oracle measured over these two cases on an MI355X was 1.948e-3; the bound
    (FP16_TOL) is 2x that, rounded up."""
    g = engine("fp16")
    worst = 0.0
    for si in (case([12, 9], [5, 14], 12, 11), case([16, 12, 7], [5, 23, 40], 16, 12)):
        res = run(g, si)
        for b, (lp, am, gap) in enumerate(oracle_scores(si)):
            worst = max(worst, float((res.logprob[b] - lp).abs().max()))
    print(f"fp16 score: max |dlogprob| vs oracle = {worst:.3e}")
    assert worst <= FP16_TOL


# ---- 7. errors and state -------------------------------------------------------------------------------------------------------------------
def _gen(g, seed=3):
    ids, mask = synth.prompt_ids(2, 12, CFG4["num_text_tokens"], 71, pad_left=[0, 3])
    emb = g(torch.from_numpy(ids), torch.ones(2, 12, dtype=torch.bool))
    out = list(g.generate(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS, attention_mask=torch.from_numpy(mask), max_new_token=12,
                          min_new_token=12, return_hidden=True, noise="device", seed=seed))[-1]
    return [i.cpu() for i in out.ids], [h.cpu() for h in out.hiddens]


def test_score_errors_and_generate_state():
    g = engine()
    before = _gen(g)
    si = case([12, 9], [5, 14], 12, 81)
    emb = g(si["ids"], si["text_mask"])
    right = si["mask"].flip(1)
    with pytest.raises(ValueError, match="LEFT"):
        g.score(emb, right, si["targets"], si["n_targets"])
    bad = si["targets"].clone(); bad[1, 2, 3] = 626
    with pytest.raises(ValueError, match="outside"):
        g.score(emb, si["mask"], bad, si["n_targets"])
    nt = si["n_targets"].clone(); nt[0] = emb.shape[1] + 1
    big = torch.zeros(2, emb.shape[1] + 1, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="n_targets"):
        g.score(emb, si["mask"], big, nt)
    long_si = case([250], [40], 250, 82)
    with pytest.raises(ValueError, match="max_seq"):
        run(g, long_si)
    # the C layer names its limits too
    tg = si["targets"].to(torch.int32).cuda(); msk = si["mask"].cuda()
    nta = np.array([3, 300], dtype=np.int32)
    lp = torch.empty(2, si["targets"].shape[1], 4, device="cuda"); am = torch.empty(2, si["targets"].shape[1], 4, dtype=torch.int32, device="cuda")
    rc = g._lib.ctts_gpt_score(g._h, 2, int(emb.shape[1]), msk.data_ptr(), emb.data_ptr(), tg.data_ptr(), nta.ctypes.data_as(C.c_void_p),
                               int(si["targets"].shape[1]), lp.data_ptr(), am.data_ptr(), g._stream())
    assert rc != 0 and b"n_targets[1]" in g._lib.ctts_last_error()
    # a live generate() on this engine (or one sharing its KV cache) refuses scoring
    ids, mask = synth.prompt_ids(1, 8, CFG4["num_text_tokens"], 72)
    gen = g.generate(g(torch.from_numpy(ids), torch.ones(1, 8, dtype=torch.bool)), torch.from_numpy(ids), torch.tensor([0.3] * 4), EOS,
                     attention_mask=torch.from_numpy(mask), max_new_token=64, min_new_token=64, stream=True, stream_batch=4, noise="device", seed=1)
    next(gen)
    try:
        with pytest.raises(_lib.HipBackendError, match="generate"):
            g.score(emb, si["mask"], si["targets"], si["n_targets"])
    finally:
        gen.close()
    # entries beyond n_b are 0 / -1
    res_dev = run(g, si)
    assert len(res_dev.logprob[0]) == int(si["n_targets"][0])
    after = _gen(g)
    for b in range(2):
        assert torch.equal(before[0][b], after[0][b]) and torch.equal(before[1][b], after[1][b]), f"generate() after score() differs, row {b}"


def test_score_pads_unused_entries():
    g = engine()
    si = case([12, 9], [5, 14], 12, 83)
    emb = g(si["ids"], si["text_mask"])
    B, maxt = 2, int(si["targets"].shape[1])
    tg = si["targets"].to(torch.int32).cuda(); msk = si["mask"].cuda()
    nta = si["n_targets"].numpy().astype(np.int32)
    lp = torch.full((B, maxt, 4), 7.0, device="cuda"); am = torch.full((B, maxt, 4), 7, dtype=torch.int32, device="cuda")
    _lib.check(g._lib.ctts_gpt_score(g._h, B, int(emb.shape[1]), msk.data_ptr(), emb.data_ptr(), tg.data_ptr(), nta.ctypes.data_as(C.c_void_p), maxt,
                                     lp.data_ptr(), am.data_ptr(), g._stream()), "score")
    lp, am = lp.cpu(), am.cpu()
    n0 = int(nta[0])
    assert bool((lp[0, n0:] == 0).all()) and bool((am[0, n0:] == -1).all())
    assert bool((lp[0, :n0] < 0).all()) and bool((am[0, :n0] >= 0).all())


# ---- 8. the pipeline -----------------------------------------------------------------------------------------------------------------------
def test_pipeline_score_codes_and_wavs(tmp_path):
    from chatttsplus_amd.hip_models import DVAEEncoder, GPT
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams
    g = GPT(LLAMA4, max_batch=4, max_seq_len=256, weight_dtype="fp32")
    g.load_state_dict(_sd())
    pipe = ChatTTSPlusPipeline.from_components(g, None, synth.toy_tokenizer(str(tmp_path / "tok")), torch.device("cuda:0"))
    try:
        texts = synth.toy_texts(3, 8, 30, seed=91)
        params = InferCodeParams(prompt="", temperature=0.3, show_tqdm=False)
        gcodes = torch.Generator().manual_seed(92)
        codes = [torch.randint(0, 625, (n, 4), generator=gcodes) for n in (7, 19, 12)]
        res = pipe.score(texts, codes=codes, params_infer_code=params)
        ids, mask, tm = pipe._code_prompt(texts, params, g)
        si = score_inputs(ids.cpu(), mask.cpu(), tm.cpu(), codes, EOS)
        ref = g.score(g(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])
        for b in range(3):
            assert torch.equal(res.logprob[b], ref.logprob[b]) and torch.equal(res.argmax[b], ref.argmax[b])
        assert res.loss == ref.loss and res.accuracy == ref.accuracy
        # wavs: encoded by the dvae_encode model (built as tests/test_gpu_encoder.py builds it), then scored
        enc = DVAEEncoder(dim=512, max_seconds=8.0, pre_bound=True)
        enc.load_state_dict(synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234))
        pipe.models_dict["dvae_encode"] = enc
        rng = np.random.Generator(np.random.Philox(key=93))
        wavs = [torch.from_numpy((rng.standard_normal(n) * 0.1).astype(np.float32)) for n in (6000, 9000)]
        res_w = pipe.score(texts[:2], wavs=wavs, params_infer_code=params)
        wcodes = [enc(w.view(1, -1).cuda(), "encode")[0].t().cpu() for w in wavs]
        res_c = pipe.score(texts[:2], codes=wcodes, params_infer_code=params)
        for b in range(2):
            assert torch.equal(res_w.logprob[b], res_c.logprob[b]) and torch.equal(res_w.argmax[b], res_c.argmax[b])
    finally:
        g.close()
