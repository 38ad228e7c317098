"""Every decode launch plan against the CPU oracle.

plan_layers (gpt_engine.hip) picks a kernel chain per decode step from the dtype, the row count, the longest context and a dozen options.  Each case below
names the plan it was written for (GPT.decode_plan(), read back from the engine after every decode call) and then pins that plan's numbers to the oracle:
the hidden row AND the code logits of every step, teacher-forced with the oracle's own ids.  A moved threshold fails a case on its plan assertion -- it does
not silently move the case to another kernel chain -- and test_cases_cover_every_plan_feature fails when a plan feature has no case at all.

Tolerances are the project's (tests/test_gpu_gpt.py): per row rms-rel <= tol and max abs <= 4 tol scale with tol = 2e-5 (fp32 engines) / 2e-3
(fp16 engines: weights and KV rounded to fp16, fp32 accumulate); logits max abs <= 4 tol max(|ref|max, 1).

The oracle result of a shape is computed once (module cache keyed by (B, T, pads, N)) and shared by the dtype and option variants of that shape.
tools/decode_plan_oracle.py runs the same cases through the same driver and records the figures (profiles/decode_plan_oracle.jsonl)."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

from chatttsplus_amd import synth
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
TOL = {"fp32": 2e-5, "fp16": 2e-3}
# engines: (max_batch, max_seq_len).  "wide" serves the row-count sweep, "long" the context edges, "full" the cases that fill every KV lane to max_seq
ENGINES = {"wide": (128, 160), "long": (17, 800), "full": (9, 64)}

Case = namedtuple("Case", "wd engine opts B T pads N expect")

# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
# `expect` pins decode_plan() fields: an int is an exact value, ">0" / ">1" / ">2" a lower bound.  The values follow plan_layers with the engines' defaults:
# persistent_rows 8 (fp32) / 5 (fp16), valu_rows 2, split_rows 8, split_decode_rows 9, split_nbg2_rows 17, down_splitk_rows 9, nbg2_rows 81 (fp32) / 57 (fp16),
# attn_wide_blocks 512 (fp32) / 4096 (fp16), weight prefetch on the packed path from 9 (fp32 head / tail operands) / 17 (fp16) rows.
CASES = []


def sweep_pads(B, T=12):
    """pads (5 i) % 11, the last row of a batch left with a single real key"""
    p = [(5 * i) % 11 for i in range(B)]
    if B > 1:
        p[-1] = T - 1
    return tuple(p)


def _sweep(wd, opts, rows, **expect):
    for B in rows:
        CASES.append(Case(wd, "wide", dict(opts), B, 12, sweep_pads(B), 4, dict(expect)))


def _ctx(wds, opts, T, lengths, engine="long", N=4, **expect):
    """one case per dtype; an expectation named fp32_<field> / fp16_<field> holds for that dtype only"""
    for wd in wds:
        e = {k: v for k, v in expect.items() if not k.startswith(("fp32_", "fp16_"))}
        e.update({k[5:]: v for k, v in expect.items() if k.startswith(wd + "_")})
        CASES.append(Case(wd, engine, dict(opts), len(lengths), T, tuple(T - n for n in lengths), N, e))


CHAIN = dict(persist=0, fuse_heads=0, form_logits=0)
# the persistent launch: one (row, head) item per attention workgroup up to 5 rows, two from 6 rows on (fp32 only); VALU products and the fused heads up to 2 rows
_sweep("fp32", {}, (1, 2), persist=1, valu=1, fuse_heads=1, form_logits=1, form_parts=0, form_xh=0, S=">2")
_sweep("fp32", {}, (3, 5), persist=1, valu=0, fuse_heads=0, form_logits=0, form_parts=0, form_xh=0, S=1)
_sweep("fp32", {}, (6, 8), persist=1, valu=0, fuse_heads=0, form_logits=0, form_parts=0, form_xh=0, S=1)      # (two items per workgroup: the kernel's R > 5 instances)
# head / tail fp16 operands (spd) on the packed residual stream: one 16-row chunk with the in-launch split-K combine, then 32-row blocks from 17 rows on
SPD = dict(CHAIN, S=1, valu=0, splitd=0, xhm=1, spd=1, down_sk=1, pf_kb=">0", form_parts=0, form_xh=1, form_split=1)
_sweep("fp32", {}, (9, 16), nbg=1, chunks=1, form_nbg=1, attn_wave8=1, **SPD)
_sweep("fp32", {}, (31,), nbg=2, chunks=1, form_nbg=2, attn_wave8=1, **SPD)
_sweep("fp32", {}, (43, 64), nbg=2, chunks=2, attn_wave8=0, **SPD)      # 43: the first row count whose rows x heads reach attn_wide_blocks (4-wave attention blocks), 11-row tail block
_sweep("fp32", {}, (65,), nbg=2, chunks=">2", attn_wave8=0, **SPD)       # a 1-row tail block
_sweep("fp32", {}, (128,), nbg=2, chunks=">2", attn_wave8=0, **SPD)
# the launch chain below the persistent launch's rows: VALU / exact-f32 MFMA products, the down projection as split-K launch slices, S = its cap at 1-2 rows
SLICES = dict(CHAIN, splitd=1, xhm=0, spd=0, down_sk=0, pf_kb=0, nbg=1, chunks=1, form_parts=1, form_xh=0, form_split=0)
_sweep("fp32", {"persistent_rows": 0}, (1, 2), S=">2", valu=1, form_valu=1, **SLICES)
_sweep("fp32", {"persistent_rows": 0}, (3, 4, 8), S=1, valu=0, form_valu=0, **SLICES)
_sweep("fp32", {"persistent_rows": 0, "valu_rows": 0}, (1, 2), S=">2", valu=0, form_valu=0, **SLICES)
_sweep("fp32", {"persistent_rows": 0, "valu_rows": 4}, (3, 4), S=1, valu=1, form_valu=1, **SLICES)
# the exact-f32 packed path (what a checkpoint outside the fp16 range falls back to): 16-row chunks up to 80 rows, 32-row blocks from 81
EXACT = dict(CHAIN, S=1, valu=0, splitd=0, xhm=1, spd=0, pf_kb=0, form_parts=0, form_xh=1, form_split=0)
_sweep("fp32", {"split_decode_rows": 0}, (9, 16), nbg=1, chunks=1, down_sk=1, **EXACT)
_sweep("fp32", {"split_decode_rows": 0}, (17,), nbg=1, chunks=2, down_sk=1, **EXACT)
_sweep("fp32", {"split_decode_rows": 0}, (33,), nbg=1, chunks=">2", down_sk=1, attn_wave8=1, **EXACT)
_sweep("fp32", {"split_decode_rows": 0}, (80,), nbg=1, chunks=">2", down_sk=1, attn_wave8=0, **EXACT)
_sweep("fp32", {"split_decode_rows": 0}, (81, 128), nbg=2, chunks=">2", down_sk=0, **EXACT)
_sweep("fp32", {"split_nbg2_rows": 99}, (17,), nbg=1, chunks=2, **SPD)      # head / tail operands on two and three 16-row chunks
_sweep("fp32", {"split_nbg2_rows": 99}, (33,), nbg=1, chunks=">2", **SPD)
_sweep("fp32", {"down_splitk_rows": 0}, (9,), nbg=1, chunks=1, **dict(SPD, down_sk=0))

_sweep("fp16", {}, (1, 2), persist=1, valu=0, fuse_heads=1, form_logits=1, form_parts=0, form_xh=0, S=">2")
_sweep("fp16", {}, (5,), persist=1, valu=0, fuse_heads=0, form_logits=0, form_parts=0, form_xh=0, S=1)
SLICES16 = dict(SLICES, valu=0, form_valu=0)
_sweep("fp16", {}, (6,), S=1, **SLICES16)                                   # the first row count of the launch chain
XH16 = dict(CHAIN, S=1, valu=0, splitd=0, xhm=1, spd=0, form_parts=0, form_xh=1, form_split=0)      # (fp16 engines: 8-wave attention blocks at every row count)
_sweep("fp16", {}, (9, 16), nbg=1, chunks=1, down_sk=1, pf_kb=0, **XH16)    # the first packed-residual band: EPI_RESID_XH_SK on one chunk, no prefetch workgroups
_sweep("fp16", {}, (33, 56), nbg=1, chunks=">2", down_sk=1, pf_kb=">0", **XH16)
_sweep("fp16", {}, (57, 64), nbg=2, chunks=2, down_sk=0, pf_kb=">0", form_nbg=2, attn_wave8=1, **XH16)      # 57: the switch to 32-row blocks, tail block of 25 rows
_sweep("fp16", {}, (65, 128), nbg=2, chunks=">2", down_sk=0, pf_kb=">0", form_nbg=2, attn_wave8=1, **XH16)
_sweep("fp16", {"persistent_rows": 0}, (1, 2), S=">2", **SLICES16)
_sweep("fp16", {"persistent_rows": 0}, (4,), S=1, **SLICES16)
_sweep("fp16", {"persistent_rows": 0, "split_rows": 0}, (4,), nbg=1, chunks=1, down_sk=0, pf_kb=0, **XH16)
_sweep("fp16", {"attn_wide_blocks": 1}, (9,), nbg=1, chunks=1, down_sk=1, pf_kb=0, wide_blocks=1, attn_wave8=0, **XH16)      # the 4-wave attention blocks
_sweep("fp16", {"attn_wide_blocks": 1}, (57,), nbg=2, chunks=2, down_sk=0, pf_kb=">0", wide_blocks=1, attn_wave8=0, **XH16)
_sweep("fp16", {"down_splitk_rows": 0}, (9,), nbg=1, chunks=1, down_sk=0, pf_kb=0, **XH16)

# context edges: the attention loops advance 128 keys per iteration on 4-wave blocks and 256 on 8-wave blocks; the rows cross those edges during the forced steps
L130 = (1, 2, 7, 8, 9, 63, 64, 65, 125, 126, 127, 128, 130)
L258 = L130 + (253, 254, 255, 256)
L772 = (772, 771, 769, 766, 1)
# the packed residual stream on either dtype: head / tail fp16 pairs on fp32 engines, fp16 rows on fp16 engines
XH = dict({k: v for k, v in XH16.items() if k not in ("spd", "form_split")}, fp32_spd=1, fp16_spd=0, fp32_form_split=1, fp16_form_split=0)
_ctx(("fp32", "fp16"), {}, 130, L130, nbg=1, chunks=1, down_sk=1, attn_wave8=1, fp32_pf_kb=">0", fp16_pf_kb=0, **XH)
_ctx(("fp32", "fp16"), {"attn_wide_blocks": 1}, 130, L130, wide_blocks=1, attn_wave8=0, nbg=1, chunks=1, down_sk=1, **XH)
_ctx(("fp32", "fp16"), {}, 258, L258, fp32_nbg=2, fp32_chunks=1, fp16_nbg=1, fp16_chunks=2, down_sk=1, pf_kb=">0", attn_wave8=1, **XH)
# > 768 keys at 5 rows on the launch chain (fp16 engines too: their only S = 2 case): two key splits -> the softmax-combine prologue (PRO_ATTN) feeding the fp32 residual epilogue with partials
_ctx(("fp32", "fp16"), {"persistent_rows": 0}, 772, L772, **dict(SLICES16, S=2))
_ctx(("fp32",), {}, 772, L772, persist=1, fuse_heads=0, form_logits=0)
# S = its cap (8) at 2 rows: the 3-key row leaves most of its shares empty
_ctx(("fp32", "fp16"), {"persistent_rows": 0}, 772, (772, 3), S=">2", fp32_valu=1, fp16_valu=0, fp32_form_valu=1, fp16_form_valu=0, **{k: v for k, v in SLICES16.items() if k not in ("valu", "form_valu")})
# ... and the same rows on the persistent launch: two key shares per (row, head) (the only cases with persist > 1)
_ctx(("fp32", "fp16"), {}, 772, (772, 3), persist=">1", fuse_heads=1, form_logits=1)

# the KV cache filled to max_seq: T = 40 and the largest max_new_token that begin accepts on a 64-position cache, on every KV lane (9 rows), 3 rows and 1 row
FULL_T, FULL_N = 40, ENGINES["full"][1] - 40
_ctx(("fp32", "fp16"), {}, FULL_T, (40, 37, 1, 40, 22, 8, 40, 39, 40), engine="full", N=FULL_N, nbg=1, chunks=1, down_sk=1, **XH)
_ctx(("fp32", "fp16"), {}, FULL_T, (40, 1, 33), engine="full", N=FULL_N, persist=1, fuse_heads=0)
_ctx(("fp32", "fp16"), {}, FULL_T, (40,), engine="full", N=FULL_N, persist=1, fuse_heads=1, form_logits=1)


def case_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts.items()) or "default"
    return f"{c.wd}-{c.engine}-B{c.B}-T{c.T}-{o}"


# ---- engines, oracle, driver ----------------------------------------------------------------------------------------------------------------------------
_sd_cache, _oracle, _engines, _refs = [], [], {}, {}


def state_dict():
    if not _sd_cache:
        _sd_cache.append(synth.gpt_state_dict(synth.GPT_REAL, 1234))
        _oracle.append(ref_cpu.OracleGPT(_sd_cache[0], 12))
    return _sd_cache[0]


def engine(kind, wd):
    """One engine per (kind, dtype) for the whole module.  graph_steps 1: a decode call of one step with use_graph set really replays a captured graph."""
    from chatttsplus_amd.hip_models import GPT
    if (kind, wd) not in _engines:
        mb, ms = ENGINES[kind]
        g = GPT(LLAMA, max_batch=mb, max_seq_len=ms, weight_dtype=wd, options={"graph_steps": 1})
        g.load_state_dict(state_dict())
        _engines[(kind, wd)] = g
    return _engines[(kind, wd)]


def close_engines():
    for g in _engines.values():
        g.close()
    _engines.clear()


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    close_engines()
    _refs.clear()


def reference(B, T, pads, N):
    """The free-running oracle (SeededNoise, logits traced) for one shape, computed once and never modified."""
    key = (B, T, tuple(pads), N)
    if key not in _refs:
        state_dict()
        ids, mask = synth.prompt_ids(B, T, synth.GPT_REAL["num_text_tokens"], 300 + B, pad_left=list(pads))
        o = _oracle[0]
        emb = o.embed(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
        ref = o.generate(emb, torch.from_numpy(ids), ref_cpu.SamplerParams(min_new_token=N), attention_mask=torch.from_numpy(mask),
                         max_new_token=N, noise=ref_cpu.SeededNoise(5), trace_logits=True)
        assert ref.steps == N and len(ref.logits_trace) == N and all(int(h.shape[0]) == N for h in ref.hiddens)
        _refs[key] = (mask, emb, ref)
    return _refs[key]


def begin(g, B, T, mask, max_new, out_ids, hid, fin, end, st):
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, max_new, max_new, LW, LP, 4)
    io = _lib.GenIO(ids=out_ids.data_ptr(), hiddens=hid.data_ptr(), finish=fin.data_ptr(), end_idx=end.data_ptr(), noise=None, n_draws=0, seed=1)
    _lib.check(g._lib.ctts_gpt_begin(g._h, B, T, mask.data_ptr(), C.byref(sc), C.byref(io), st), "begin")


def run_case(c):
    """Runs one case: the oracle's ids forced into the engine step by step, decode calls alternating graph replay and eager launches.  Returns what was
    measured (nothing is asserted here): the plans read after every decode call, per-row hidden errors, per-step logit errors, the saturation count."""
    from chatttsplus_amd import _lib
    g = engine(c.engine, c.wd)
    mask, emb, ref = reference(c.B, c.T, c.pads, c.N)
    B, T, N = c.B, c.T, c.N
    lib, h, dev = g._lib, g._h, g.device
    saved = {k: g.get_option(k) for k in c.opts}
    try:
        for k, v in c.opts.items():
            g.set_option(k, v)
        forced = torch.stack([r for r in ref.ids], 0).to(torch.int32).to(dev)          # [B,N,4]
        out_ids = torch.zeros(B, N, 4, dtype=torch.int32, device=dev)
        hid = torch.zeros(B, N, 768, dtype=torch.float32, device=dev)
        fin = torch.zeros(B, dtype=torch.int32, device=dev); end = torch.zeros(B, dtype=torch.int32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        msk = torch.from_numpy(mask).to(dev).to(torch.int32)
        embd = emb.to(dev).contiguous()
        begin(g, B, T, msk, N, out_ids, hid, fin, end, st)
        _lib.check(lib.ctts_gpt_prefill(h, embd.data_ptr(), st), "prefill")
        _lib.check(lib.ctts_gpt_sample(h, st), "sample")
        logits, plans = [g.last_logits(B).cpu().reshape(B * 4, -1)], []
        for i in range(1, N):
            f = forced[:, i - 1].contiguous()
            _lib.check(lib.ctts_gpt_force_ids(h, f.data_ptr(), st), "force")
            _lib.check(lib.ctts_gpt_decode(h, 1, i % 2, st), "decode")           # odd calls replay a hipGraph, even calls launch eagerly
            logits.append(g.last_logits(B).cpu().reshape(B * 4, -1))
            plans.append(g.decode_plan())
        torch.cuda.synchronize()
        steps, alld, nsat = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(lib.ctts_gpt_progress(h, C.byref(steps), C.byref(alld), st), "progress")
        _lib.check(lib.ctts_gpt_saturations(h, C.byref(nsat), st), "saturations")
        hid = hid.cpu()
    finally:
        for k, v in saved.items():
            g.set_option(k, v)
    scale = max(float(torch.stack(ref.hiddens).abs().max()), 1.0)
    rows = []
    for b in range(B):
        d = hid[b] - ref.hiddens[b]
        rows.append((float(d.pow(2).mean().sqrt()) / float(ref.hiddens[b].pow(2).mean().sqrt()), float(d.abs().max())))
    lerr = [(float((logits[i] - ref.logits_trace[i]).abs().max()), max(float(ref.logits_trace[i].abs().max()), 1.0)) for i in range(N)]
    return dict(plans=plans, steps=int(steps.value), rows=rows, scale=scale, logits=lerr, saturations=int(nsat.value))


def plan_mismatches(plan, expect):
    # attn_wave8: the unsplit decode attention of the launch chain takes 8-wave blocks (256 keys per loop iteration) while rows x heads < wide_blocks, else 4-wave
    # blocks (128 keys); derived here from the plan's fields the way launch_attention (attention.hip) decides it
    plan = dict(plan, attn_wave8=int(plan["persist"] == 0 and plan["S"] == 1 and plan["B"] * LLAMA["num_attention_heads"] < (plan["wide_blocks"] or 256)))
    bad = []
    for k, want in expect.items():
        got = plan[k]
        ok = got > int(want[1:]) if isinstance(want, str) else got == want
        if not ok:
            bad.append(f"{k}: planned {got}, the case was written for {want}")
    return bad


def check_case(c, m):
    """(a) the plan, (b) every step's hidden row, (c) every step's logits, (d) no saturated fp16 store"""
    tol = TOL[c.wd]
    assert m["steps"] == c.N and len(m["plans"]) == c.N - 1
    for p in m["plans"]:
        assert p["B"] == c.B
        bad = plan_mismatches(p, c.expect)
        assert not bad, f"{case_id(c)} no longer runs the plan it was written for -- " + "; ".join(bad) + f" (plan {p})"
    worst = max(range(c.B), key=lambda b: m["rows"][b][0])
    print(f"{case_id(c)}: worst rms-rel {m['rows'][worst][0]:.3e} (row {worst}), worst max abs {max(r[1] for r in m['rows']):.3e} of {4 * tol * m['scale']:.3e}, "
          f"worst logit err / bound {max(e / (4 * tol * s) for e, s in m['logits']):.3f}")
    for b, (rms, mx) in enumerate(m["rows"]):
        assert mx <= tol * m["scale"] * 4 and rms <= tol, f"row {b} (pad {c.pads[b]}): max {mx} rms-rel {rms}"
    for i, (e, s) in enumerate(m["logits"]):
        assert e <= tol * 4 * s, f"step {i}: logits max abs err {e} > {tol * 4 * s}"
    assert m["saturations"] == 0


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_decode_plan_vs_oracle(c):
    check_case(c, run_case(c))


@pytest.mark.parametrize("wd", ["fp32", "fp16"])
def test_one_token_beyond_the_cache_is_refused(wd):
    """T + max_new_token = max_seq + 1: begin refuses (the full-cache cases above run T + max_new_token = max_seq on the same engine)."""
    from chatttsplus_amd import _lib
    g = engine("full", wd)
    B, T, N = 9, FULL_T, FULL_N + 1
    dev = g.device
    out_ids = torch.zeros(B, N, 4, dtype=torch.int32, device=dev)
    hid = torch.zeros(B, N, 768, dtype=torch.float32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev); end = torch.zeros(B, dtype=torch.int32, device=dev)
    msk = torch.ones(B, T, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.HipBackendError, match="max_seq"):
        begin(g, B, T, msk, N, out_ids, hid, fin, end, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


@pytest.mark.parametrize("wd", ["fp32", "fp16"])
def test_decode_plan_needs_a_planned_decode_call(wd):
    """Between begin and the first decode call of a batch there is no plan to read: an error, not the previous batch's plan."""
    from chatttsplus_amd import _lib
    g = engine("full", wd)
    B, T, N = 2, 6, 4
    dev = g.device
    out_ids = torch.zeros(B, N, 4, dtype=torch.int32, device=dev)
    hid = torch.zeros(B, N, 768, dtype=torch.float32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev); end = torch.zeros(B, dtype=torch.int32, device=dev)
    msk = torch.ones(B, T, dtype=torch.int32, device=dev)
    begin(g, B, T, msk, N, out_ids, hid, fin, end, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    with pytest.raises(_lib.HipBackendError, match="no decode call"):
        g.decode_plan()
    torch.cuda.synchronize()


# every value a decode plan feature can take, per dtype (fp16 engines have neither VALU products nor head / tail operands)
FEATURES = {
    "persist": (0, 1, ">1"), "S": (1, 2, ">2"), "nbg": (1, 2), "chunks": (1, 2, ">2"), "pf_kb": (0, ">0"),
    "splitd": (0, 1), "xhm": (0, 1), "attn_wave8": (0, 1), "down_sk": (0, 1), "fuse_heads": (0, 1), "valu": {"fp32": (0, 1), "fp16": (0,)}, "spd": {"fp32": (0, 1), "fp16": (0,)},
}


def test_cases_cover_every_plan_feature():
    """The union of what the cases pin covers every value of every decode plan feature, per dtype: a feature added to the plan (and to FEATURES) without a
    case, or a case dropped, fails here.  No GPU work."""
    from chatttsplus_amd.hip_models.gpt import GPT
    others = {"B", "splits", "dts", "wide_blocks", "prepack", "lora", "form_parts", "form_xh", "form_logits", "form_split", "form_nbg", "form_valu"}
    assert (set(FEATURES) - {"attn_wave8"}) | others == set(GPT.DECODE_PLAN_FIELDS), "a plan field is neither a feature with cases nor listed as not one"
    missing = []
    for wd in ("fp32", "fp16"):
        pinned = {}
        for c in CASES:
            if c.wd == wd:
                for k, v in c.expect.items():
                    pinned.setdefault(k, set()).add(v)
        for f, values in FEATURES.items():
            for v in (values[wd] if isinstance(values, dict) else values):
                if v not in pinned.get(f, ()):
                    missing.append(f"{wd}: no case pins {f} = {v}")
    assert not missing, missing
    assert len({(case_id(c)) for c in CASES}) == len(CASES)
