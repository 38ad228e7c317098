"""Every prompt-pass launch plan against the CPU oracle: every real prompt row, every KV slot.

plan_layers (gpt_engine.hip) picks the prompt pass's kernels by the pass height, split_gemm_shape (prefill_split.hip) picks a block shape per projection,
prefill_gemm_shape (prefill_gemm.hip) and prompt_attention_kind (attention.hip) pick the rest, and pass_rows cuts the flattened [B][T] prompt into passes.  Each
case below names the plan it was written for (GPT.prompt_plan(), read back from the engine after the prefill call) and then pins what that plan computes to the
oracle: K after RoPE and V of every layer at every real prompt slot of every lane, and the residual rows the last pass left (the last layer's MLP output, interior
rows included).  A moved threshold fails a case on its plan assertion -- it does not silently move the case to another kernel -- and
test_cases_cover_every_prompt_plan_feature fails when a plan feature has no case at all.

Per case: the KV cache is filled with a sentinel byte, begin + prefill run through the ABI, then (a) the plan, (b) the RowMeta of every real prompt row straight
from the mask, (c) K and V, (d) the last pass's residual rows, (e) the sentinel wherever the call must not write (slots at or beyond the prompt end, lanes the
call does not name), (f) no saturated fp16 store.  Pad rows are the only thing left out.  The invariant engines run the last token through the first decode
step: ctts_gpt_sample runs as well, slot T - 1 and the decode row's logits are compared too.

Tolerances are the project's (tests/test_gpu_gpt.py), per lane for each of K, V (per layer) and the residual rows: rms-rel <= tol and
max abs <= 4 tol max(|ref|max, 1) with tol = 2e-5 (fp32 engines) / 2e-3 (fp16 engines: weights and KV rounded to fp16, fp32 accumulate; the oracle's own K
rounded to fp16 sits 2.1e-4 rms-rel from itself).  |ref|max is taken over the real slots of the quantity and layer (over the real rows for the residual).

Synthetic weights at real widths, 4 decoder layers (no prompt-plan decision depends on the layer count).  The oracle result of a shape is computed once (module
cache keyed by (B, T, pads)) and shared by the dtype and option variants of that shape.  tools/prompt_plan_oracle.py runs the same cases through the same driver
and records the figures (profiles/prompt_plan_oracle.jsonl)."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from chatttsplus_amd import synth
from oracle import ref_cpu

gpu = pytest.mark.gpu

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
CFG4 = dict(synth.GPT_REAL, num_hidden_layers=4)
LLAMA4 = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=4)
SEED = 4321
L, NH, HD, H = 4, 12, 64, 768
TOL = {"fp32": 2e-5, "fp16": 2e-3}
SENTINEL = 0xA5                  # a finite value in either cache dtype
MAX_NEW = 2
# engines: (max_batch, max_seq_len).  "wide" serves the row-count sweep (its KV cache: 226 MB in fp32), "long" the two prime-ish row counts, "mid" the passes of 256 rows
# and the invariant engines
ENGINES = {"wide": (17, 520), "long": (3, 700), "mid": (5, 170)}
CREATION_OPTIONS = ("batch_invariant", "schedule_invariant")      # part of the engine's identity; every other option is set for the case and restored

Case = namedtuple("Case", "wd engine opts pass_rows B T pads expect")

# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
# `expect` pins prompt_plan() fields: an int is an exact value, ">1" a lower bound, a name an attention / GEMM kind (GPT.PROMPT_ATTN_KINDS / PROMPT_GEMM_KINDS).
# Unprefixed fields describe a full pass, last_* the last pass; a call of one pass must report the same plan twice (check_case).  The values follow plan_layers and
# split_gemm_shape with the engines' defaults: prefill_split_rows 65, prefill_small_blocks 192, prefill_ring4_blocks 256, prefill_splitk_rows 2048,
# prefill_pp_blocks 1 (round counts 36 per 512 blocks of 128 x 128, 45 / 60 per 256 counter-phased blocks NT 3 / 4), prefill_gemm from 1536 rows, 256 x 128 gate|up from 8192.
CASES = []


def ragged(B, T, k, m):
    """pads (k i) % m, the last row of a batch left with a single real key"""
    assert m <= T
    p = [(k * i) % m for i in range(B)]
    if B > 1:
        p[-1] = T - 1
    return tuple(p)


def gemms(qkv, o, gu, down, down_sliced=0, pre=""):
    return {pre + "qkv": qkv, pre + "o": o, pre + "gu": gu, pre + "down": down, pre + "qkv_sliced": 0, pre + "o_sliced": 0, pre + "gu_sliced": 0, pre + "down_sliced": down_sliced}


def _case(wds, B, T, pads, expect, opts=None, engine="wide", pass_rows=None):
    assert len(pads) == B and all(0 <= p < T for p in pads)
    for wd in wds:
        CASES.append(Case(wd, engine, dict(opts or {}), pass_rows, B, T, tuple(pads), dict(expect)))


# the decode kernels' prompt pass: one weight tile per 16 * nbg-row block, RMSNorm in the block up to 64 rows, the row attention
TILE = dict(passes=1, prepack=0, pfg=0, pfs=0, anchor=0, **gemms("tile_norm", "tile_packed", "tile_norm", "tile_packed"))
# ... on the rows normalised once (norm_pack) above 64 rows
PACKED = dict(passes=1, nbg=2, prepack=1, pfg=0, pfs=0, anchor=0, **gemms("tile_packed", "tile_packed", "tile_packed", "tile_packed"))
# fp32 engines from prefill_split_rows = 65 rows: head / tail fp16 operands, the split attention kernel
SPLIT = dict(passes=1, nbg=2, prepack=1, pfg=0, pfs=1, anchor=0, attn="split")
# fp16 engines from 1536 rows: the LDS-staged GEMM of prefill_gemm.hip
PFG = dict(passes=1, nbg=2, prepack=1, pfg=1, pfs=0, anchor=0, attn="mfma")
BOTH = ("fp32", "fp16")

# ---- default engines, one pass
_case(BOTH, 1, 1, (0,), dict(TILE, nbg=1, attn="row", rows_full=1, pre_T=1))
_case(BOTH, 2, 8, ragged(2, 8, 3, 5), dict(TILE, nbg=1, attn="row", rows_full=16))                       # nbg: 1 up to 16 rows ...
_case(BOTH, 1, 17, (5,), dict(TILE, nbg=2, attn="row", rows_full=17))                                    # ... 2 above
_case(("fp16",), 1, 63, (20,), dict(TILE, nbg=2, attn="row", rows_full=63))                              # fp16: the row attention up to 63 rows ...
_case(("fp32",), 1, 64, (9,), dict(TILE, nbg=2, attn="row", rows_full=64))                               # fp32: pfs off at 64 rows
_case(("fp16",), 1, 64, (9,), dict(TILE, nbg=2, attn="mfma", rows_full=64))                              # ... the MFMA flash attention from 64, still without prepack
_case(("fp16",), 4, 16, ragged(4, 16, 5, 11), dict(TILE, nbg=2, attn="mfma", rows_full=64))              #     (four sequences in one 64-query block column each)
S64 = gemms("split64", "split64", "split64", "split64", 1)
_case(("fp32",), 1, 65, (0,), dict(SPLIT, rows_full=65, **S64))                                          # pfs on at 65 rows; 65 keys: a second 64-key chunk of one key
_case(("fp32",), 5, 13, ragged(5, 13, 3, 7), dict(SPLIT, rows_full=65, **S64))
_case(("fp16",), 1, 65, (0,), dict(PACKED, attn="mfma", rows_full=65))                                   # fp16: prepack on at 65 rows
_case(("fp16",), 5, 13, ragged(5, 13, 3, 7), dict(PACKED, attn="mfma", rows_full=65))
_case(("fp32",), 3, 43, ragged(3, 43, 7, 19), dict(SPLIT, rows_full=129, **S64))                         # 129 rows: a 1-row tail block
_case(("fp32",), 1, 129, (70,), dict(SPLIT, rows_full=129, **S64))                                       #   T = 129, the first real key mid-chunk (slot 70)
_case(("fp16",), 3, 43, ragged(3, 43, 7, 19), dict(PACKED, attn="mfma", rows_full=129))
_case(("fp16",), 1, 129, (70,), dict(PACKED, attn="mfma", rows_full=129))
# fp32: the block shapes of the split GEMMs by round-count arithmetic
_case(("fp32",), 8, 64, ragged(8, 64, 11, 29), dict(SPLIT, rows_full=512, **S64))                                                                   # 512 | 513: gate|up 64 x 64 -> ring4
_case(("fp32",), 9, 57, ragged(9, 57, 5, 23), dict(SPLIT, rows_full=513, **gemms("split64", "split64", "ring4", "split64", 1)))
_case(("fp32",), 5, 128, ragged(5, 128, 37, 101), dict(SPLIT, rows_full=640, **gemms("split64", "split64", "ring4", "split64", 1)))                  # 640 | 641: gate|up ring4 -> ring2
_case(("fp32",), 1, 641, (200,), dict(SPLIT, rows_full=641, **gemms("split64", "split64", "ring2", "split64", 1)), engine="long")
_case(("fp32",), 8, 128, ragged(8, 128, 29, 97), dict(SPLIT, rows_full=1024, **gemms("split64", "split64", "ring2", "split64", 1)))                  # 1024 | 1025: sliced down 64 x 64 -> ring4
_case(("fp32",), 5, 205, ragged(5, 205, 67, 131), dict(SPLIT, rows_full=1025, **gemms("split64", "split64", "ring2", "ring4", 1)))
_case(("fp32",), 5, 256, ragged(5, 256, 71, 193), dict(SPLIT, rows_full=1280, **gemms("split64", "split64", "ring2", "ring4", 1)))                   # 1280 | 1281: qkv 64 x 64 -> ring4, sliced down
_case(("fp32",), 3, 427, ragged(3, 427, 130, 300), dict(SPLIT, rows_full=1281, **gemms("ring4", "split64", "pp3", "ring2", 1)))                      #   ring4 -> ring2, gate|up -> counter-phased NT 3
_case(("fp32",), 4, 512, ragged(4, 512, 171, 400), dict(SPLIT, rows_full=2048, **gemms("ring2", "split64", "pp3", "ring2", 1)))                      # 2048 | 2049: down sliced -> unsliced (64 x 64 again),
_case(("fp32",), 3, 683, ragged(3, 683, 250, 600), dict(SPLIT, rows_full=2049, **gemms("ring2", "split64", "pp4", "split64", 0)), engine="long")     #   gate|up NT 3 -> NT 4
_case(("fp32",), 16, 256, ragged(16, 256, 37, 129), dict(SPLIT, rows_full=4096, **gemms("pp3", "split64", "pp3", "split64", 0)))                     # 4096 | 4097: o_proj and down leave 64 x 64
_case(("fp32",), 17, 241, ragged(17, 241, 31, 127), dict(SPLIT, rows_full=4097, **gemms("pp3", "ring4", "pp4", "ring4", 0)))
# fp32 with options
_case(("fp32",), 3, 127, ragged(3, 127, 40, 90), dict(SPLIT, rows_full=381, **gemms("pp4", "pp4", "pp4", "pp4", 0)), opts={"prefill_pp_blocks": -4})      # a partial 256-row block
_case(("fp32",), 3, 127, ragged(3, 127, 40, 90), dict(SPLIT, rows_full=381, **gemms("pp3", "pp3", "pp3", "pp3", 0)), opts={"prefill_pp_blocks": -3})
_case(("fp32",), 3, 43, ragged(3, 43, 7, 19), dict(SPLIT, rows_full=129, **gemms("ring2", "ring2", "ring2", "ring2", 1)),                                 # the 2-stage ring the bitwise tests anchor on
      opts={"prefill_small_blocks": 0, "prefill_ring4_blocks": 0})
_case(("fp32",), 3, 127, ragged(3, 127, 40, 90), dict(SPLIT, rows_full=381, **gemms("split64", "split64", "split64", "split64", 0)), opts={"prefill_splitk_rows": 0})
_case(("fp32",), 5, 13, ragged(5, 13, 3, 7), dict(PACKED, attn="row", rows_full=65), opts={"prefill_split_rows": 0})                                     # the exact-f32 packed path (what a checkpoint
_case(("fp32",), 3, 43, ragged(3, 43, 7, 19), dict(PACKED, attn="row", rows_full=129), opts={"prefill_split_rows": 0})                                   #   beyond the fp16 range falls back to)
# fp16: prefill_gemm from 1536 rows, gate|up on 256 x 128 from 8192
_case(("fp16",), 5, 307, ragged(5, 307, 97, 211), dict(PACKED, attn="mfma", rows_full=1535))
_case(("fp16",), 6, 256, ragged(6, 256, 71, 193), dict(PFG, rows_full=1536, **gemms("pfg0", "pfg0", "pfg0", "pfg0")))
_case(("fp16",), 17, 481, ragged(17, 481, 53, 311), dict(PFG, rows_full=8177, **gemms("pfg0", "pfg0", "pfg0", "pfg0")))      # (8191 is prime: the largest B x T below 8192 the engine holds)
_case(("fp16",), 16, 512, ragged(16, 512, 171, 400), dict(PFG, rows_full=8192, **gemms("pfg0", "pfg0", "pfg1", "pfg0")))
# ---- several passes (CTTS_PASS_ROWS 256): sequences straddle the boundaries, a pass starts mid-sequence and attends to keys an earlier pass wrote, the last pass is shorter
# (the single-key sequence sits second, so that the last pass holds real rows of a sequence that began in the pass before)
P3 = dict(passes=">1", rows_full=256)


def _pads4(T):
    return (37, T - 1, 74, 11)


_case(("fp32",), 4, 143, _pads4(143), dict(P3, rows_last=60, pfs=1, attn="split", prepack=1, **S64, last_pfs=0, last_prepack=0, last_attn="row", last_nbg=2,
                                                         **gemms("tile_norm", "tile_packed", "tile_norm", "tile_packed", pre="last_")), engine="mid", pass_rows=256)
_case(("fp32",), 4, 160, _pads4(160), dict(P3, rows_last=128, pfs=1, attn="split", **S64, last_pfs=1, last_attn="split", **gemms("split64", "split64", "split64", "split64", 1, pre="last_")),
      engine="mid", pass_rows=256)
_case(("fp16",), 4, 143, _pads4(143), dict(P3, rows_last=60, pfg=0, attn="mfma", prepack=1, **gemms("tile_packed", "tile_packed", "tile_packed", "tile_packed"), last_prepack=0, last_attn="row",
                                                         **gemms("tile_norm", "tile_packed", "tile_norm", "tile_packed", pre="last_")), engine="mid", pass_rows=256)
_case(("fp16",), 4, 160, _pads4(160), dict(P3, rows_last=128, attn="mfma", prepack=1, last_prepack=1, last_attn="mfma", **gemms("tile_packed", "tile_packed", "tile_packed", "tile_packed", pre="last_")),
      engine="mid", pass_rows=256)
# ---- invariant engines: T - 1 prompt rows per sequence, the last token through the first decode step
# fp32 batch_invariant: the split GEMMs at every pass height, the down projection's K never sliced
INV32 = dict(passes=1, pfs=1, pfg=0, anchor=1, attn="split", **gemms("split64", "split64", "split64", "split64", 0))
_case(("fp32",), 1, 2, (0,), dict(INV32, nbg=1, prepack=0, rows_full=1, pre_T=1), opts={"batch_invariant": 1}, engine="mid")
_case(("fp32",), 1, 18, (4,), dict(INV32, nbg=2, prepack=0, rows_full=17, pre_T=17), opts={"batch_invariant": 1}, engine="mid")
_case(("fp32",), 5, 14, ragged(5, 14, 3, 7), dict(INV32, nbg=2, prepack=1, rows_full=65, pre_T=13), opts={"batch_invariant": 1}, engine="mid")
# fp16 schedule_invariant: prefill_gemm shape 0 and the anchored MFMA attention at every pass height
INV16 = dict(nbg=2, prepack=1, pfs=0, pfg=1, anchor=1, attn="mfma_anchor", **gemms("pfg0", "pfg0", "pfg0", "pfg0"))
_case(("fp16",), 1, 2, (0,), dict(INV16, passes=1, rows_full=1, pre_T=1), opts={"schedule_invariant": 1}, engine="mid")
_case(("fp16",), 3, 22, ragged(3, 22, 5, 13), dict(INV16, passes=1, rows_full=63), opts={"schedule_invariant": 1}, engine="mid")
_case(("fp16",), 4, 17, ragged(4, 17, 5, 11), dict(INV16, passes=1, rows_full=64), opts={"schedule_invariant": 1}, engine="mid")
_case(("fp16",), 4, 76, ragged(4, 76, 23, 61), dict(INV16, passes=1, rows_full=300, pre_T=75), opts={"schedule_invariant": 1}, engine="mid")
_case(("fp16",), 4, 144, _pads4(144), dict(INV16, passes=">1", rows_full=256, rows_last=60, last_pfg=1, last_attn="mfma_anchor", **gemms("pfg0", "pfg0", "pfg0", "pfg0", pre="last_")),
      opts={"schedule_invariant": 1}, engine="mid", pass_rows=256)


def case_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts.items()) or "default"
    return f"{c.wd}-{c.engine}{'-p' + str(c.pass_rows) if c.pass_rows else ''}-B{c.B}-T{c.T}-{o}"


def invariant(c):
    return any(c.opts.get(k) for k in CREATION_OPTIONS)


# ---- engines, oracle, driver ----------------------------------------------------------------------------------------------------------------------------
_sd_cache, _oracle, _engines, _refs = [], [], {}, {}
BIG_ROWS = 2100          # oracle results above this many rows (200 MB of K / V at 8192) are not kept beyond the next such shape


def state_dict():
    if not _sd_cache:
        _sd_cache.append(synth.gpt_state_dict(CFG4, SEED))
        _oracle.append(ref_cpu.OracleGPT(_sd_cache[0], NH))
    return _sd_cache[0]


def engine(c):
    """One engine per (kind, dtype, options at creation, pass_rows) for the whole module."""
    from chatttsplus_amd.hip_models import GPT
    created = {k: v for k, v in c.opts.items() if k in CREATION_OPTIONS}
    key = (c.engine, c.wd, tuple(sorted(created.items())), c.pass_rows)
    if key not in _engines:
        mb, ms = ENGINES[c.engine]
        if c.pass_rows:
            os.environ["CTTS_PASS_ROWS"] = str(c.pass_rows)      # read once at finalize (as tests/test_gpu_score.py sets it)
        try:
            g = GPT(LLAMA4, max_batch=mb, max_seq_len=ms, weight_dtype=c.wd, options=created)
            g.load_state_dict(state_dict())
        finally:
            os.environ.pop("CTTS_PASS_ROWS", None)
        _engines[key] = g
    return _engines[key]


def close_engines():
    for g in _engines.values():
        g.close()
    _engines.clear()


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    close_engines()
    _refs.clear()


def reference(B, T, pads):
    """The oracle's forward over the whole prompt of one shape, computed once and never modified: mask, embeddings, K / V [L][B][NH][T][64], the residual rows
    before the final norm [B][T][H], the code logits of the last row [B * 4][V]."""
    key = (B, T, tuple(pads))
    if key not in _refs:
        state_dict()
        if B * T > BIG_ROWS:
            for k in [k for k in _refs if k[0] * k[1] > BIG_ROWS]:
                del _refs[k]
        ids, mask = synth.prompt_ids(B, T, CFG4["num_text_tokens"], 700 + B + T, pad_left=list(pads))
        o = _oracle[0]
        m = torch.from_numpy(mask)
        emb = o.embed(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
        pos = (m.cumsum(1) - 1).masked_fill(m == 0, 1)
        o.alloc_cache(B, T)
        with torch.no_grad():
            hid = o.forward(emb, m, pos)
            logits = o.code_logits(hid[:, -1])
        _refs[key] = dict(mask=mask, emb=emb, kc=o.kc, vc=o.vc, resid=o.last_residual, logits=logits)
        o.kc = o.vc = o.last_residual = None
    return _refs[key]


def begin(g, B, T, mask, st, bufs):
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models.gpt import sampler_cfg_from_objects
    dev = g.device
    bufs["ids"] = torch.zeros(B, MAX_NEW, 4, dtype=torch.int32, device=dev)
    bufs["hid"] = torch.zeros(B, MAX_NEW, H, dtype=torch.float32, device=dev)
    bufs["fin"] = torch.zeros(B, dtype=torch.int32, device=dev); bufs["end"] = torch.zeros(B, dtype=torch.int32, device=dev)
    sc = sampler_cfg_from_objects(torch.tensor([0.3] * 4), 625, MAX_NEW, MAX_NEW, LW, LP, 4)
    io = _lib.GenIO(ids=bufs["ids"].data_ptr(), hiddens=bufs["hid"].data_ptr(), finish=bufs["fin"].data_ptr(), end_idx=bufs["end"].data_ptr(), noise=None, n_draws=0, seed=1)
    _lib.check(g._lib.ctts_gpt_begin(g._h, B, T, mask.data_ptr(), C.byref(sc), C.byref(io), st), "begin")


def debug_read(g, name, arr, st):
    from chatttsplus_amd import _lib
    nb = C.c_size_t(0)
    _lib.check(g._lib.ctts_gpt_debug_read(g._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes, C.byref(nb), st), f"debug_read({name})")
    assert nb.value == arr.nbytes, f"debug_read({name}): {nb.value} bytes for a buffer of {arr.nbytes}"
    return arr


def named_plan(plan):
    """prompt_plan() with the attention / GEMM kinds by name"""
    from chatttsplus_amd.hip_models.gpt import GPT
    p = dict(plan)
    for pre in ("", "last_"):
        p[pre + "attn"] = GPT.PROMPT_ATTN_KINDS[p[pre + "attn"]]
        for k in ("qkv", "o", "gu", "down"):
            p[pre + k] = GPT.PROMPT_GEMM_KINDS[p[pre + k]]
    return p


def kv_views(g, esz):
    """the caller's KV tensor as [layer][k | v][lane][head][slot][64] elements, and as bytes [..][slot][64 * esz]"""
    mb, ms = g.max_batch, g.max_seq
    n = L * 2 * mb * NH * ms * HD * esz
    return g._kv[:n].view(torch.float16 if esz == 2 else torch.float32).view(L, 2, mb, NH, ms, HD), g._kv[:n].view(L, 2, mb, NH, ms, HD * esz)


def lane_errors(got, ref, real):
    """got, ref [B][...][T][..] with the slot axis at 2 (K / V: [B][NH][T][64]) or [B][1][T][H]; real [B][T].  Per lane over its real slots: rms-rel, max abs and the
    slot of the max; and |ref|max over all real slots.  Everything outside `real` is left out (the engine's pad slots hold the pad rows' K / V)."""
    m = real[:, None, :, None]
    zero = torch.zeros((), device=got.device)
    d = torch.where(m, got.float() - ref, zero)
    r = torch.where(m, ref, zero)
    rms = (d.double().pow(2).sum((1, 2, 3)) / r.double().pow(2).sum((1, 2, 3)).clamp_min(1e-300)).sqrt()
    per_slot = d.abs().amax((1, 3))                       # [B][T]
    mx, slot = per_slot.max(1)
    return rms.cpu(), mx.cpu(), slot.cpu(), float(r.abs().max())


def run_case(c):
    """Runs one case: sentinel, begin + prefill (+ sample on the invariant engines), the reads.  Returns what was measured (nothing is asserted here)."""
    from chatttsplus_amd import _lib
    g = engine(c)
    ref = reference(c.B, c.T, c.pads)
    B, T = c.B, c.T
    lib, h, dev = g._lib, g._h, g.device
    inv = invariant(c)
    Tp = T - 1 if inv else T                               # prompt rows per sequence
    run_opts = {k: v for k, v in c.opts.items() if k not in CREATION_OPTIONS}
    saved = {k: g.get_option(k) for k in run_opts}
    m = dict(inv=inv, Tp=Tp)
    try:
        for k, v in run_opts.items():
            g.set_option(k, v)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        msk = torch.from_numpy(ref["mask"]).to(dev).to(torch.int32).contiguous()
        embd = ref["emb"].to(dev).contiguous()
        kv, kvb = kv_views(g, 2 if g.dtype_code == _lib.DTYPE_F16 else 4)
        g._kv.fill_(SENTINEL)
        bufs = {}
        begin(g, B, T, msk, st, bufs)
        _lib.check(lib.ctts_gpt_prefill(h, embd.data_ptr(), st), "prefill")
        m["plan"] = named_plan(g.prompt_plan())
        R = B * Tp
        m["meta"] = debug_read(g, "meta_pre", np.zeros((R, 4), dtype=np.int32), st)
        n_last = m["plan"]["rows_last"]
        x_pre = debug_read(g, "x_pre", np.zeros((n_last, H), dtype=np.float32), st)
        # (e) nothing else written: slots at or beyond the prompt end, lanes the call does not name
        m["stray_bytes"] = int((kvb[:, :, :B, :, Tp:] != SENTINEL).sum()) + int((kvb[:, :, B:] != SENTINEL).sum())
        if inv:
            _lib.check(lib.ctts_gpt_sample(h, st), "sample")
            lg = g.last_logits(B).reshape(B * 4, -1).cpu()
            m["logit_err"] = float((lg - ref["logits"]).abs().max())
            m["logit_scale"] = max(float(ref["logits"].abs().max()), 1.0)
            m["stray_bytes"] += int((kvb[:, :, :B, :, T:] != SENTINEL).sum()) + int((kvb[:, :, B:] != SENTINEL).sum())
        torch.cuda.synchronize()
        nsat = C.c_int32(0)
        _lib.check(lib.ctts_gpt_saturations(h, C.byref(nsat), st), "saturations")
        m["saturations"] = int(nsat.value)
        # (c) K and V of every layer at every real slot [pad_b, T) of every lane (the invariant engines: slot T - 1 is the decode row's), compared on the device
        real = msk.bool()
        for which, name in ((0, "K"), (1, "V")):
            rows = []
            for l in range(L):
                r = (ref["kc"] if which == 0 else ref["vc"])[l].to(dev)
                rows.append(lane_errors(kv[l, which, :B, :, :T], r, real))
            m[name] = dict(rms=torch.stack([x[0] for x in rows]), mx=torch.stack([x[1] for x in rows]), slot=torch.stack([x[2] for x in rows]), scale=[max(x[3], 1.0) for x in rows])
        # (d) the residual rows the last pass left: its real rows against the oracle's, through the RowMeta the engine used
        r0 = R - n_last
        lane = torch.from_numpy(m["meta"][r0:, 0].astype(np.int64)); slot = torch.from_numpy(m["meta"][r0:, 2].astype(np.int64))
        ok = (lane >= 0) & (lane < B) & (slot >= 0) & (slot < T)
        lane, slot = lane.clamp(0, B - 1), slot.clamp(0, T - 1)
        is_real = ok & torch.from_numpy(ref["mask"]).bool()[lane, slot]
        got = torch.zeros(B, 1, T, H); want = torch.zeros(B, 1, T, H); seen = torch.zeros(B, T, dtype=torch.bool)
        got[lane[is_real], 0, slot[is_real]] = torch.from_numpy(x_pre)[is_real]
        want[lane[is_real], 0, slot[is_real]] = ref["resid"][lane[is_real], slot[is_real]]
        seen[lane[is_real], slot[is_real]] = True
        rms, mx, sl, scale = lane_errors(got, want, seen)
        m["X"] = dict(rms=rms[None], mx=mx[None], slot=sl[None], scale=[max(scale, 1.0)], lanes=seen.any(1), rows=int(is_real.sum()))
    finally:
        for k, v in saved.items():
            g.set_option(k, v)
    return m


def plan_mismatches(plan, expect):
    bad = []
    for k, want in expect.items():
        got = plan[k]
        ok = got > int(want[1:]) if isinstance(want, str) and want.startswith(">") else got == want
        if not ok:
            bad.append(f"{k}: planned {got}, the case was written for {want}")
    if plan["passes"] == 1:
        bad += [f"one pass, but last_{k} = {plan['last_' + k]} differs from {k} = {plan[k]}" for k in plan if "last_" + k in plan and plan["last_" + k] != plan[k]]
        if plan["rows_last"] != plan["rows_full"]:
            bad.append(f"one pass of {plan['rows_full']} rows, but rows_last = {plan['rows_last']}")
    return bad


def bounds(c, q, m):
    """(rms-rel bound, max-abs bound per layer) of quantity q"""
    tol = TOL[c.wd]
    return tol, [4 * tol * s for s in m[q]["scale"]]


def worst(c, m):
    """per quantity: the worst rms-rel and the worst max abs as a fraction of its bound, with the layer / lane / slot where they occur (tools/prompt_plan_oracle.py)"""
    real_lanes = torch.from_numpy(np.asarray(c.pads)) < c.T
    out = {}
    for q in ("K", "V", "X"):
        e = m[q]
        lanes = e.get("lanes", real_lanes)
        rms = torch.where(lanes[None], e["rms"], torch.zeros(()).double())
        _, mb = bounds(c, q, m)
        frac = torch.where(lanes[None], e["mx"], torch.zeros(())) / torch.tensor(mb)[:, None]
        i, j = divmod(int(rms.argmax()), rms.shape[1]); k, n = divmod(int(frac.argmax()), frac.shape[1])
        out[q] = dict(rms_rel=float(rms[i, j]), rms_at=dict(layer=i, lane=j), max_abs=float(e["mx"][k, n]), max_abs_bound=mb[k], max_abs_at=dict(layer=k, lane=n, slot=int(e["slot"][k, n])))
    return out


def check_case(c, m):
    """(a) the plan, (b) the row map, (c) K and V, (d) the last pass's residual rows, (e) nothing else written, (f) no saturated fp16 store"""
    B, T, Tp = c.B, c.T, m["Tp"]
    p = m["plan"]
    # (a)
    bad = plan_mismatches(p, c.expect)
    assert not bad, f"{case_id(c)} no longer runs the plan it was written for -- " + "; ".join(bad) + f" (plan {p})"
    R = B * Tp
    passes = (R + p["rows_full"] - 1) // p["rows_full"]
    assert p["passes"] == passes and p["pre_T"] == Tp and p["rows_last"] == R - (passes - 1) * p["rows_full"], f"{case_id(c)}: {R} rows as {p}"
    # (b) straight from the mask: the row of (b, t) sits at b Tp + t, writes lane b slot t, rotates by cumsum(mask) - 1 and attends from its sequence's left pad
    mask = reference(B, T, c.pads)["mask"]
    meta = m["meta"].reshape(B, Tp, 4)
    real = mask[:, :Tp] != 0
    want = np.stack([np.broadcast_to(np.arange(B)[:, None], (B, Tp)), (np.cumsum(mask, 1) - 1)[:, :Tp], np.broadcast_to(np.arange(Tp)[None], (B, Tp)),
                     np.broadcast_to(np.asarray(c.pads)[:, None], (B, Tp))], -1)
    assert np.array_equal(meta[real], want[real]), f"{case_id(c)}: RowMeta {{lane, pos, slot, kv_start}} of a real prompt row differs from the mask's"
    w = worst(c, m)
    print(f"{case_id(c)}: " + "; ".join(f"{q} rms-rel {w[q]['rms_rel']:.3e} max abs {w[q]['max_abs']:.3e} of {w[q]['max_abs_bound']:.3e}" for q in ("K", "V", "X"))
          + (f"; logits {m['logit_err']:.3e} of {4 * TOL[c.wd] * m['logit_scale']:.3e}" if m["inv"] else ""))
    # (c), (d): every lane that has a real slot (every lane has: pads < T), every layer
    assert m["X"]["rows"] == int((mask[:, :Tp] != 0).reshape(-1)[R - p["rows_last"]:].sum()), "a real row of the last pass was not compared"
    for q in ("K", "V", "X"):
        tol, mb = bounds(c, q, m)
        e = m[q]
        for l in range(e["rms"].shape[0]):
            for b in range(B):
                if q == "X" and not bool(e["lanes"][b]):
                    continue                                   # no real row of this lane in the last pass
                rms, mx = float(e["rms"][l, b]), float(e["mx"][l, b])
                assert rms <= tol and mx <= mb[l], (f"{case_id(c)}: {q} layer {l} lane {b} (pad {c.pads[b]}): rms-rel {rms:.3e} (bound {tol:.1e}), max abs {mx:.3e} at slot "
                                                    f"{int(e['slot'][l, b])} (bound {mb[l]:.3e})")
    if m["inv"]:
        assert m["logit_err"] <= 4 * TOL[c.wd] * m["logit_scale"], f"{case_id(c)}: decode row logits max abs err {m['logit_err']}"
    # (e), (f)
    assert m["stray_bytes"] == 0, f"{case_id(c)}: {m['stray_bytes']} bytes written at or beyond the prompt end or in lanes the call does not name"
    assert m["saturations"] == 0


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_prompt_plan_vs_oracle(c):
    check_case(c, run_case(c))


def _begun(g, B, T):
    dev = g.device
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    msk = torch.ones(B, T, dtype=torch.int32, device=dev)
    bufs = {}
    begin(g, B, T, msk, st, bufs)
    return st, bufs


@gpu
@pytest.mark.parametrize("wd", ["fp32", "fp16"])
def test_prompt_plan_needs_a_prompt_pass(wd):
    """Between begin and the prefill call of a batch there is no plan to read: an error, not the previous batch's plan."""
    from chatttsplus_amd import _lib
    g = engine(Case(wd, "mid", {}, 256, 0, 0, (), {}))
    st, bufs = _begun(g, 2, 6)
    emb = torch.zeros(2, 6, H, device=g.device)
    _lib.check(g._lib.ctts_gpt_prefill(g._h, emb.data_ptr(), st), "prefill")
    assert g.prompt_plan()["rows_full"] == 12
    st, bufs = _begun(g, 2, 5)
    with pytest.raises(_lib.HipBackendError, match="no prompt pass"):
        g.prompt_plan()
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("wd", ["fp32", "fp16"])
def test_prompt_plan_after_score_describes_the_score_call(wd):
    """score() runs the prompt pass over its own [B][T]: the plan read afterwards is that call's (here three passes of 256, 256 and 88 rows)."""
    g = engine(Case(wd, "mid", {}, 256, 0, 0, (), {}))
    B, T = 4, 150
    emb = torch.zeros(B, T, H, device=g.device)
    mask = torch.ones(B, T, dtype=torch.long)
    g.score(emb, mask, torch.zeros(B, 3, 4, dtype=torch.int32), torch.full((B,), 3, dtype=torch.int32))
    p = g.prompt_plan()
    assert (p["passes"], p["rows_full"], p["rows_last"], p["pre_T"]) == (3, 256, 88, T)
    assert p["pfs"] == (1 if wd == "fp32" else 0) and p["last_pfs"] == p["pfs"]


# every value a prompt plan feature can take, per dtype: fp16 engines have no head / tail operands (pfs, the split kinds, sliced), fp32 engines no prefill_gemm and no
# MFMA attention; 256 x 256 prefill_gemm blocks (pfg2) exist in diagnostic builds only
_SPLITS = ("split64", "ring4", "ring2", "pp3", "pp4")
FEATURES = {
    "passes": (1, ">1"), "nbg": (1, 2), "prepack": (0, 1), "anchor": (0, 1),
    "pfg": {"fp32": (0,), "fp16": (0, 1)}, "pfs": {"fp32": (0, 1), "fp16": (0,)},
    "attn": {"fp32": ("row", "split"), "fp16": ("row", "mfma", "mfma_anchor")},
    "qkv": {"fp32": ("tile_norm", "tile_packed") + _SPLITS, "fp16": ("tile_norm", "tile_packed", "pfg0")},
    "o": {"fp32": ("tile_packed",) + _SPLITS, "fp16": ("tile_packed", "pfg0")},
    "gu": {"fp32": ("tile_norm", "tile_packed") + _SPLITS, "fp16": ("tile_norm", "tile_packed", "pfg0", "pfg1")},
    "down": {"fp32": ("tile_packed",) + _SPLITS, "fp16": ("tile_packed", "pfg0")},
    "down_sliced": {"fp32": (0, 1), "fp16": (0,)},
}
# plan fields that are no feature: the call's geometry, the projections whose K is never sliced, per-utterance adapters (their prompt pass: tests/test_gpu_lora_rows.py)
NOT_FEATURES = {"rows_full", "rows_last", "pre_T", "qkv_sliced", "o_sliced", "gu_sliced", "lora"}


def test_cases_cover_every_prompt_plan_feature():
    """The union of what the cases pin covers every value of every prompt plan feature, per dtype, every GEMM kind of every projection that is reachable on that
    dtype included: a field added to the plan without a case, or a case dropped, fails here.  A last_* field counts as its feature (the last pass is a pass).  No GPU work."""
    from chatttsplus_amd.hip_models.gpt import GPT
    base = set(FEATURES) | NOT_FEATURES
    assert base | {"last_" + f for f in base - {"passes", "rows_full", "rows_last", "pre_T"}} == set(GPT.PROMPT_PLAN_FIELDS), "a plan field is neither a feature with cases nor listed as not one"
    kinds = set(GPT.PROMPT_GEMM_KINDS) - {"pfg2"}
    assert kinds == {v for f in ("qkv", "o", "gu", "down") for wd in BOTH for v in FEATURES[f][wd]}, "a GEMM kind is reachable on no projection"
    assert set(GPT.PROMPT_ATTN_KINDS) == {v for wd in BOTH for v in FEATURES["attn"][wd]}
    missing = []
    for wd in BOTH:
        pinned = {}
        for c in CASES:
            if c.wd == wd:
                for k, v in c.expect.items():
                    pinned.setdefault(k[5:] if k.startswith("last_") else k, set()).add(v)
        for f, values in FEATURES.items():
            for v in (values[wd] if isinstance(values, dict) else values):
                if v not in pinned.get(f, ()):
                    missing.append(f"{wd}: no case pins {f} = {v}")
    assert not missing, missing
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for c in CASES:
        assert set(c.expect) <= set(GPT.PROMPT_PLAN_FIELDS), set(c.expect) - set(GPT.PROMPT_PLAN_FIELDS)
        mb, ms = ENGINES[c.engine]
        assert c.B <= mb and c.T + MAX_NEW <= ms
        assert c.B == 1 or c.T - 1 in c.pads, "every batch leaves one row a single real key"
