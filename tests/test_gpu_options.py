"""The engine's named options (ctts_gpt_set_option / ctts_gpt_get_option, include/ctts_hip.h): every option that can be set can be read back, a value is
clamped exactly as the if-chain did that preceded the option table (EXPECT below is transcribed from that chain, branch by branch -- it is NOT derived from
the table), refusals stay refusals, and "batch_invariant" reports its pins while the stored values wait underneath.

Engines without weights: options are settable before finalize, and nothing here launches a kernel."""
import os
import re

import pytest

from chatttsplus_amd import _lib

pytestmark = pytest.mark.gpu

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
PROBES = (-1000000, -5, -4, -3, -1, 0, 1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 256, 257, 4096, 4097, 1000000)
REFUSED = object()
INT_MAX = 0x7FFFFFFF


def at_least(lo):                       # value < lo ? lo : value
    return lambda v: lo if v < lo else v


def clamp(lo, hi):                      # value < lo ? lo : (value > hi ? hi : value)
    return lambda v: lo if v < lo else (hi if v > hi else v)


def flag(v):                            # value ? 1 : 0
    return 1 if v else 0


def auto_below_zero(hi):                # value < 0 ? -1 : (value > hi ? hi : value)
    return lambda v: -1 if v < 0 else (hi if v > hi else v)


# one entry per branch of the former ctts_gpt_set_option chain, in its order
EXPECT = {
    "batch_invariant": flag,                                                  # fp32 engines; fp16: refused (below)
    "prefill_split_rows": at_least(0),
    "split_decode_rows": at_least(0),
    "split_nbg2_rows": at_least(17),
    "weight_prefetch_kb": clamp(0, 4096),
    "valu_rows": clamp(0, 4),
    "persistent_rows": clamp(0, 8),                                           # CTTS_PERSIST_MAX_ROWS = PL_MAXR = 8; before finalize the stored value reads back
    "persistent_delay_lora": auto_below_zero(256),
    "prefill_small_blocks": at_least(0),
    "prefill_ring4_blocks": at_least(0),
    "prefill_splitk_rows": at_least(0),
    "prefill_pp_blocks": lambda v: 0 if v < -4 else v,
    "attn_wide_blocks": at_least(0),
    "persistent_share_keys": lambda v: 384 if v < 64 else v,
    "persistent_lora": flag,
    "persistent_heads": flag,
    "persistent_layers_per_launch": at_least(0),
    "persistent_schedule": lambda v: v if 1 <= v <= 3 else 1,
    "lora_fold": lambda v: 1 if (v < 0 or v > 3) else v,
    "persistent_fault": at_least(0),
    "persistent_pair_keys": at_least(0),
    "persistent_max_keys": at_least(0),
    "persistent_splits": clamp(0, 5),                                         # PL_SMAX = 5
    "persistent_pace": auto_below_zero(64),
    "persistent_delay_att": clamp(0, 256),
    "persistent_delay": clamp(0, 256),
    "persistent_delay_act": clamp(0, 256),
    "persistent_delay_x": clamp(0, 256),
    "persistent_nap_qkv": clamp(0, 256),
    "persistent_nap": clamp(0, 256),
    "persistent_poll": lambda v: -1 if v < 0 else (v & 1),
    "persistent_timestamps": flag,
    "decode_splits": lambda v: REFUSED if (v < 0 or v > 8) else v,            # SMAX = 8: refused, not clamped
    "split_rows": clamp(0, 32),
    "nbg2_rows": at_least(17),
    "down_splitk_rows": at_least(0),
    "graph_steps": clamp(1, 64),
    "graph_steps_persistent": clamp(1, 64),
}
# settable before this change but not readable: the reason this test exists
FORMERLY_WRITE_ONLY = ("persistent_pair_keys", "persistent_layers_per_launch", "persistent_schedule", "persistent_fault", "persistent_max_keys", "persistent_splits",
                       "persistent_pace", "persistent_delay", "persistent_delay_act", "persistent_delay_x", "persistent_delay_att", "persistent_nap",
                       "persistent_nap_qkv", "persistent_poll", "persistent_timestamps")
# what get_option reports while batch_invariant is on (include/ctts_hip.h)
PINS = {"persistent_rows": 0, "valu_rows": 0, "split_decode_rows": 1, "split_rows": 0, "down_splitk_rows": 1, "nbg2_rows": 0, "split_nbg2_rows": 0,
        "decode_splits": 1, "attn_wide_blocks": INT_MAX, "prefill_split_rows": 1, "prefill_splitk_rows": 0}


def bare_engine(dtype):
    from chatttsplus_amd.hip_models import GPT
    return GPT(LLAMA, max_batch=2, max_seq_len=64, weight_dtype=dtype)


def header_option_names():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctts_hip.h")
    text = open(path).read()
    comment = text[text.index("/* Named engine options"):text.index("Unknown names are an error. */")]
    return sorted(set(re.findall(r'"([a-z0-9_]+)"', comment)))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_every_option_clamps_as_before_and_reads_back(dtype):
    g = bare_engine(dtype)
    try:
        assert set(FORMERLY_WRITE_ONLY) <= set(EXPECT) and len(FORMERLY_WRITE_ONLY) == 15
        for name in sorted(EXPECT, key=lambda n: n == "batch_invariant"):      # batch_invariant last: while it is on, pinned options read their pins
            for v in PROBES:
                want = EXPECT[name](v)
                if name == "batch_invariant" and dtype == "fp16":
                    want = REFUSED
                before = g.get_option(name)
                if want is REFUSED:
                    with pytest.raises(_lib.HipBackendError, match=name):
                        g.set_option(name, v)
                    assert g.get_option(name) == before, f"{name}: the refused value {v} changed the option"
                else:
                    g.set_option(name, v)
                    got = g.get_option(name)
                    assert got == want, f"{dtype} {name}: set {v} reads {got}, the chain stored {want}"
                    if name == "batch_invariant":
                        g.set_option(name, 0)
    finally:
        g.close()


def test_formerly_write_only_options_read_back():
    """fails before the option table: these fifteen could be set and not read"""
    g = bare_engine("fp32")
    try:
        for name in FORMERLY_WRITE_ONLY:
            g.set_option(name, 1)
            assert g.get_option(name) == EXPECT[name](1)
    finally:
        g.close()


def test_every_option_the_header_names_is_readable():
    names = header_option_names()
    assert "persistent_pair_keys" in names and "lora_mlp_live" in names and len(names) >= 36
    assert set(names) <= set(EXPECT) | {"lora_mlp_live"}, "the header names an option this test does not know"
    g = bare_engine("fp32")
    try:
        for name in names:
            g.get_option(name)
        assert g.get_option("lora_mlp_live") == 0
        with pytest.raises(_lib.HipBackendError, match="unknown option 'lora_mlp_live'"):      # read only
            g.set_option("lora_mlp_live", 1)
    finally:
        g.close()


def test_batch_invariant_reports_pins_and_keeps_stored_values():
    g = bare_engine("fp32")
    first = {"persistent_rows": 3, "valu_rows": 1, "split_decode_rows": 12, "split_rows": 6, "down_splitk_rows": 11, "nbg2_rows": 40, "split_nbg2_rows": 20,
             "decode_splits": 2, "attn_wide_blocks": 300, "prefill_split_rows": 100, "prefill_splitk_rows": 1000}
    second = {k: v + 1 for k, v in first.items()}
    assert set(first) == set(PINS)
    try:
        for k, v in first.items():
            g.set_option(k, v)
            assert g.get_option(k) == v
        g.set_option("batch_invariant", 1)
        for k, pin in PINS.items():
            assert g.get_option(k) == pin, f"{k} reads {g.get_option(k)} under batch_invariant, the header says {pin}"
        unpinned = [n for n in EXPECT if n not in PINS and n != "batch_invariant"]
        for k in unpinned:                                 # everything else stays live
            g.set_option(k, 2)
            assert g.get_option(k) == EXPECT[k](2)
        for k, v in second.items():                        # stored, not used: the pins still read
            g.set_option(k, v)
            assert g.get_option(k) == PINS[k]
        with pytest.raises(_lib.HipBackendError, match="decode_splits"):
            g.set_option("decode_splits", 9)
        g.set_option("batch_invariant", 0)
        for k, v in second.items():
            assert g.get_option(k) == v, f"{k}: the value stored while batch_invariant was on did not return"
    finally:
        g.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_unknown_names_are_errors(dtype):
    g = bare_engine(dtype)
    try:
        with pytest.raises(_lib.HipBackendError, match="set_option: unknown option 'no_such_option'"):
            g.set_option("no_such_option", 1)
        with pytest.raises(_lib.HipBackendError, match="get_option: unknown option 'no_such_option'"):
            g.get_option("no_such_option")
    finally:
        g.close()
