"""Guided refine-text, host side (no GPU): the pure-Python automaton (guide_allowed / guide_step, the twin of the device state machine in sampler_text_kernel),
the source extraction from a refine prompt, the default free set, and every refusal that is decided on the host."""
import random

import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models.gpt import (GUIDE_MAX_FREE, GUIDE_MAX_SRC, DecodeSession, TextGuide, check_guide_src, guide_allowed, guide_arrays,
                                            guide_eos_removable, guide_standin, guide_step, resolve_guides, text_rows_cfg)
from chatttsplus_amd.pipeline import (REFINE_FREE_TOKENS, ChatTTSPlusPipeline, check_refine_sources, default_text_guide, refine_sources,
                                      resolve_refine_guided)

EOS, VOCAB = 11, 64
FREE = (9, 20, 33)


def _walk(rng, src, free, max_run, limit):
    """one random walk: uniform draws from the allowed set until EOS; returns the ids (EOS included)"""
    n, cur, run, out = len(src), 0, 0, []
    for t in range(limit):
        a = guide_allowed(cur, run, t, limit, n, max_run, src, free, EOS)
        assert a and guide_standin(cur, n, src, EOS) in a
        idx = rng.choice(a)
        out.append(idx)
        cur, run, fin = guide_step(cur, run, t, limit, n, max_run, idx, src=src, eos=EOS)
        if fin:
            return out
    raise AssertionError(f"no EOS within the limit {limit}: {out}")


def _strip(ids, src, free):
    """greedy removal of free tokens: an id that matches the next source id is the source's (the precedence rule), any other one is a free token"""
    k, runs, run = 0, [], 0
    for i in ids:
        if k < len(src) and i == src[k]:
            k += 1
            runs.append(run)
            run = 0
        else:
            assert i in free, f"id {i} is neither the next source id nor a free id"
            run += 1
    runs.append(run)
    return k, runs


@pytest.mark.parametrize("max_run", [0, 1, 2, 3])
def test_random_walks_keep_every_source_token(max_run):
    rng = random.Random(1000 + max_run)
    seen_precedence = False
    for n in range(1, 13):
        for extra in range(1, 9):
            for rep in range(6):
                # sources over the plain ids AND the free ids: src[cur] in `free` is the precedence case
                src = [rng.choice([15, 16, 17, 18] + list(FREE)) for _ in range(n)]
                limit = n + extra
                ids = _walk(rng, src, FREE, max_run, limit)
                assert ids[-1] == EOS and EOS not in ids[:-1] and len(ids) <= limit
                k, runs = _strip(ids[:-1], src, FREE)
                assert k == n, f"src {src} -> {ids}: {k} of {n} source ids"
                assert max(runs) <= max_run
                if max_run == 0 or extra == 1:
                    assert ids == src + [EOS]                  # no slack (or no free run): exactly the source
                seen_precedence = seen_precedence or any(s in FREE for s in src)
    assert seen_precedence


def test_precedence_and_slack_rules():
    src = [9, 15]                                              # src[0] is a free id
    # a draw of 9 at cur = 0 is the source's: cur advances, run stays 0
    assert guide_step(0, 0, 0, 10, 2, 2, 9, src=src, eos=EOS) == (1, 0, False)
    assert guide_step(1, 0, 1, 10, 2, 2, 9, src=src, eos=EOS) == (1, 1, False)       # ... at cur = 1 it is a free token
    assert guide_step(2, 1, 5, 10, 2, 2, EOS, src=src, eos=EOS) == (2, 1, True)
    # slack: limit 4, n = 2: step 0 has slack 1 (free allowed), step 1 with cur = 0 has slack 0
    assert guide_allowed(0, 0, 0, 4, 2, 2, src, FREE, EOS) == sorted({9, 20, 33})
    assert guide_allowed(0, 1, 1, 4, 2, 2, src, FREE, EOS) == [9]
    # the end: EOS plus free while a step is left behind it
    assert guide_allowed(2, 0, 2, 4, 2, 2, src, FREE, EOS) == sorted({EOS, *FREE})
    assert guide_allowed(2, 0, 3, 4, 2, 2, src, FREE, EOS) == [EOS]
    assert guide_allowed(2, 2, 2, 4, 2, 2, src, FREE, EOS) == [EOS]                  # run == max_run
    # min_new_token removes EOS only while another element remains
    assert guide_eos_removable(2, 0, 2, 4, 2, 2, FREE) and not guide_eos_removable(2, 0, 3, 4, 2, 2, FREE) and not guide_eos_removable(2, 0, 2, 4, 2, 2, ())


def test_guide_arrays_layout():
    sl, cat, off = guide_arrays([3, 0, 7], [[5, 6], None, [8]])
    assert sl.tolist() == [3, 0, 7] and cat.tolist() == [5, 6, 8] and off.tolist() == [0, 2, 2, 3]


# ---- source extraction and the default free set ----------------------------------------------------------------------------------------------------------
def test_sources_from_a_refine_prompt(tmp_path):
    tok = synth.toy_tokenizer(str(tmp_path))
    texts = ["a b c", "d [uv_break]", "b a d c a"]
    ids, att, _ = tok.encode([f"[Sbreak]{t}[Pbreak][speed_5]" for t in texts], 4)
    assert int((att[1] == 0).sum()) > 0                         # left-padded rows included
    srcs = refine_sources(tok, ids, att)
    # the very tokenisation the model sees: what the tokenizer makes of the text alone (the toy tokenizer knows its tags; its words share one id)
    assert srcs == [tok._tokenizer(t, add_special_tokens=False)["input_ids"] for t in texts]
    assert [len(s) for s in srcs] == [3, 2, 5] and srcs[1][1] == synth.TOY_VOCAB.index("[uv_break]")
    assert refine_sources(tok, ids[..., 0], att) == srcs      # [B, T] ids as well
    check_refine_sources(srcs, 6)
    with pytest.raises(_lib.HipBackendError, match="utterance 2 has 5 tokens and needs max_new_token >= 6"):
        check_refine_sources(srcs, 5)
    ids2, att2, _ = tok.encode(["a b c"], 4)
    with pytest.raises(_lib.HipBackendError, match=r"no \[Sbreak\]"):
        refine_sources(tok, ids2, att2)
    ids3, att3, _ = tok.encode(["[Sbreak][Pbreak]"], 4)
    with pytest.raises(_lib.HipBackendError, match="no token between"):
        check_refine_sources(refine_sources(tok, ids3, att3), 8)


class _FakeBert:
    unk_token_id = 1

    def __init__(self, known):
        self.known = known

    def convert_tokens_to_ids(self, name):
        return self.known.get(name, self.unk_token_id)


class _FakeTok:
    def __init__(self, known):
        self._tokenizer = _FakeBert(known)


def test_default_free_set():
    tok = _FakeTok({"[uv_break]": 40, "[laugh]": 41, "[lbreak]": 42, "[other]": 43})
    g = default_text_guide(tok)
    assert g.free_ids == (40, 42, 41) and g.max_run == 2      # in REFINE_FREE_TOKENS order; [v_break] / [llbreak] map to the unknown id: skipped
    assert set(REFINE_FREE_TOKENS) == {"[uv_break]", "[v_break]", "[lbreak]", "[llbreak]", "[laugh]"}
    with pytest.raises(_lib.HipBackendError, match="knows none of"):
        default_text_guide(_FakeTok({"[other]": 43}))
    assert resolve_refine_guided(False, tok) is None and resolve_refine_guided(None, tok) is None
    assert resolve_refine_guided(True, tok).free_ids == (40, 42, 41)
    mine = TextGuide([7], 1)
    assert resolve_refine_guided(mine, tok) is mine
    with pytest.raises(_lib.HipBackendError, match="False, True or a TextGuide"):
        resolve_refine_guided("yes", tok)


def test_toy_tokenizer_default_free_set(tmp_path):
    tok = synth.toy_tokenizer(str(tmp_path))
    assert default_text_guide(tok).free_ids == (synth.TOY_VOCAB.index("[uv_break]"),)


# ---- refusals decided on the host ----------------------------------------------------------------------------------------------------------------------
def test_text_guide_refusals():
    with pytest.raises(_lib.HipBackendError, match="at most 64"):
        TextGuide(list(range(GUIDE_MAX_FREE + 1)))
    with pytest.raises(_lib.HipBackendError, match="listed twice"):
        TextGuide([3, 4, 3])
    with pytest.raises(_lib.HipBackendError, match="max_run=-1"):
        TextGuide([3], max_run=-1)
    with pytest.raises(_lib.HipBackendError, match="negative"):
        TextGuide([-2])
    g = TextGuide([3, EOS])
    with pytest.raises(_lib.HipBackendError, match="is the EOS token"):
        g.check(EOS, VOCAB)
    with pytest.raises(_lib.HipBackendError, match="outside 0..63"):
        TextGuide([64]).check(EOS, VOCAB)
    assert TextGuide(list(range(12, 12 + GUIDE_MAX_FREE)), 0).max_run == 0


def test_guide_src_refusals():
    assert check_guide_src(torch.tensor([15, 16]), 3, EOS, VOCAB) == [15, 16]
    with pytest.raises(_lib.HipBackendError, match="n == 0"):
        check_guide_src([], 8, EOS, VOCAB)
    with pytest.raises(_lib.HipBackendError, match="needs 3 tokens .* limit is 2"):
        check_guide_src([15, 16], 2, EOS, VOCAB)
    with pytest.raises(_lib.HipBackendError, match="outside 0..63"):
        check_guide_src([15, 64], 8, EOS, VOCAB)
    with pytest.raises(_lib.HipBackendError, match="is the EOS token"):
        check_guide_src([15, EOS], 8, EOS, VOCAB)
    with pytest.raises(_lib.HipBackendError, match=f"at most {GUIDE_MAX_SRC}"):
        check_guide_src([15] * (GUIDE_MAX_SRC + 1), 4096, EOS, VOCAB)


def test_resolve_guides_refusals():
    g = TextGuide(FREE)
    assert resolve_guides(None, None, 2, True, EOS, VOCAB, [8, 8]) is None
    assert resolve_guides(g, [[15], None], 2, True, EOS, VOCAB, [8, 8]) == [[15], None]
    assert resolve_guides(g, None, 2, True, EOS, VOCAB, [8, 8]) == [None, None]
    with pytest.raises(_lib.HipBackendError, match="without the per-call part"):
        resolve_guides(None, [[15], None], 2, True, EOS, VOCAB, [8, 8])
    with pytest.raises(_lib.HipBackendError, match="a guide on a code row"):
        resolve_guides(g, [[15], None], 2, False, EOS, VOCAB, [8, 8])
    with pytest.raises(_lib.HipBackendError, match="1 entries for 2"):
        resolve_guides(g, [[15]], 2, True, EOS, VOCAB, [8, 8])
    with pytest.raises(_lib.HipBackendError, match=r"guide_src\[1\]: a source of 2 ids needs 3 tokens"):
        resolve_guides(g, [[15], [15, 16]], 2, True, EOS, VOCAB, [8, 2])         # against the sequence's OWN limit
    with pytest.raises(_lib.HipBackendError, match="is the EOS token"):
        resolve_guides(TextGuide([EOS]), None, 1, True, EOS, VOCAB, [8])
    with pytest.raises(_lib.HipBackendError, match="must be a TextGuide"):
        resolve_guides([9], None, 1, True, EOS, VOCAB, [8])


def test_text_rows_dict_takes_a_guide():
    cfg = text_rows_cfg(dict(eos_token=EOS, max_new_token=8, guide=TextGuide(FREE)))
    assert cfg.infer_text == 1 and cfg.max_new_token == 8
    with pytest.raises(_lib.HipBackendError, match="unknown key"):
        text_rows_cfg(dict(eos_token=EOS, max_new_token=8, guides=1))


def test_pipeline_level_refusals():
    pipe = ChatTTSPlusPipeline.__new__(ChatTTSPlusPipeline)
    with pytest.raises(_lib.HipBackendError, match=r"infer_sharded\(refine_guided"):
        pipe.infer_sharded(["a"], refine_guided=True)
