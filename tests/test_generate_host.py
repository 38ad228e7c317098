"""Host logic of generate()'s driver (CPU): the one compaction rule against both formulas it replaced, and the call resolver -- the "auto" noise rule, the seed
draw, the prompt_of refusals and the per-row arrays."""
import itertools

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import compact_keep, compact_size, resolve_generate


# ---- the compaction rule ---------------------------------------------------------------------------------------------------------------------------
def _session_formula(live_flags):
    """SessionBook.plan before the rule was shared: live rows + the first free rows up to compact_size(live)"""
    B = len(live_flags)
    live = [r for r in range(B) if live_flags[r]]
    free = [r for r in range(B) if not live_flags[r]]
    target = compact_size(len(live))
    return sorted(live + free[:target - len(live)]) if live and target < B else None


def _generate_formula(row_seq, done_seq):
    """generate()'s loop before the rule was shared: rows by the sequence they hold, finished sequences in a set"""
    live = [r for r, sq in enumerate(row_seq) if sq not in done_seq]
    target = compact_size(len(live))
    if live and target < len(row_seq):
        fill = [r for r, sq in enumerate(row_seq) if sq in done_seq][:target - len(live)]
        return sorted(live + fill)
    return None


def _check_pattern(flags, rng):
    row_seq = [int(s) for s in rng.permutation(len(flags)) + 100]          # the sequences the rows hold, in any order
    done = {sq for sq, f in zip(row_seq, flags) if not f}
    want = _session_formula(flags)
    assert _generate_formula(row_seq, done) == want
    got = compact_keep(flags)
    assert got == want, flags
    if got is not None:
        assert got == sorted(set(got)) and len(got) == compact_size(sum(flags)) < len(flags) and all(r in got for r, f in enumerate(flags) if f)


def test_compact_keep_every_pattern_up_to_12_rows():
    rng = np.random.Generator(np.random.Philox(key=3))
    for B in range(1, 13):
        for flags in itertools.product((False, True), repeat=B):
            _check_pattern(list(flags), rng)
    assert compact_keep([]) is None and compact_keep([False] * 5) is None and compact_keep([True] * 5) is None
    assert compact_keep([True, False, True, False]) == [0, 2]


@pytest.mark.parametrize("B", [17, 33, 65])
def test_compact_keep_random_patterns_across_the_quanta(B):
    """above 16 rows compact_size rounds up (to 2, 4, 8): finished rows stay as padding, the first ones"""
    rng = np.random.Generator(np.random.Philox(key=B))
    padded = 0
    for _ in range(400):
        flags = [bool(x) for x in rng.random(B) < rng.random()]
        _check_pattern(flags, rng)
        keep = compact_keep(flags)
        padded += keep is not None and len(keep) > sum(flags)
    for n_live in range(1, B + 1):                                        # and one pattern per live count: every size of the rule is crossed
        _check_pattern([r < n_live for r in rng.permutation(B)], rng)
    possible = any(n < compact_size(n) < B for n in range(1, B + 1))      # (not at 17 rows: up to 16 live rows every size exists, and 17 live rows stay)
    assert bool(padded) == possible, "no pattern kept a finished row as padding"


# ---- the call resolver -------------------------------------------------------------------------------------------------------------------------------
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
FACTS = dict(max_batch=12, num_vq=4, vocab_code=626, vocab_text=21178, fp16_invariant=False)


def _resolve(n, facts=None, **kw):
    args = dict(temperature=torch.tensor([0.3] * 4), eos_token=625, max_new_token=20, logits_warpers=LW, logits_processors=[])
    args.update(kw)
    return resolve_generate(n, **dict(FACTS, **(facts or {})), **args)


@pytest.mark.parametrize("n, kw, facts, want", [
    (1, {}, {}, "torch"),
    (4, {}, {}, "torch"),                                        # 4 * 4 * 626 = 10016 <= 16384
    (5, {}, {}, "device"),                                       # more sequences than the reference's slices of 4
    (1, dict(infer_text=True, temperature=torch.tensor([0.7]), eos_token=21177), {}, "device"),      # 21178 > 16384
    (4, {}, dict(vocab_code=1024), "torch"),                     # 16384 numbers per step: the last that stays on the host
    (4, {}, dict(vocab_code=1025), "device"),
    (1, {}, dict(fp16_invariant=True), "device"),                # an fp16 engine under an invariant option takes device noise only
    (3, dict(prompt_of=[0, 1, 2, 0]), {}, "torch"),              # the rule counts sequences, not prompts
    (3, dict(prompt_of=[0, 1, 2, 0, 1]), {}, "device"),
])
def test_auto_noise_rule(n, kw, facts, want):
    call = _resolve(n, facts, **kw)
    assert call.noise == want and (call.rows_per_seq, call.V) == ((1, 21178) if kw.get("infer_text") else (4, facts.get("vocab_code", 626)))
    assert _resolve(n, facts, noise="torch", **kw).noise == "torch" and _resolve(n, facts, noise="device", seed=1, **kw).noise == "device"


def test_seed_is_drawn_exactly_for_device_noise_without_one():
    def after(**kw):
        torch.manual_seed(77)
        call = _resolve(kw.pop("n", 2), **kw)
        return call, torch.random.get_rng_state()

    torch.manual_seed(77)
    untouched = torch.random.get_rng_state()
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())
    one_draw = torch.random.get_rng_state()
    for kw in (dict(noise="device"), dict(n=5), dict(infer_text=True, temperature=torch.tensor([0.7]))):          # chosen by name or by the "auto" rule
        call, state = after(**kw)
        assert call.noise == "device" and call.seed == drawn and torch.equal(state, one_draw)
    for kw in (dict(noise="device", seed=5), dict(noise="torch"), dict(), dict(noise="torch", seed=5), dict(noise=torch.ones(3, 8, 626))):
        call, state = after(**kw)
        assert call.seed == kw.get("seed", 0) and torch.equal(state, untouched)
    assert torch.is_tensor(after(noise=torch.ones(3, 8, 626))[0].noise)


def test_prompt_of_refusals_keep_their_text():
    with pytest.raises(_lib.HipBackendError, match=r"prompt_of\[1\]=3 is out of range: the call has 2 prompts"):
        _resolve(2, prompt_of=[0, 3, 1])
    with pytest.raises(_lib.HipBackendError, match="prompt_of: prompt 1 is named by no sequence"):
        _resolve(2, prompt_of=[0, 0])
    with pytest.raises(_lib.HipBackendError, match="prompt_of: shared prompt passes are code mode only"):
        _resolve(1, prompt_of=[0, 0], infer_text=True, temperature=torch.tensor([0.7]))
    with pytest.raises(_lib.HipBackendError, match="prompt_of: 13 sequences exceed max_batch=12"):
        _resolve(2, prompt_of=[0, 1] + [0] * 11)
    call = _resolve(3, prompt_of=[0, 0, 1, 1, 2, 2])
    assert call.B == 6 and call.share[0].dtype == np.int32 and call.share[0].tolist() == [0, 0, 1, 1, 2, 2] and call.share[1] == 3
    assert _resolve(3).share is None and _resolve(3).B == 3


def test_per_row_arrays():
    call = _resolve(3, utt_ids=[7, 2 ** 40, 9], row_limits=[1, 20, 5], sampling_per_row=[None, dict(temperature=0.7), None])
    assert call.utt_ids.dtype == np.uint64 and call.utt_ids.tolist() == [7, 2 ** 40, 9]
    assert call.row_limits.dtype == np.int32 and call.row_limits.tolist() == [1, 20, 5] and len(call.knobs) == 3
    assert abs(call.knobs[1].temperature[0] - 0.7) < 1e-6 and abs(call.knobs[0].temperature[0] - 0.3) < 1e-6
    plain = _resolve(3)
    assert plain.utt_ids is None and plain.row_limits is None and plain.knobs is None
    with pytest.raises(AssertionError, match="utt_ids: one id per sequence"):
        _resolve(3, utt_ids=[1, 2])
    with pytest.raises(AssertionError, match="max_new_tokens_per_row: one limit per sequence"):
        _resolve(3, row_limits=[1, 2, 3, 4])
    with pytest.raises(_lib.HipBackendError, match="sampling_per_row: 2 entries for 3 sequences"):
        _resolve(3, sampling_per_row=[None, None])
    with pytest.raises(AssertionError, match="utt_ids: one id per sequence"):             # the arrays are per sequence, not per prompt
        _resolve(2, prompt_of=[0, 1, 1], utt_ids=[1, 2])
    with pytest.raises(_lib.HipBackendError, match="sampling_per_row: per-utterance sampling parameters are code mode only"):
        _resolve(1, infer_text=True, temperature=torch.tensor([0.7]), sampling_per_row=[None])


def test_the_record_holds_what_the_resolver_decides():
    call = _resolve(2, max_new_token=33, infer_text=False)
    assert sorted(vars(call)) == sorted(["B", "share", "sc", "knobs", "noise", "seed", "utt_ids", "row_limits", "rows_per_seq", "V"])
    assert call.sc.max_new_token == 33 and call.sc.eos_token == 625 and not call.sc.infer_text
    assert _resolve(1, infer_text=True, temperature=torch.tensor([0.7]), eos_token=21177).sc.infer_text == 1


# ---- a failed begin / admit leaves nothing staged ------------------------------------------------------------------------------------------------------
class FakeLib:
    """stands in for the engine library: notes every call, and the calls named in `fail` return non-zero"""

    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def ctts_last_error(self):
        return b"made to fail"

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name[len("ctts_gpt_"):],) + tuple(args[1:]))
            return 1 if name in self.fail else 0
        return call


def _fake_engine(monkeypatch, fail):
    import ctypes as C
    from chatttsplus_amd.hip_models.gpt import GPT
    lib = FakeLib(fail)
    monkeypatch.setattr(_lib, "load", lambda: lib)              # (_lib.check asks it for the error text)
    g = object.__new__(GPT)
    g._lib, g._h, g.device, g.num_vq = lib, C.c_void_p(), torch.device("cpu"), 4
    return g, lib


CLEARS = [("set_row_sampling", None, 0), ("set_row_modes", None, 0), ("share_prompts", 0, None, 0)]


@pytest.mark.parametrize("fail", [(), ("ctts_gpt_begin",), ("ctts_gpt_share_prompts",)], ids=["ok", "begin-fails", "staging-fails"])
def test_begin_clears_what_it_staged(monkeypatch, fail):
    from types import SimpleNamespace
    g, lib = _fake_engine(monkeypatch, fail)
    sc = _lib.SamplerCfg()
    knobs = (_lib.RowSampling * 2)()
    args = (None, 2, 5, torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5, 8), sc, _lib.GenIO(), SimpleNamespace(lps=None, tids=None))
    kw = dict(knobs=knobs, modes=np.array([0, 1], dtype=np.int32), share=(np.array([0, 0], dtype=np.int32), 1))
    if fail:
        with pytest.raises(_lib.HipBackendError, match="made to fail"):
            g._begin_state(*args, **kw)
    else:
        g._begin_state(*args, **kw)
    names = [c[0] for c in lib.calls]
    staged = ["set_row_sampling", "set_row_modes", "share_prompts"]
    assert names[:3] == staged and [c for c in lib.calls if c[0] in staged][-3:] == CLEARS, "every staged request is cleared, whatever begin did"
    assert ("begin" in names) == ("ctts_gpt_share_prompts" not in fail) and ("prefill" in names) == (not fail)
    lib.calls.clear()
    lib.fail.clear()
    g._begin_state(*args)                                      # a plain begin stages nothing; whatever an earlier failure left pending ends with it too
    assert lib.calls[0][0] == "begin" and lib.calls[1:4] == CLEARS and [c[0] for c in lib.calls[4:]] == ["prefill"]


@pytest.mark.parametrize("fail", [(), ("ctts_gpt_admit",)], ids=["ok", "admit-fails"])
def test_admit_clears_the_shared_prompts_it_staged(monkeypatch, fail):
    from types import SimpleNamespace
    from chatttsplus_amd.hip_models.gpt import DecodeSession
    g, lib = _fake_engine(monkeypatch, fail)
    ses = object.__new__(DecodeSession)
    ses.gpt, ses.sc, ses.text_sc, ses._adapters, ses.launched = g, _lib.SamplerCfg(), None, False, 9
    ses.shared_prompts, ses.admissions = [], []
    ses._share = ([0, 0], 1, None)                              # tickets 0 and 1 name the one prompt
    ses._req = {tk: (torch.zeros(5, 8), 5, None, None, 0) for tk in (0, 1)}
    ses.book = SimpleNamespace(utts={tk: dict(utt_id=40 + tk, limit=7, slot=tk, attempt=0) for tk in (0, 1)})
    if fail:
        with pytest.raises(_lib.HipBackendError, match="made to fail"):
            ses._seat([(2, 0), (3, 1)], None)
    else:
        ses._seat([(2, 0), (3, 1)], None)
    names = [c[0] for c in lib.calls]
    assert names == ["share_prompts", "admit", "share_prompts"], "staged next to the admit it is for, and cleared after it"
    assert lib.calls[0][1] == 2 and lib.calls[0][3] == 1 and lib.calls[-1] == ("share_prompts", 0, None, 0)
    assert ses.shared_prompts == [(2, 1)] and ses.admissions == ([] if fail else [(9, 2)])
