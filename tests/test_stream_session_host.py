"""Streaming from a serving session, host side (no GPU): the settled-sample rule (vocoder.settled_samples, window_token_range(clamp_tail=False)) against the
receptive-field model of tests/test_host_logic.py, its C twin ctts_synth_window_range, and SessionBook's window bookkeeping against scripted row reports."""
import ctypes as C

import numpy as np
import pytest

import chatttsplus_amd.hip_models.vocoder as voc
from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import SESSION_OUT_OF_SCOPE, SessionBook, refuse_out_of_scope

HOP, HALO = 256, voc.Synth.HALO_FRAMES


def _total(n):
    return HOP * (2 * n - 1) if n > 0 else 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------------------
def test_settled_samples_is_monotone_bounded_and_zero_below_the_hold_back():
    hold = (HALO + 2 + 1) // 2                                    # tokens before the first sample settles: 2 n - (HALO + 2) > 0
    prev = 0
    for n in range(0, 400):
        s = voc.settled_samples(n, HOP, HALO)
        assert prev <= s <= _total(n) and s % HOP == 0
        assert (s == 0) == (n < hold), f"n = {n}: {s} settled samples, hold-back {hold} tokens"
        assert s == HOP * max(0, 2 * n - HALO - 2)
        assert voc.settled_samples(n, HOP, HALO, finished=True) == _total(n)
        prev = s
    assert _total(300) - voc.settled_samples(300, HOP, HALO) == HOP * (HALO + 1)      # what an unfinished utterance holds back: 106 frames = 53 tokens


def test_settled_windows_need_no_later_frame_and_their_token_range_ignores_n():
    """test_window_token_range_covers_the_receptive_field's model: a window [c0, c1) depends on mel frames c0/hop - 1 - (halo - 3) .. (c1 - 1)/hop + 2 + (halo - 3)."""
    rng = np.random.Generator(np.random.Philox(key=11))
    for _ in range(2000):
        n = int(rng.integers(1, 900))
        st = voc.settled_samples(n, HOP, HALO)
        if st == 0:
            with pytest.raises(ValueError, match="not settled"):
                voc.window_token_range(n, 0, 1, HOP, HALO, clamp_tail=False)
            continue
        s1 = int(rng.integers(1, st + 1)); s0 = int(rng.integers(0, s1))
        a, b, off, c0, c1 = voc.window_token_range(n, s0, s1, HOP, HALO, clamp_tail=False)
        assert (c0, c1) == (s0, s1) and 0 <= a < b <= n and off == 2 * a * HOP
        need_lo = max(0, c0 // HOP - 1 - (HALO - 3))
        need_hi = (c1 - 1) // HOP + 2 + (HALO - 3)              # NOT clamped to the prefix: every needed frame must exist
        assert need_hi <= 2 * n - 1, "a settled window depends on a frame the prefix does not have"
        assert 2 * a <= need_lo and need_hi <= 2 * b - 1
        assert c1 - off <= HOP * (2 * (b - a) - 1)
        for N in (n + 1, n + int(rng.integers(1, 500)), 5000):
            assert voc.window_token_range(N, s0, s1, HOP, HALO, clamp_tail=False) == (a, b, off, c0, c1)
        assert voc.settled_token_range(n, s0, s1, HOP, HALO) == (a, b, off, c0, c1)
        with pytest.raises(ValueError, match="not settled"):
            voc.window_token_range(n, s0, st + 1, HOP, HALO, clamp_tail=False)
    # the default stays today's rule
    assert voc.window_token_range(200, 1000, 5000) == voc.window_token_range(200, 1000, 5000, HOP, 105, clamp_tail=True)


def test_the_c_twin_equals_the_python_functions():
    lib = _lib.load()                                             # loads without a GPU: the entry is host code
    rng = np.random.Generator(np.random.Philox(key=12))
    out = (C.c_int64 * 5)()
    refused = 0
    for i in range(2000):
        n = int(rng.integers(0, 900))
        total = _total(n)
        s0 = int(rng.integers(0, total + 50)); s1 = int(rng.integers(s0, total + 400))
        clamp = bool(i % 2)
        if not clamp and i % 4 == 0:
            s1 = min(s1, voc.settled_samples(n, HOP, HALO))
        hop, halo = (HOP, HALO) if i % 5 else (int(rng.integers(1, 600)), int(rng.integers(3, 200)))
        rc = lib.ctts_synth_window_range(n, s0, s1, hop, halo, int(clamp), out)
        try:
            want = voc.window_token_range(n, s0, s1, hop, halo, clamp_tail=clamp)
        except ValueError:
            assert rc == 1 and b"not settled" in lib.ctts_last_error()
            refused += 1
            continue
        assert rc == 0 and tuple(out) == want, f"n={n} s0={s0} s1={s1} hop={hop} halo={halo} clamp={clamp}: {tuple(out)} vs {want}"
    assert 100 < refused < 1500


# ---- SessionBook ------------------------------------------------------------------------------------------------------------------------------------------
def _book(rows=4, out_slots=6, **kw):
    return SessionBook(rows, out_slots, 8, max_seq=400, max_new_token=200, stream_batch=8, **kw)


class Script:
    """Drives a SessionBook as DecodeSession.step does -- plan, report -- with token counts the test scripts: every live row gains `gain` tokens per report
    up to its `ends` entry (ticket -> (tokens, fin bits)), where it finishes."""

    def __init__(self, book, ends, gain=5):
        self.book, self.ends, self.gain, self.n = book, ends, gain, {}
        self.windows, self.done, self.stale = {}, {}, None

    def step(self, first_eos=()):
        b = self.book
        for tk in b.take_dropped():
            self.done[tk] = (0, True)
        b.plan()
        b.cancel_rows()
        lay, states = b.book.layout(), []
        for t in lay:
            if t is None or t not in b.book.tickets:
                states.append((1, 0))
                continue
            tk = b.book.tickets[t][0]
            u = b.utts[tk]
            if tk in first_eos and u["attempt"] == 0:
                states.append((2, 0))
                continue
            end, fin = self.ends[tk]
            n = min(self.n.get((tk, u["attempt"]), 0) + self.gain, end)
            self.n[(tk, u["attempt"])] = n
            if u["cancelled"]:
                states.append((1, n))
            else:
                states.append((fin if n >= end else 0, n))
        # the report is read one chunk late, as in the session: interpret the PREVIOUS one
        prev, self.stale = self.stale, (lay, states)
        if prev is None:
            return
        for tk, n, fin, cancelled in b.report(*prev):
            self.done[tk] = (n, cancelled)
            b.release(tk)
        for w in b.take_windows():
            self.windows.setdefault(w[0], []).append(w)

    def run(self, **kw):
        for _ in range(400):
            if self.book.idle():
                break
            self.step(**kw)
        assert self.book.idle()
        for tk in self.book.take_dropped():
            self.done[tk] = (0, True)
        for w in self.book.take_windows():
            self.windows.setdefault(w[0], []).append(w)


def _check_cover(ws, total):
    """consecutive, disjoint, covering [0, total); exactly one final window, the last"""
    assert [w[5] for w in ws] == [False] * (len(ws) - 1) + [True]
    pos = 0
    for tk, slot, n, s0, s1, final in ws:
        assert s0 == pos and s1 >= s0
        assert final or s1 > s0, "an empty window that is not the final one"
        pos = s1
    assert pos == total


def test_windows_are_consecutive_disjoint_and_cover_the_utterance():
    b = _book()
    ends = {}
    kinds = ["exact", "eager", None, "exact", "eager", None, "exact"]
    lims = [150, 140, 90, 60, 55, 30, 3]
    for k, lim in zip(kinds, lims):
        tk = b.submit(10, 100 + len(ends), limit=lim, stream=k, stream_batch=None if k is None else 8)
        ends[tk] = (lim, 1)
    s = Script(b, ends)
    s.run()
    assert sorted(s.done) == sorted(ends) and all(s.done[tk] == (ends[tk][0], False) for tk in ends)
    for tk, k in enumerate(kinds):
        if k is None:
            assert tk not in s.windows, "a plain ticket got a window"
            continue
        ws = s.windows[tk]
        _check_cover(ws, _total(lims[tk]))
        for _, slot, n, s0, s1, final in ws[:-1]:
            assert slot is not None and n < lims[tk]
            if k == "exact":
                assert s1 <= voc.settled_samples(n, HOP, HALO), "an exact window reaches past the settled samples"
                assert s1 - s0 >= 8 * 2 * HOP
            else:
                assert s1 <= _total(n) and s1 - s0 <= b.stream_speed
        if lims[tk] >= 120:
            assert len(ws) >= 3, f"a {lims[tk]}-token {k} utterance streamed {len(ws) - 1} windows before its end"
    assert len(s.windows[6]) == 1                                # 3 tokens: only the final window


def test_eager_follows_infer_stream_rule():
    """infer(stream=True, continuous=True): a window once stream_batch new tokens exist, to the prefix's end, at most stream_speed samples"""
    b = _book(rows=1, stream_speed=3000)
    tk = b.submit(10, 1, limit=40, stream="eager")
    s = Script(b, {tk: (40, 1)}, gain=4)
    s.run()
    ws = s.windows[tk]
    _check_cover(ws, _total(40))
    seen = 0
    for _, _, n, s0, s1, final in ws[:-1]:
        assert n - seen >= 8 and s1 == min(s0 + 3000, _total(n))
        seen = n


def test_a_cancel_yields_a_final_window():
    b = _book(rows=2, out_slots=2)
    ends = {}
    for i in range(3):
        ends[b.submit(10, i, limit=150, stream="exact")] = (150, 1)
    s = Script(b, ends, gain=10)
    assert b.cancel(2) == "queued"                               # cancelled while queued: an empty final window
    for _ in range(9):
        s.step()
    assert b.cancel(0) == "seated"
    s.run()
    n0, c0 = s.done[0]
    assert c0 and 0 < n0 < 150
    _check_cover(s.windows[0], _total(n0))
    assert len(s.windows[0]) >= 2 and s.done[1] == (150, False)
    _check_cover(s.windows[1], _total(150))
    assert s.windows[2] == [(2, None, 0, 0, 0, True)] and s.done[2] == (0, True)


def test_a_first_token_eos_requeue_emits_nothing_twice():
    b = _book(rows=2)
    ends = {b.submit(10, 7, limit=130, stream="exact"): (130, 2), b.submit(10, 8, limit=130, stream="eager"): (130, 2)}
    s = Script(b, ends, gain=6)
    s.run(first_eos=(0, 1))
    for tk in (0, 1):
        assert b.utts.get(tk) is None and s.done[tk] == (130, False)
        _check_cover(s.windows[tk], _total(130))                 # from sample 0 once: the attempt that ended at once emitted nothing
        assert len(s.windows[tk]) >= 3


def test_refusals():
    b = SessionBook(4, 6, 8, 64, 24, max_new_text=16)
    with pytest.raises(ValueError, match="stream= is for code utterances"):
        b.submit(10, 1, mode="text", stream="exact")
    with pytest.raises(ValueError, match="stream='now'"):
        b.submit(10, 1, stream="now")
    with pytest.raises(ValueError, match="stream_batch"):
        b.submit(10, 1, stream_batch=4)
    assert not b.utts and not b.queue
    for name in ("stream", "stream_batch"):
        assert "streaming windows" in SESSION_OUT_OF_SCOPE[name]
        with pytest.raises(_lib.HipBackendError, match="streaming windows.*per utterance at submit"):
            refuse_out_of_scope({name: True}, "use infer() for it")
    refuse_out_of_scope(dict(stream=False, stream_batch=None), "use infer() for it")


# ---- SynthSession: chunks under the public ticket (a scripted DecodeSession, as tests/test_text_rows_host.py drives it) ------------------------------------------
def test_synth_session_delivers_chunks_under_the_public_ticket():
    import types

    import torch

    from chatttsplus_amd.hip_models.gpt import SessionWindow
    from chatttsplus_amd.pipeline import SessionChunk, SessionDetails
    from tests.test_text_rows_host import _code_result, _session, _text_result
    ses, fake, _, _ = _session()
    plain_submit, asked, due = fake.submit, [], []

    def submit(emb, mask, utt_id, stream=None, stream_batch=None, stream_hidden=True, **kw):
        asked.append((utt_id, kw.get("mode", "code"), stream, stream_batch, stream_hidden))
        return plain_submit(emb, mask, utt_id, **kw)
    fake.submit = submit
    fake.take_windows = lambda: [due.pop(0) for _ in range(len(due))]
    calls = []

    def synth_windows(srcs, skips, counts, pcm16=False):
        calls.append((list(skips), list(counts), pcm16))
        return [torch.full((c,), float(i), dtype=torch.int16 if pcm16 else torch.float32) for i, c in enumerate(counts)]
    ses.pipe.synth = types.SimpleNamespace(cfg=types.SimpleNamespace(hop=256), synth_windows=synth_windows)
    a = ses.submit("hello", utt_id=1, stream="exact", stream_batch=8)      # refined first: the text stage streams nothing
    b = ses.submit("plain", utt_id=2, refine=False)
    c = ses.submit("pcm", utt_id=3, refine=False, stream="eager", pcm16=True)
    d = ses.submit("gone", utt_id=4, stream="exact")
    assert asked == [(1, "text", None, None, True), (2, "code", None, None, True), (3, "code", "eager", None, True), (4, "text", None, None, True)]
    for bad in (dict(stream="x"), dict(pcm16=True), dict(stream_batch=4), dict(stream="exact", stream_batch=0)):
        with pytest.raises(_lib.HipBackendError):
            ses.submit("t", **bad)
    assert ses.cancel(d)
    fake.script = [[_text_result(a, [7, 8]), _text_result(d, [5], cancelled=True)]]
    out = ses.poll()
    assert [(t, type(x), int(x.wav.shape[0]), x.final, cn) for t, x, cn in out] == [(d, SessionChunk, 0, True, True)]
    assert asked[-1] == (1, "code", "exact", 8, True)
    code_a = fake.submits[-1]["ticket"]
    hid = torch.zeros(200, 8)
    # one step: a window of each streaming ticket is due, nothing finished
    due += [SessionWindow(code_a, 70, 0, 8448, False, 0, torch.zeros(70, 4, dtype=torch.int32), hid[:70]),
            SessionWindow(c, 24, 0, 12000, False, 0, torch.zeros(24, 4, dtype=torch.int32), hid[:24], mode="eager")]
    fake.script = [[]]
    out = ses.poll()
    assert [(t, x.start, int(x.wav.shape[0]), x.final, x.n_tokens, x.wav.dtype, cn) for t, x, cn in out] == \
        [(a, 0, 8448, False, 70, torch.float32, False), (c, 0, 12000, False, 24, torch.int16, False)]
    assert calls == [([0], [8448], False), ([0], [12000], True)], "one call per sample format, the windows of a format together"
    # the last step: the finals come with the results; the plain utterance goes through the usual batched call
    due += [SessionWindow(code_a, 90, 8448, 256 * 179, True, 10, torch.zeros(80, 4, dtype=torch.int32), hid[10:90]),
            SessionWindow(c, 30, 12000, 256 * 59, True, 0, torch.zeros(30, 4, dtype=torch.int32), hid[:30], mode="eager")]
    fake.script = [[_code_result(code_a, 90), _code_result(b, 2), _code_result(c, 30, cancelled=True)]]
    out = {t: (x, cn) for t, x, cn in ses.drain()}
    assert sorted(out) == [a, b, c]
    assert calls[-2:] == [([8448 - 2 * 10 * 256], [256 * 179 - 8448], False), ([12000], [256 * 59 - 12000], True)]
    xa, xc = out[a][0], out[c][0]
    assert xa.final and xa.start == 8448 and xa.wav.shape[0] == 256 * 179 - 8448 and isinstance(xa.details, SessionDetails) and xa.details.refined_text == "w7 w8"
    assert xc.final and out[c][1] and xc.wav.dtype == torch.int16 and xc.start == 12000
    assert isinstance(out[b][0], SessionDetails) and out[b][0].wav.shape[0] == 6 and not out[b][1]
    assert not ses._streams and not ses._refining and not ses._public
