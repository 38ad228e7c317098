"""Serving session, host side (no GPU): the bookkeeping of GPT.open_session (SessionBook next to RowBook) against scripted row reports, and the two ABI
symbols' declaration, binding and documentation."""
import os
import re

import pytest

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import RowBook, SessionBook, compact_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE, LIMIT, EOS_END = 0, 1, 3           # RowState.fin as rows_enqueue reports it


def _book(rows=6, out_slots=12, max_batch=8, **kw):
    return SessionBook(rows, out_slots, max_batch, max_seq=64, max_new_token=24, **kw)


def _states(book, fin=None):
    """a row report of the current layout: every row live after 3 tokens unless `fin` = {row: (fin, end)} says otherwise; free rows report finished"""
    lay = book.book.layout()
    return lay, [(fin or {}).get(r, (LIVE, 3) if tk is not None else (LIMIT, 0)) for r, tk in enumerate(lay)]


def test_first_plan_begins_with_what_is_queued_and_rows_equal_slots():
    b = _book(rows=3)
    assert not b.plan() and not b.begun and b.idle()
    tk = [b.submit(10, 100 + i) for i in range(5)]
    p = b.plan()
    assert p.begin == [(0, tk[0]), (1, tk[1]), (2, tk[2])] and not p.grow and not p.admit and p.compact is None
    assert b.begun and b.lanes == [0, 1, 2] and b.queue == tk[3:]
    assert [b.utts[t]["slot"] for t in tk[:3]] == [0, 1, 2]      # ctts_gpt_begin writes row r's outputs at index r
    assert not b.plan(), "three rows, all live: the queue waits"
    assert b.n_live() == 3 and not b.idle()


def test_grow_admit_then_compact_decisions():
    b = _book(rows=6)
    tk = [b.submit(8, i) for i in range(2)]
    assert len(b.plan().begin) == 2
    tk += [b.submit(8, i) for i in range(2, 7)]
    p = b.plan()                                       # no free row: the batch grows to its bound of 6, one utterance keeps waiting
    assert p.grow == 4 and p.lanes == [2, 3, 4, 5] and p.admit == [(2, tk[2]), (3, tk[3]), (4, tk[4]), (5, tk[5])]
    assert b.queue == [tk[6]] and b.lanes == [0, 1, 2, 3, 4, 5]
    # rows 1 and 4 finish: the queued utterance takes a free row first, nothing grows
    lay, st = _states(b, {1: (LIMIT, 24), 4: (EOS_END, 7)})
    done = b.report(lay, st)
    assert sorted((t, n, f) for t, n, f, c in done) == [(tk[1], 24, LIMIT), (tk[4], 7, EOS_END)] and not any(c for *_, c in done)
    p = b.plan()
    assert p.grow == 0 and p.admit == [(1, tk[6])] and p.compact is None
    # nothing queued, 5 of 6 rows live: compact_size keeps 5
    for t, *_ in done:
        b.release(t)
    p = b.plan()
    assert p.compact == [0, 1, 2, 3, 5] and compact_size(5) == 5
    assert b.lanes == [0, 1, 2, 3, 5] and len(b.book.row_tk) == 5
    assert not b.plan()


def test_free_lane_mirror_after_compaction():
    """rows holding lanes 1 and 3 survive a compaction: the grown rows get lanes 0, 2, 4 -- lowest free first, not B .."""
    b = _book(rows=8)
    tk = [b.submit(8, i) for i in range(4)]
    b.plan()
    lay, st = _states(b, {0: (LIMIT, 4), 2: (LIMIT, 4)})
    for t, *_ in b.report(lay, st):
        b.release(t)
    assert b.plan().compact == [1, 3] and b.lanes == [1, 3]
    assert b.free_lanes()[:3] == [0, 2, 4]
    new = [b.submit(8, 10 + i) for i in range(3)]
    p = b.plan()
    assert p.grow == 3 and p.lanes == [0, 2, 4] and p.admit == [(2, new[0]), (3, new[1]), (4, new[2])]
    assert b.lanes == [1, 3, 0, 2, 4]


def test_out_slots_are_recycled_only_after_release():
    b = _book(rows=4, out_slots=3)
    tk = [b.submit(8, i) for i in range(5)]
    assert len(b.plan().begin) == 3 and b.free_slots == []
    assert not b.plan(), "no output slot is free: the queue waits although the batch could grow"
    lay, st = _states(b, {1: (LIMIT, 9)})
    done = b.report(lay, st)
    assert [(t, n) for t, n, *_ in done] == [(tk[1], 9)] and b.utts[tk[1]]["slot"] == 1
    assert not b.plan(), "the finished utterance's result has not been cloned out yet"
    b.release(tk[1])
    p = b.plan()
    assert p.admit == [(1, tk[3])] and b.utts[tk[3]]["slot"] == 1 and b.queue == [tk[4]]
    assert tk[1] not in b.utts


def test_cancel_of_queued_and_of_seated_tickets():
    b = _book(rows=2)
    tk = [b.submit(8, i) for i in range(4)]
    b.plan()
    assert b.cancel(tk[3]) == "queued" and b.queue == [tk[2]]
    assert b.cancel(tk[3]) is None and b.cancel(999) is None
    assert b.take_dropped() == [tk[3]] and b.take_dropped() == []
    assert b.cancel(tk[1]) == "seated"
    assert b.cancel_rows() == [1] and b.cancel_rows() == [], "the device is told once"
    # a report enqueued before the cancel still shows the row live; the next one shows it finished without EOS, short of its limit
    lay, st = _states(b)
    assert b.report(lay, st) == []
    lay, st = _states(b, {1: (LIMIT, 5)})
    assert b.report(lay, st) == [(tk[1], 5, LIMIT, True)]
    # an utterance that reached its limit (or EOS) before the cancel landed is a completed one
    assert b.cancel(tk[0]) == "seated"
    lay, st = _states(b, {0: (LIMIT, 24)})
    assert b.report(lay, st) == [(tk[0], 24, LIMIT, False)]
    b.release(tk[0]); b.release(tk[1]); b.release(tk[3])
    assert b.plan().admit == [(0, tk[2])]
    # cancelled right after being seated, before any step: the row is named, the result is empty
    assert b.cancel(tk[2]) == "seated" and b.cancel_rows() == [0]
    lay, st = _states(b, {0: (LIMIT, 0)})
    assert b.report(lay, st) == [(tk[2], 0, LIMIT, True)]


def test_first_token_eos_goes_back_to_the_head_of_the_queue():
    b = _book(rows=2, out_slots=2)
    tk = [b.submit(8, i) for i in range(3)]
    b.plan()
    lay, st = _states(b, {0: (EOS_END, 0)})
    assert b.report(lay, st) == [] and b.queue == [tk[0], tk[2]] and b.utts[tk[0]]["attempt"] == 1
    assert b.free_slots == [0], "a re-queued utterance holds no slot"
    p = b.plan()
    assert p.admit == [(0, tk[0])] and b.utts[tk[0]]["slot"] == 0
    # without ensure_non_empty the empty result is delivered
    b2 = _book(rows=2, ensure_non_empty=False)
    t = b2.submit(8, 0)
    b2.plan()
    lay, st = _states(b2, {0: (EOS_END, 0)})
    assert b2.report(lay, st) == [(t, 0, EOS_END, False)]
    # a cancelled utterance is not served again
    b3 = _book(rows=2)
    t = b3.submit(8, 0)
    b3.plan()
    b3.cancel(t)
    lay, st = _states(b3, {0: (EOS_END, 0)})
    assert b3.report(lay, st) == [(t, 0, 1, True)] and b3.queue == []


def test_stale_report_cannot_finish_a_rows_new_occupant():
    b = _book(rows=1)
    t0, t1 = b.submit(8, 0), b.submit(8, 1)
    b.plan()
    old = _states(b, {0: (LIMIT, 6)})
    again = _states(b, {0: (LIMIT, 6)})                # the same row state, enqueued one chunk later
    assert [t for t, *_ in b.report(*old)] == [t0]
    b.release(t0)
    assert b.plan().admit == [(0, t1)]
    assert b.report(*again) == [] and b.n_live() == 1
    assert isinstance(b.book, RowBook)


def test_prompt_that_does_not_fit_is_refused_at_submit():
    b = _book()
    with pytest.raises(ValueError, match=r"prompt of 41 tokens \+ max_new_token=24 exceed max_seq_len=64"):
        b.submit(41, 0)
    assert b.submit(40, 0) == 0 and b.utts[0]["limit"] == 24
    assert b.utts[b.submit(8, 1, limit=99)]["limit"] == 24 and b.utts[b.submit(8, 2, limit=0)]["limit"] == 1
    with pytest.raises(ValueError):
        SessionBook(9, 4, 8, 64, 24)


# -- the request policy (generate_many drives the same book): own_slots and admit_min.  The expected plans are worked out by hand from the rule in SessionBook's
#    docstring: queued utterances are seated only if len(free) >= min(admit_min, queued), since_free >= 4 or len(free) == B.
def _finish(b, rows, n=5):
    """rows `rows` report their limit after n tokens; the results are released"""
    done = b.report(*_states(b, {r: (LIMIT, n) for r in rows}))
    for t, *_ in done:
        b.release(t)
    return [t for t, *_ in done]


def test_own_slots_10_tickets_on_4_rows_open_at_4_and_never_grow():
    b = _book(rows=4, out_slots=10, own_slots=True)
    tk = [b.submit(8, 100 + i) for i in range(10)]
    p = b.plan()
    assert p.begin == [(r, tk[r]) for r in range(4)] and b.lanes == [0, 1, 2, 3] and b.queue == tk[4:]
    assert not b.plan(), "no free row: the queue waits, the batch does not grow"
    assert _finish(b, [1]) == [tk[1]]
    p = b.plan()
    assert p.admit == [(1, tk[4])] and p.grow == 0 and p.compact is None
    assert sorted(_finish(b, [0, 2, 3])) == [tk[0], tk[2], tk[3]]
    p = b.plan()
    assert p.admit == [(0, tk[5]), (2, tk[6]), (3, tk[7])] and p.grow == 0
    assert sorted(_finish(b, [0, 1, 2, 3])) == tk[4:8]
    p = b.plan()
    assert p.admit == [(0, tk[8]), (1, tk[9])] and p.grow == 0 and len(b.book.row_tk) == 4 and b.queue == []
    # ticket k wrote slot k throughout, no slot was ever recycled, and only the empty queue lets the batch shrink
    assert [b.utts[t]["slot"] for t in tk[8:]] == tk[8:] and b.free_slots == []
    assert b.plan().compact == [0, 1] and b.lanes == [0, 1]
    assert tk == list(range(10))


def test_admit_min_holds_one_free_row_for_three_plans():
    b = _book(rows=4, out_slots=8, own_slots=True, admit_min=2)
    tk = [b.submit(8, i) for i in range(8)]
    assert len(b.plan().begin) == 4
    _finish(b, [2])
    for held in range(3):                              # since_free = 1, 2, 3: one free row < min(admit_min = 2, 4 queued)
        p = b.plan()
        assert not p and p.compact is None and b.queue == tk[4:], f"plan {held + 1} after the row fell free: held back, empty, no compaction"
    assert b.plan().admit == [(2, tk[4])], "the fourth plan that saw the free row seats it (since_free = 4)"
    # two free rows reach admit_min: at once
    _finish(b, [0, 1])
    assert b.plan().admit == [(0, tk[5]), (1, tk[6])]
    # one utterance left in the queue: min(admit_min, queued) = 1, one free row is enough
    _finish(b, [3])
    assert b.plan().admit == [(3, tk[7])] and b.queue == []
    # the counter starts over after an admission: a row that falls free now is held for three plans again
    b2 = _book(rows=2, out_slots=8, own_slots=True, admit_min=2)
    t2 = [b2.submit(8, i) for i in range(8)]
    b2.plan()
    _finish(b2, [0])
    assert [bool(b2.plan()) for _ in range(4)] == [False, False, False, True]
    _finish(b2, [1])
    assert [bool(b2.plan()) for _ in range(4)] == [False, False, False, True] and b2.queue == t2[4:]


def test_admit_min_every_row_free_admits_at_once():
    b = _book(rows=2, out_slots=6, own_slots=True, admit_min=3)
    tk = [b.submit(8, i) for i in range(6)]
    b.plan()
    _finish(b, [0, 1])                                 # 2 free rows < min(3, 4 queued), first plan to see them -- but they are the whole batch
    assert b.plan().admit == [(0, tk[2]), (1, tk[3])]


def test_own_slots_first_token_eos_returns_to_its_own_slot():
    b = _book(rows=2, out_slots=4, own_slots=True)
    tk = [b.submit(8, i) for i in range(4)]
    b.plan()
    _finish(b, [1])
    assert b.plan().admit == [(1, tk[2])]
    _finish(b, [0])
    assert b.plan().admit == [(0, tk[3])]             # rows now hold tickets (3, 2): row order and slot order differ
    assert b.report(*_states(b, {0: (EOS_END, 0), 1: (EOS_END, 0)})) == []
    assert b.queue == [tk[3], tk[2]], "back at the head of the queue, in row order"
    assert [b.utts[t]["attempt"] for t in (tk[2], tk[3])] == [1, 1] and b.free_slots == []
    p = b.plan()
    assert p.admit == [(0, tk[3]), (1, tk[2])]
    assert b.utts[tk[3]]["slot"] == tk[3] and b.utts[tk[2]]["slot"] == tk[2], "each returns to its own output index"
    # the session's recycled slots would have handed them out lowest first
    s = _book(rows=2, out_slots=4)
    for i in range(4):
        s.submit(8, i)
    s.plan()
    _finish(s, [1]); s.plan(); _finish(s, [0]); s.plan()
    s.report(*_states(s, {0: (EOS_END, 0), 1: (EOS_END, 0)}))
    s.plan()
    assert (s.utts[3]["slot"], s.utts[2]["slot"]) == (0, 1)


def test_report_exposes_the_live_rows_token_counts():
    b = _book(rows=3, own_slots=True, out_slots=3)
    tk = [b.submit(8, i) for i in range(3)]
    b.plan()
    b.report(*_states(b, {0: (LIVE, 7), 1: (LIMIT, 9), 2: (LIVE, 0)}))
    assert b.live == [(tk[0], 7), (tk[2], 0)]


def test_admit_min_1_without_own_slots_reproduces_every_plan_above(monkeypatch):
    """the session's policy, named explicitly: the tests of the default book pass unchanged"""
    import functools
    import sys
    monkeypatch.setattr(sys.modules[__name__], "_book", functools.partial(_book, admit_min=1, own_slots=False))
    for test in (test_first_plan_begins_with_what_is_queued_and_rows_equal_slots, test_grow_admit_then_compact_decisions, test_free_lane_mirror_after_compaction,
                 test_out_slots_are_recycled_only_after_release, test_cancel_of_queued_and_of_seated_tickets, test_first_token_eos_goes_back_to_the_head_of_the_queue,
                 test_stale_report_cannot_finish_a_rows_new_occupant, test_prompt_that_does_not_fit_is_refused_at_submit):
        test()


def test_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    assert re.search(r"int ctts_gpt_grow\(ctts_gpt\* h, int n, void\* stream\);", header)
    assert re.search(r"int ctts_gpt_cancel\(ctts_gpt\* h, int n, const int32_t\* rows_host, void\* stream\);", header)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "ctts_gpt_grow" in bound and len(bound["ctts_gpt_grow"][1]) == 3
    assert "ctts_gpt_cancel" in bound and len(bound["ctts_gpt_cancel"][1]) == 4
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`ctts_gpt_grow`" in doc and "`ctts_gpt_cancel`" in doc
