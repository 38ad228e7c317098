"""Text rows beside code rows, host side (no GPU): SessionBook with utterance modes against scripted row reports, the refine -> code chaining of SynthSession
against a fake DecodeSession, and the three ABI symbols' declaration, binding and documentation."""
import os
import re
import types

import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import SESSION_OUT_OF_SCOPE, SessionBook, SessionResult, refuse_out_of_scope, text_rows_cfg
from chatttsplus_amd.pipeline import InferCodeParams, RefineTextParams, SessionDetails, SynthSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE, LIMIT, EOS_END = 0, 1, 3           # RowState.fin as rows_enqueue reports it


def _book(rows=4, out_slots=6, max_batch=8, **kw):
    return SessionBook(rows, out_slots, max_batch, max_seq=64, max_new_token=24, max_new_text=16, **kw)


def _states(book, fin=None):
    lay = book.book.layout()
    return lay, [(fin or {}).get(r, (LIVE, 3) if tk is not None else (LIMIT, 0)) for r, tk in enumerate(lay)]


# ---- SessionBook ------------------------------------------------------------------------------------------------------------------------------------------
def test_mode_defaults_to_code_and_text_needs_a_text_limit():
    b = SessionBook(4, 6, 8, 64, 24)
    assert b.utts[b.submit(8, 1)]["mode"] == "code"
    with pytest.raises(ValueError, match='mode="text" needs a session opened with text_rows'):
        b.submit(8, 2, mode="text")
    with pytest.raises(ValueError, match="mode='speech'"):
        b.submit(8, 2, mode="speech")
    with pytest.raises(ValueError, match=r"text rows' max_new_token=25 must be 1..max_new_token=24"):
        SessionBook(4, 6, 8, 64, 24, max_new_text=25)
    assert SessionBook(4, 6, 8, 64, 24, max_new_text=24).max_new_text == 24


def test_text_and_code_utterances_queue_together_and_share_slots():
    b = _book(rows=4, out_slots=3)
    tk = [b.submit(8, 10, mode="text"), b.submit(9, 11), b.submit(8, 12, mode="text", limit=99), b.submit(8, 13, limit=99), b.submit(8, 14, mode="text", limit=5)]
    assert [b.utts[t]["mode"] for t in tk] == ["text", "code", "text", "code", "text"]
    assert [b.utts[t]["limit"] for t in tk] == [16, 24, 16, 24, 5], "a text utterance's limit is the text rows' own"
    p = b.plan()                                       # one queue, one slot space: three slots for five utterances of either kind
    assert p.begin == [(0, tk[0]), (1, tk[1]), (2, tk[2])] and [b.utts[t]["slot"] for t in tk[:3]] == [0, 1, 2]
    assert b.queue == tk[3:] and not b.plan(), "no free slot: the queue waits whatever the mode"
    # the text utterance of row 0 ends: its slot is recycled by the next utterance in line, a code one, after release
    lay, st = _states(b, {0: (LIMIT, 16)})
    done = b.report(lay, st)
    assert done == [(tk[0], 16, LIMIT, False)]
    assert not b.plan(), "the slot is held until the result has been cloned out"
    b.release(tk[0])
    p = b.plan()
    assert p.admit == [(0, tk[3])] and b.utts[tk[3]]["slot"] == 0 and b.utts[tk[3]]["mode"] == "code"
    lay, st = _states(b, {1: (EOS_END, 7)})
    for t, *_ in b.report(lay, st):
        b.release(t)
    p = b.plan()
    assert p.admit == [(1, tk[4])] and b.utts[tk[4]]["slot"] == 1 and b.utts[tk[4]]["mode"] == "text"


def test_first_token_eos_requeues_with_its_mode():
    b = _book(rows=2)
    t_text, t_code = b.submit(8, 1, mode="text"), b.submit(8, 2)
    assert len(b.plan().begin) == 2
    lay, st = _states(b, {0: (EOS_END, 0), 1: (EOS_END, 0)})
    assert b.report(lay, st) == [] and b.queue == [t_text, t_code]
    assert (b.utts[t_text]["attempt"], b.utts[t_text]["mode"], b.utts[t_text]["limit"]) == (1, "text", 16)
    assert (b.utts[t_code]["attempt"], b.utts[t_code]["mode"], b.utts[t_code]["limit"]) == (1, "code", 24)
    p = b.plan()
    assert p.admit == [(0, t_text), (1, t_code)]
    # without ensure_non_empty an empty text utterance is delivered as it is
    b = _book(rows=1, ensure_non_empty=False)
    t = b.submit(8, 1, mode="text")
    b.plan()
    assert b.report(*_states(b, {0: (EOS_END, 0)})) == [(t, 0, EOS_END, False)]


def test_cancel_of_a_text_utterance_queued_and_seated():
    b = _book(rows=1)
    seated, queued = b.submit(8, 1, mode="text"), b.submit(8, 2, mode="text")
    b.plan()
    assert b.cancel(queued) == "queued" and b.take_dropped() == [queued] and b.utts[queued]["mode"] == "text"
    assert b.cancel(seated) == "seated" and b.cancel_rows() == [0] and b.cancel(seated) is None
    assert b.report(*_states(b, {0: (LIMIT, 4)})) == [(seated, 4, LIMIT, True)]


def test_out_of_scope_names_keep_their_messages():
    for name in ("infer_text", "refine_text_only", "params_refine_text"):
        assert SESSION_OUT_OF_SCOPE[name] == "the refine-text pass inside a code session"
        with pytest.raises(_lib.HipBackendError, match="refine-text pass inside a code session"):
            refuse_out_of_scope({name: True}, "x")
    assert "text_rows" not in SESSION_OUT_OF_SCOPE and "refine" not in SESSION_OUT_OF_SCOPE


def test_text_rows_cfg():
    sc = text_rows_cfg(dict(temperature=0.5, top_P=0.6, top_K=10, eos_token=21177, max_new_token=16, min_new_token=2))
    assert sc.infer_text == 1 and sc.use_penalty == 0 and sc.eos_token == 21177 and sc.max_new_token == 16 and sc.min_new_token == 2 and sc.top_k == 10
    assert abs(sc.temperature[0] - 0.5) < 1e-7
    obj = RefineTextParams(max_new_token=12)
    obj.eos_token = 7
    assert text_rows_cfg(obj).max_new_token == 12 and text_rows_cfg(obj).top_k == 20
    with pytest.raises(_lib.HipBackendError, match="unknown key"):
        text_rows_cfg(dict(eos_token=1, max_new_token=2, repetition_penalty=1.1))
    with pytest.raises(_lib.HipBackendError, match="needs eos_token"):
        text_rows_cfg(dict(max_new_token=2))


# ---- SynthSession: refine -> code under one ticket ------------------------------------------------------------------------------------------------------------
class FakeDecode:
    """records what SynthSession asks of a DecodeSession; step() hands back what the test scripted"""

    def __init__(self):
        self.submits, self.cancels, self.script, self._next, self.live = [], [], [], 0, set()
        self.book = types.SimpleNamespace(idle=lambda: not self.live)
        self.batch_trace = []

    def submit(self, emb, mask, utt_id, limit=None, sampling=None, adapter_slot=None, mode="code"):
        tk, self._next = self._next, self._next + 1
        self.submits.append(dict(ticket=tk, utt_id=utt_id, limit=limit, sampling=sampling, adapter_slot=adapter_slot, mode=mode, T=int(emb.shape[0])))
        self.live.add(tk)
        return tk

    def cancel(self, tk):
        self.cancels.append(tk)
        return tk in self.live

    def step(self):
        out = self.script.pop(0) if self.script else []
        self.live -= {r.ticket for r in out}
        return out

    def close(self):
        pass


class FakeTok:
    eos_token, break_0_ids, spk_emb_ids = 99, 50, 3

    def decode(self, ids):
        return [" ".join(f"w{int(i)}" for i in x) for x in ids]


def _session(refine=RefineTextParams(max_new_token=16, show_tqdm=False), return_details=True):
    fake = FakeDecode()
    opened = {}

    def open_session(*a, **kw):
        opened.update(kw)
        return fake

    G = type("G", (), dict(__call__=lambda self, i, m, **kw: torch.zeros(i.shape[0], i.shape[1], 8), open_session=staticmethod(open_session), num_vq=4,
                           emb_code=[types.SimpleNamespace(num_embeddings=626)]))
    prompts = []

    def enc(kind):
        def f(text, *a, **kw):
            prompts.append((kind, list(text)))
            T = 5 if kind == "refine" else 7
            return torch.zeros(1, T, 4, dtype=torch.long), torch.ones(1, T, dtype=torch.bool), torch.ones(1, T, dtype=torch.bool)
        return f
    pipe = types.SimpleNamespace(normalizer=lambda t, *a: t.strip(), models_dict=dict(tokenizer=FakeTok()), device="cpu", _refine_prompt=enc("refine"),
                                 _code_prompt=enc("code"), _decode_to_wavs=lambda srcs, dec: [torch.ones(3 * int(s.shape[0])) for s in srcs])
    params = InferCodeParams(max_new_token=24, spk_emb=torch.zeros(8), show_tqdm=False)
    ses = SynthSession(pipe, G(), params, True, 4, 1, return_details, refine=refine)
    return ses, fake, opened, prompts


def _text_result(tk, ids, cancelled=False):
    return SessionResult(ticket=tk, utt_id=0, ids=torch.tensor(ids, dtype=torch.long), cancelled=cancelled, mode="text")


def _code_result(tk, n, cancelled=False):
    return SessionResult(ticket=tk, utt_id=0, ids=torch.zeros(n, 4, dtype=torch.long), hiddens=torch.zeros(n, 8), logprobs=torch.zeros(n, 4), sampled_logprobs=torch.zeros(n, 4),
                         cancelled=cancelled)


def test_synth_session_chains_refine_into_code_under_one_ticket():
    ses, fake, opened, prompts = _session()
    assert opened["text_rows"] == dict(temperature=0.7, top_P=0.7, top_K=20, eos_token=99, max_new_token=16, min_new_token=0)
    a = ses.submit(" hello ", utt_id=41)
    b = ses.submit("plain", utt_id=42, refine=False, max_new_token=9)
    assert [(s["mode"], s["utt_id"], s["T"], s["limit"]) for s in fake.submits] == [("text", 41, 5, None), ("code", 42, 7, 9)]
    assert prompts == [("refine", ["hello"]), ("code", ["plain [uv_break]"])]
    # the text row delivers ids 7, 60 (>= break_0_ids: filtered, as infer does), 8: nothing is returned, the code utterance is submitted under the same utterance id
    fake.script = [[_text_result(a, [7, 60, 8])]]
    assert ses.poll() == []
    assert prompts[-1] == ("code", ["w7 w8 [uv_break]"])
    code_tk = fake.submits[-1]["ticket"]
    assert (fake.submits[-1]["mode"], fake.submits[-1]["utt_id"]) == ("code", 41) and code_tk != a
    assert not fake.book.idle()
    fake.script = [[_code_result(code_tk, 4), _code_result(b, 2)]]
    out = {t: (d, c) for t, d, c in ses.drain()}
    assert sorted(out) == [a, b], "the refined utterance is delivered under the ticket submit() returned"
    assert isinstance(out[a][0], SessionDetails) and out[a][0].refined_text == "w7 w8" and out[a][0].wav.shape[0] == 12 and not out[a][1]
    assert out[b][0].refined_text is None and out[b][0].wav.shape[0] == 6
    assert not ses._refining and not ses._public and not ses._code_tk and not ses._refined


def test_synth_session_cancel_in_either_stage():
    ses, fake, _, prompts = _session(return_details=False)
    a, b = ses.submit("one", utt_id=1), ses.submit("two", utt_id=2)
    # a: cancelled during its refine stage -> an empty waveform, cancelled=True, no code stage
    assert ses.cancel(a) and not ses.cancel(a) and fake.cancels == [a]
    fake.script = [[_text_result(a, [5], cancelled=True), _text_result(b, [6])]]
    out = ses.poll()
    assert [(t, int(w.shape[0]), c) for t, w, c in out] == [(a, 0, True)]
    assert [s["mode"] for s in fake.submits] == ["text", "text", "code"] and fake.submits[-1]["utt_id"] == 2
    # b: cancelled during its code stage -> the engine's cancel is asked for the code-stage ticket, the result comes back under b
    code_tk = fake.submits[-1]["ticket"]
    assert ses.cancel(b) and fake.cancels[-1] == code_tk
    fake.script = [[_code_result(code_tk, 3, cancelled=True)]]
    assert [(t, int(w.shape[0]), c) for t, w, c in ses.poll()] == [(b, 9, True)]
    # a session opened without refine: refine=True at submit is refused, the default does not refine
    ses, fake, opened, _ = _session(refine=None)
    assert opened["text_rows"] is None
    with pytest.raises(_lib.HipBackendError, match="refine=True needs a session opened with refine="):
        ses.submit("x", refine=True)
    ses.submit("x")
    assert [s["mode"] for s in fake.submits] == ["code"]
    with pytest.raises(_lib.HipBackendError, match="repetition_penalty must be 1"):
        _session(refine=RefineTextParams(repetition_penalty=1.2))


def test_a_refused_code_stage_ends_its_utterance_and_loses_no_other_result():
    """the code prompt of a refined text may no longer fit (DecodeSession.submit refuses it): that ticket is delivered empty with cancelled=True and the reason on
    record; the other results of the same step are delivered"""
    ses, fake, _, _ = _session()
    a, b, c = ses.submit("one", utt_id=1), ses.submit("two", utt_id=2, refine=False), ses.submit("three", utt_id=3)
    submit = fake.submit

    def refusing(emb, mask, utt_id, **kw):
        if utt_id == 1:
            raise _lib.HipBackendError("submit: prompt of 99 tokens + max_new_token=24 exceed max_seq_len=64")
        return submit(emb, mask, utt_id, **kw)
    fake.submit = refusing
    fake.script = [[_text_result(a, [7, 8]), _code_result(b, 2), _text_result(c, [9])]]
    out = {t: (d, cn) for t, d, cn in ses.poll()}
    assert sorted(out) == [a, b] and out[a][1] and out[a][0].wav.shape[0] == 0 and out[a][0].refined_text == "w7 w8" and "exceed max_seq_len" in ses.failed[a]
    assert not out[b][1] and out[b][0].wav.shape[0] == 6
    assert fake.submits[-1]["utt_id"] == 3 and fake.submits[-1]["mode"] == "code", "the refine stage delivered behind the refused one was dropped"
    assert a not in ses._refining and a not in ses._refined


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    assert re.search(r"int ctts_gpt_enable_text_rows\(ctts_gpt\* h, const ctts_sampler_cfg\* text_sc, int32_t\* text_ids_dev, void\* stream\);", header)
    assert re.search(r"int ctts_gpt_set_row_modes\(ctts_gpt\* h, const int32_t\* modes, int B\);", header)
    assert re.search(r"int ctts_gpt_admit_modes\(ctts_gpt\* h, int n, const int32_t\* rows, const int32_t\* modes, void\* stream\);", header)
    assert "one mode at a time" not in header and '"text_rows_live"' in header
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert len(bound["ctts_gpt_enable_text_rows"][1]) == 4 and len(bound["ctts_gpt_set_row_modes"][1]) == 3 and len(bound["ctts_gpt_admit_modes"][1]) == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`ctts_gpt_enable_text_rows`" in doc and "`ctts_gpt_set_row_modes`" in doc and "`ctts_gpt_admit_modes`" in doc
    common = open(os.path.join(ROOT, "chatttsplus_amd", "csrc", "common.h")).read()
    assert re.search(r"int mode;", common) and "pad1" not in common
