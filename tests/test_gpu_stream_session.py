"""Streaming from a serving session (SynthSession.submit(stream="exact" | "eager"), DecodeSession.take_windows, ctts_synth_windows).  Synthetic weights at real
widths, 4 decoder layers (tests/test_gpu_score.py), the toy tokenizer and texts of tests/test_gpu_session.py's pipeline test.

The utterances run to their token limits: min_new_token equals the session's max_new_token, so EOS is never drawn and a limit of 60..140 is the length.
Checked: an "exact" ticket's chunks are consecutive and concatenate, bit for bit, to the vocoding of the delivered hidden rows and to the same text's batch-1
infer(stream=False) waveform (batch_invariant fp32 engine; a default-mode fp16 engine: against its own hidden rows only); every "eager" chunk is the slice of
the waveform of the prefix it reports; plain utterances beside them are what they are without any streaming ticket; a cancel ends a ticket with a final chunk
and the audio of the tokens written; refine -> stream under one ticket; the codes path; and at the DecodeSession level with out_slots == rows and a queue,
that the views a window hands out are written rows of the utterance's own slot."""
import pytest
import torch

from chatttsplus_amd import _lib, synth
from tests.test_gpu_score import CFG4, EOS, LLAMA4, engine

pytestmark = pytest.mark.gpu

INV = dict(batch_invariant=1)
MAX_NEW, SEED = 140, 5151
LIMS = [140, 120, 60, 130, 97, 125, 70, 140, 121, 88, 135, 64]
KINDS = ["exact", "exact", None, "eager", "exact", "exact", None, "eager", "exact", None, "exact", None]
CANCELLED = 0                                       # utterance 0 ("exact", limit 140) is cancelled once its first chunk has arrived


def _synth(max_batch=12, codes=False):
    from chatttsplus_amd.hip_models import Synth
    if codes:
        s = Synth(dict(synth.DVAE_FULL_DEC), dict(synth.VOCOS_REAL), max_frames=2 * MAX_NEW + 64, device="cuda:0", max_batch=max_batch,
                  vq_cfg=dict(dim=1024, levels=[5, 5, 5, 5], G=2, R=2))
        s.load("dvae.", synth.dvae_full_decoder_state_dict(synth.DVAE_FULL_DEC, 1234))
    else:
        s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * MAX_NEW + 64, device="cuda:0", max_batch=max_batch)
        s.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    s.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    return s


def _params(**kw):
    from chatttsplus_amd.pipeline import InferCodeParams
    return InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=MAX_NEW, min_new_token=MAX_NEW,
                           show_tqdm=False, spk_emb=torch.from_numpy(synth.speaker_vector(1234)).float(), **kw)


_state = {}


def _pipe(tmp_path_factory, dtype="fp32", options=INV):
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    key = (dtype, tuple(sorted((options or {}).items())))
    if key not in _state:
        if "syn" not in _state:
            _state["syn"] = _synth()
            _state["tok"] = synth.toy_tokenizer(str(tmp_path_factory.mktemp("tok")))
        g = engine(dtype, options, max_batch=10, max_seq=256)
        _state[key] = ChatTTSPlusPipeline.from_components(g, _state["syn"], _state["tok"], torch.device("cuda:0"))
    return _state[key]


def _texts():
    return synth.toy_texts(12, 8, 30, seed=68)


def _run(pipe, kinds, cancel=None, **open_kw):
    """The arrival schedule of every scenario here: 4 texts, three polls, then the other 8 (the batch grows 4 -> 10 rows, across the 8-row persistent limit and the
    9-row threshold, two wait in the queue).  -> per utterance dict(chunks=[SessionChunk], out=(wav, cancelled) of a plain one, res=SessionResult), batch_trace"""
    from chatttsplus_amd.pipeline import SessionChunk
    texts = _texts()
    rec = {u: dict(chunks=[], out=None, res=None, cancelled=False) for u in range(12)}
    with pipe.open_session(_params(), rows=10, seed=SEED, **open_kw) as ses:
        step, by_tk, tk_of = ses.session.step, {}, {}

        def spy():
            out = step()
            for r in out:
                rec[by_tk[ses._public.get(r.ticket, r.ticket)]]["res"] = r
            return out
        ses.session.step = spy

        def sub(u):
            t = ses.submit(texts[u], utt_id=u, max_new_token=LIMS[u], stream=kinds[u], stream_batch=8 if kinds[u] == "exact" else None)
            by_tk[t], tk_of[u] = u, t

        def take(out):
            for t, d, c in out:
                r = rec[by_tk[t]]
                if isinstance(d, SessionChunk):
                    assert not r["chunks"] or not r["chunks"][-1].final, "a chunk behind the final one"
                    r["chunks"].append(d)
                    r["cancelled"] = c
                else:
                    assert r["out"] is None
                    r["out"], r["cancelled"] = d, c
        for u in range(4):
            sub(u)
        for _ in range(3):
            take(ses.poll())
        for u in range(4, 12):
            sub(u)
        asked = False
        while not ses.session.book.idle():
            take(ses.poll())
            if cancel is not None and not asked and rec[cancel]["chunks"]:
                assert ses.cancel(tk_of[cancel])
                asked = True
        trace = list(ses.batch_trace)
    torch.cuda.synchronize()
    return rec, trace


def _concat(chunks):
    pos = 0
    for c in chunks:
        assert c.start == pos, f"chunk starts at sample {c.start}, the previous one ended at {pos}"
        pos += int(c.wav.shape[0])
    assert chunks[-1].final and not any(c.final for c in chunks[:-1])
    return torch.cat([c.wav for c in chunks])


@pytest.fixture(scope="module")
def main(tmp_path_factory):
    pipe = _pipe(tmp_path_factory)
    rec, trace = _run(pipe, KINDS, cancel=CANCELLED)
    return pipe, rec, trace


@pytest.fixture(scope="module")
def alone(tmp_path_factory):
    """every text through its own batch-1 infer(stream=False): (ids, wav) per utterance"""
    from chatttsplus_amd.pipeline import InferDetails
    pipe = _pipe(tmp_path_factory)
    out = []
    for u, t in enumerate(_texts()):
        d = list(pipe.infer([t], skip_refine_text=True, params_infer_code=_params(), noise="device", noise_seed=SEED, utt_ids=[u],
                            max_new_tokens_per_utterance=[LIMS[u]], return_details=True))
        assert len(d) == 1 and isinstance(d[0], InferDetails) and len(d[0].wavs) == 1
        out.append((d[0].ids[0].cpu(), d[0].wavs[0]))
    return out


def test_the_batch_crossed_the_persistent_limit_and_every_utterance_ran_to_its_limit(main):
    pipe, rec, trace = main
    print(f"batch_trace {trace}")
    sizes = [b for _, b in trace]
    assert sizes[0] == 4 and max(sizes) == 10
    for u in range(12):
        n = int(rec[u]["res"].ids.shape[0])
        assert (n == LIMS[u]) if u != CANCELLED else (0 < n < LIMS[u]), f"utterance {u}: {n} tokens, limit {LIMS[u]}"
        assert (rec[u]["out"] is None) == (KINDS[u] is not None) and bool(rec[u]["chunks"]) == (KINDS[u] is not None)
        assert rec[u]["cancelled"] == (u == CANCELLED)


def test_exact_chunks_concatenate_to_the_offline_waveform(main, alone):
    pipe, rec, _ = main
    for u in [u for u in range(12) if KINDS[u] == "exact" and u != CANCELLED]:
        ch = rec[u]["chunks"]
        wav = _concat(ch)
        print(f"utterance {u} (limit {LIMS[u]}): chunks of {[int(c.wav.shape[0]) for c in ch]} samples at tokens {[c.n_tokens for c in ch]}")
        if LIMS[u] >= 120:
            assert len(ch) >= 3, f"utterance {u}: {len(ch) - 1} chunks before the final one"
        ref = pipe._decode_to_wavs([rec[u]["res"].hiddens])[0]
        assert wav.shape == ref.shape == (256 * (2 * LIMS[u] - 1),)
        assert torch.equal(wav, ref), f"utterance {u}: the chunks are not the vocoding of the delivered hidden rows (max diff {float((wav - ref).abs().max())})"
        assert torch.equal(rec[u]["res"].ids.cpu(), alone[u][0]), f"utterance {u}: ids differ from its batch-1 infer"
        assert torch.equal(wav, alone[u][1]), f"utterance {u}: the chunks are not the batch-1 infer(stream=False) waveform"
        for c in ch[:-1]:
            assert c.start + int(c.wav.shape[0]) <= 256 * max(0, 2 * c.n_tokens - pipe.synth.HALO_FRAMES - 2)


def test_eager_chunks_are_slices_of_the_prefix_they_report(main):
    pipe, rec, _ = main
    for u in [u for u in range(12) if KINDS[u] == "eager"]:
        ch, hid = rec[u]["chunks"], rec[u]["res"].hiddens
        _concat(ch)
        if LIMS[u] >= 120:
            assert len(ch) >= 3
        differs = False
        whole = pipe.synth.decode_batch([hid])[0]
        for c in ch:
            assert 0 < c.n_tokens <= LIMS[u] and (c.n_tokens == LIMS[u]) == c.final
            pre = pipe.synth.decode_batch([hid[:c.n_tokens]])[0]
            k = int(c.wav.shape[0])
            assert torch.equal(c.wav, pre[c.start:c.start + k]), f"utterance {u}: the chunk at {c.start} is not a slice of its {c.n_tokens}-token prefix waveform"
            differs = differs or not torch.equal(c.wav, whole[c.start:c.start + k])
        assert differs, "every eager chunk equals the offline waveform: the prefixes were never shorter than the utterance"


def test_a_cancel_ends_the_ticket_with_the_audio_of_the_tokens_written(main, alone):
    pipe, rec, _ = main
    r = rec[CANCELLED]
    res, ch = r["res"], r["chunks"]
    n = int(res.ids.shape[0])
    assert res.cancelled and r["cancelled"] and len(ch) >= 2 and 0 < n < LIMS[CANCELLED]
    assert torch.equal(res.ids.cpu(), alone[CANCELLED][0][:n]), "the cancelled utterance's ids are not a prefix of its uncancelled run"
    wav = _concat(ch)
    assert wav.shape == (256 * (2 * n - 1),) and torch.equal(wav, pipe._decode_to_wavs([res.hiddens])[0])


def test_plain_utterances_are_what_they_are_without_streaming_tickets(main, tmp_path_factory):
    pipe, rec, _ = main
    rec0, _ = _run(pipe, [None] * 12)
    for u in [u for u in range(12) if KINDS[u] is None]:
        a, b = rec[u], rec0[u]
        assert torch.equal(a["res"].ids, b["res"].ids) and torch.equal(a["res"].hiddens, b["res"].hiddens) and torch.equal(a["out"], b["out"]), f"utterance {u}"
        assert a["out"].shape == (256 * (2 * LIMS[u] - 1),)
    for u in [u for u in range(12) if KINDS[u] == "exact" and u != CANCELLED]:      # ... and a streamed one is its own plain delivery
        assert torch.equal(_concat(rec[u]["chunks"]), rec0[u]["out"])


def test_pcm16_chunks_and_details(tmp_path_factory):
    from chatttsplus_amd.pipeline import SessionChunk, SessionDetails
    pipe = _pipe(tmp_path_factory)
    texts = _texts()
    got = {}
    with pipe.open_session(_params(), rows=4, seed=SEED, return_details=True) as ses:
        a = ses.submit(texts[1], utt_id=1, max_new_token=LIMS[1], stream="exact", stream_batch=8, pcm16=True)
        b = ses.submit(texts[1], utt_id=1, max_new_token=LIMS[1], stream="exact", stream_batch=8)
        c = ses.submit(texts[2], utt_id=2, max_new_token=LIMS[2], stream="exact")
        assert ses.cancel(c)                                              # still queued: one empty final chunk
        for t, d, cn in ses.drain():
            got.setdefault(t, []).append((d, cn))
        with pytest.raises(_lib.HipBackendError, match="belong to a streaming utterance"):
            ses.submit(texts[0], pcm16=True)
        with pytest.raises(_lib.HipBackendError, match="stream='x'"):
            ses.submit(texts[0], stream="x")
    assert [(int(d.wav.shape[0]), d.final, cn) for d, cn in got[c]] == [(0, True, True)]
    pa, pb = [d for d, _ in got[a]], [d for d, _ in got[b]]
    assert all(isinstance(d, SessionChunk) for d in pa + pb) and len(pa) == len(pb) >= 3
    assert all(d.details is None for d in pa[:-1]) and isinstance(pa[-1].details, SessionDetails) and pa[-1].details.ids.shape[0] == LIMS[1]
    f, p = _concat(pb), _concat(pa)
    assert p.dtype == torch.int16 and torch.equal(p, torch.clamp(f, -1, 1).mul(32767).round().to(torch.int16))


def test_codes_path(tmp_path_factory):
    pipe = _pipe(tmp_path_factory)
    if getattr(pipe, "synth_codes", None) is None:
        pipe.synth_codes = _synth(max_batch=4, codes=True)
    texts = _texts()
    got, res = {}, {}
    with pipe.open_session(_params(), use_decoder=False, rows=4, seed=SEED) as ses:
        step = ses.session.step

        def spy():
            out = step()
            res.update({r.ticket: r for r in out})
            return out
        ses.session.step = spy
        tk = [ses.submit(texts[u], utt_id=u, max_new_token=LIMS[u], stream=k, stream_batch=8) for u, k in ((1, "exact"), (4, "eager"))]
        for t, d, cn in ses.drain():
            got.setdefault(t, []).append(d)
    for t, u in zip(tk, (1, 4)):
        assert res[t].hiddens is None and res[t].ids.shape[0] == LIMS[u] and len(got[t]) >= 2
    wav = _concat(got[tk[0]])
    assert torch.equal(wav, pipe._decode_to_wavs([res[tk[0]].ids], False)[0]), "codes path: the exact chunks are not ctts_synth_batch_codes of the delivered ids"
    for c in got[tk[1]]:
        pre = pipe.synth_codes.decode_batch([res[tk[1]].ids[:c.n_tokens]])[0]
        assert torch.equal(c.wav, pre[c.start:c.start + int(c.wav.shape[0])])


def test_refine_then_stream_under_one_ticket(tmp_path_factory):
    from chatttsplus_amd.hip_models import GPT
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, RefineTextParams, SessionChunk
    _pipe(tmp_path_factory)
    g = GPT(LLAMA4, max_batch=4, max_seq_len=256, weight_dtype="fp32", options=dict(INV))
    sd = synth.gpt_state_dict(CFG4, 1234)
    # (tests/test_gpu_text_rows.py: the first 10 rows of the text head are raised so that the refined texts are not empty)
    sd["head_text.parametrizations.weight.original0"] = sd["head_text.parametrizations.weight.original0"].copy()
    sd["head_text.parametrizations.weight.original0"][:10] *= 30.0
    g.load_state_dict(sd)
    refine = RefineTextParams(prompt="[oral_2]", max_new_token=16, min_new_token=2, show_tqdm=False)
    texts = _texts()
    got, res = {}, {}
    try:
        pipe = ChatTTSPlusPipeline.from_components(g, _state["syn"], _state["tok"], torch.device("cuda:0"))
        with pipe.open_session(_params(), rows=4, seed=SEED, return_details=True, refine=refine) as ses:
            step = ses.session.step

            def spy():
                out = step()
                res.update({r.ticket: r for r in out if r.mode == "code"})
                return out
            ses.session.step = spy
            a = ses.submit(texts[0], utt_id=0, max_new_token=130, stream="exact", stream_batch=8)
            b = ses.submit(texts[1], utt_id=1, max_new_token=60)
            c = ses.submit(texts[2], utt_id=2, stream="exact")
            assert ses.cancel(c)                                          # in its refine stage: ends with an empty final chunk
            for t, d, cn in ses.drain():
                got.setdefault(t, []).append((d, cn))
        assert sorted(got) == [a, b, c] and len(res) == 2
        assert [(isinstance(d, SessionChunk), int(d.wav.shape[0]), d.final, cn) for d, cn in got[c]] == [(True, 0, True, True)]
        ch = [d for d, _ in got[a]]
        code = [r for r in res.values() if r.ids.shape[0] == 130]
        assert len(code) == 1 and len(ch) >= 3 and ch[-1].details.refined_text and ch[-1].details.ids.shape[0] == 130
        assert torch.equal(_concat(ch), pipe._decode_to_wavs([code[0].hiddens])[0])
        assert len(got[b]) == 1 and not isinstance(got[b][0][0], SessionChunk) and got[b][0][0].wav.shape[0] == 256 * 119
    finally:
        g.close()


def test_fp16_default_mode_exact_chunks_are_the_vocoding_of_its_own_hidden_rows(tmp_path_factory):
    pipe = _pipe(tmp_path_factory, "fp16", None)
    rec, trace = _run(pipe, KINDS, cancel=CANCELLED)
    assert max(b for _, b in trace) == 10
    for u in [u for u in range(12) if KINDS[u] == "exact"]:
        wav = _concat(rec[u]["chunks"])
        n = int(rec[u]["res"].ids.shape[0])
        assert (n == LIMS[u]) if u != CANCELLED else (0 < n < LIMS[u])
        assert torch.equal(wav, pipe._decode_to_wavs([rec[u]["res"].hiddens])[0]), f"utterance {u}"


# ---- DecodeSession.take_windows with out_slots == rows and a queue ---------------------------------------------------------------------------------------------
def test_window_views_are_written_rows_of_the_utterances_own_slot():
    """3 rows, 3 output slots, 7 utterances: four wait in the queue and take over slots that streaming utterances held.  The session's output buffers are filled
    with sentinels first: a window's views lie in the live utterance's own slot and hold written rows only, and after the run the buffers -- fills included --
    are those of the same run without any streaming ticket (streaming stores nothing there)."""
    from tests.test_gpu_session import LP, LW, T_MAX, _pool
    from chatttsplus_amd.hip_models.vocoder import settled_samples
    FILL_F, FILL_I = -123.0, -7
    g = engine("fp32", INV, max_batch=10, max_seq=256)
    syn = _state.get("syn") or _synth()
    lens, _, ids, mask, uids = _pool()
    lims = [140, 75, 120, 66, 131, 90, 124]
    emb = g(torch.from_numpy(ids[:7]), torch.ones(7, T_MAX, dtype=torch.bool))
    msk = torch.from_numpy(mask[:7])

    def drive(kinds):
        wavs, results = {}, {}
        with g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, min_new_token=MAX_NEW, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=SEED,
                            rows=3, out_slots=3) as ses:
            ses.hid.fill_(FILL_F)
            ses.ids.fill_(FILL_I)
            tk = [ses.submit(emb[u], msk[u], uids[u], limit=lims[u], stream=kinds[u], stream_batch=8 if kinds[u] == "exact" else None) for u in range(7)]
            while not ses.book.idle():
                results.update({r.ticket: r for r in ses.step()})
                wins = ses.take_windows()
                for w in wins:
                    k = w.ids.shape[0]
                    assert w.hiddens.shape[0] == k and (w.final or k > 0)
                    if not w.final:
                        s = ses.book.utts[w.ticket]["slot"]
                        assert w.hiddens.data_ptr() == ses.hid[s, w.tok0].data_ptr() and w.ids.data_ptr() == ses.ids[s, w.tok0].data_ptr()
                        assert w.tok0 + k <= w.n_tokens, "the view is not rows of the live utterance's slot"
                        assert bool((w.hiddens != FILL_F).all()) and bool((w.ids != FILL_I).all()), "the window reads a row that has not been written"
                        if w.mode == "exact":
                            assert w.s1 <= settled_samples(w.n_tokens, 256, syn.HALO_FRAMES)
                out = syn.synth_windows([w.hiddens for w in wins], [w.s0 - 2 * w.tok0 * 256 for w in wins], [w.s1 - w.s0 for w in wins])
                for w, o in zip(wins, out):
                    wavs.setdefault(w.ticket, []).append((w, o))
            torch.cuda.synchronize()
            return tk, results, wavs, ses.hid.clone(), ses.ids.clone()

    kinds = ["exact", "eager", "exact", None, "exact", "eager", "exact"]
    tk, results, wavs, hid, idb = drive(kinds)
    tk0, results0, wavs0, hid0, idb0 = drive([None] * 7)
    assert not wavs0 and torch.equal(hid, hid0) and torch.equal(idb, idb0), "the output slots differ from the run without streaming tickets"
    assert bool((hid == FILL_F).any()), "no fill left: the comparison saw no untouched row"
    assert sorted(results) == tk and tk[3] not in wavs
    for u in range(7):
        assert torch.equal(results[tk[u]].hiddens, results0[tk0[u]].hiddens)
    for u in (0, 1, 2, 4, 5, 6):
        r, ws = results[tk[u]], wavs[tk[u]]
        assert r.ids.shape[0] == lims[u] and [w.final for w, _ in ws] == [False] * (len(ws) - 1) + [True]
        pos = 0
        for w, o in ws:
            assert w.s0 == pos
            pos = w.s1
            if kinds[u] == "eager":
                assert torch.equal(o, syn.decode_batch([r.hiddens[:w.n_tokens]])[0][w.s0:w.s1])
        assert pos == 256 * (2 * lims[u] - 1)
        if kinds[u] == "exact":
            assert len(ws) >= 3 or lims[u] < 120
            assert torch.equal(torch.cat([o for _, o in ws]), syn.decode_batch([r.hiddens])[0]), f"utterance {u}"
    with g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, seed=SEED, rows=3, text_rows=dict(eos_token=21177, max_new_token=16)) as ses:
        with pytest.raises(_lib.HipBackendError, match="stream= is for code utterances"):
            ses.submit(emb[0], msk[0], 1, mode="text", stream="exact")
        with pytest.raises(_lib.HipBackendError, match="return_hidden=True"):
            ses.submit(emb[0], msk[0], 1, stream="exact")
        assert ses.submit(emb[0], msk[0], 1, stream="exact", stream_hidden=False) == 0
    with pytest.raises(_lib.HipBackendError, match="streaming windows.*per utterance at submit"):
        g.open_session(torch.tensor([0.3] * 4), EOS, MAX_NEW, stream=True)
    assert not g.busy
