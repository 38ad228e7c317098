"""Output sample rate per utterance in a serving session and in infer() (SynthSession.submit(sample_rate=), ChatTTSPlusPipeline.resampler).  The engine,
synth, toy tokenizer, texts and token limits are tests/test_gpu_stream_session.py's: a batch_invariant fp32 engine, limits of 60 - 140 tokens that are the
lengths (min_new_token = max_new_token).

One session of ten rows serves "exact" tickets at 16 kHz, 22.05 kHz and 8 kHz (one of them int16 PCM), a plain "exact" ticket, and non-streaming tickets at
48 kHz and 24 kHz.  Checked: a resampled ticket's chunks are consecutive in OUTPUT samples and concatenate, bit for bit, to Resampler.resample of the 24 kHz
waveform the same text gets without any rate; the tickets at 24 kHz are what they are when no rate is named anywhere; a cancel ends a resampled ticket with
the resampling of the tokens written; the refusals leave the session usable."""
import pytest
import torch

from chatttsplus_amd import _lib
from tests.test_gpu_stream_session import LIMS, SEED, _params, _pipe, _texts

pytestmark = pytest.mark.gpu

# utterance -> (text, stream, sample_rate, pcm16, stream_batch); utterances 4 and 5 are one text under one noise key: the same audio as int16 and as float32
SPEC = [(0, "exact", 16000, False, 8), (1, "exact", 16000, False, 8), (2, None, 48000, False, None), (3, "exact", 22050, False, None),
        (4, "exact", 8000, True, 8), (4, "exact", 8000, False, 8), (6, "exact", None, False, 8), (7, None, None, False, None),
        (8, "exact", 22050, False, 8), (9, None, 48000, False, None), (10, "exact", 16000, False, None), (11, None, None, False, None)]
CANCELLED = 0                                       # (16 kHz, limit 140) cancelled once its first chunk has arrived


def _run(pipe, spec, cancel=None, **open_kw):
    """tests/test_gpu_stream_session.py's arrival schedule: 4 texts, three polls, then the other 8 (the batch grows 4 -> 10 rows, two wait in the queue)"""
    from chatttsplus_amd.pipeline import SessionChunk
    texts = _texts()
    rec = {u: dict(chunks=[], out=None, res=None, cancelled=False) for u in range(len(spec))}
    with pipe.open_session(_params(), rows=10, seed=SEED, **open_kw) as ses:
        step, by_tk, tk_of = ses.session.step, {}, {}

        def spy():
            out = step()
            for r in out:
                rec[by_tk[r.ticket]]["res"] = r
            return out
        ses.session.step = spy

        def sub(u):
            t, stream, rate, pcm, sb = spec[u]
            kw = {} if rate is None else dict(sample_rate=rate)
            tk = ses.submit(texts[t], utt_id=t, max_new_token=LIMS[t], stream=stream, stream_batch=sb, pcm16=pcm, **kw)
            by_tk[tk], tk_of[u] = u, tk

        def take(out):
            for t, d, c in out:
                r = rec[by_tk[t]]
                if isinstance(d, SessionChunk):
                    assert not r["chunks"] or not r["chunks"][-1].final, "a chunk behind the final one"
                    r["chunks"].append(d)
                else:
                    assert r["out"] is None
                    r["out"] = d
                r["cancelled"] = c
        for u in range(4):
            sub(u)
        for _ in range(3):
            take(ses.poll())
        for u in range(4, len(spec)):
            sub(u)
        asked = False
        while not ses.session.book.idle():
            take(ses.poll())
            if cancel is not None and not asked and rec[cancel]["chunks"]:
                assert ses.cancel(tk_of[cancel])
                asked = True
        assert not ses._rates and not ses._emitted and not ses._streams and not ses.session.book._lookback
    torch.cuda.synchronize()
    return rec


def _concat(chunks, rate):
    pos = 0
    for c in chunks:
        assert c.start == pos, f"chunk starts at output sample {c.start}, the previous one ended at {pos}"
        assert c.sample_rate == rate
        pos += int(c.wav.shape[0])
    assert chunks[-1].final and not any(c.final for c in chunks[:-1])
    assert all(int(c.wav.shape[0]) > 0 for c in chunks[:-1]), "an empty chunk that is not the final one"
    return torch.cat([c.wav for c in chunks])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    pipe = _pipe(tmp_path_factory)
    rated = _run(pipe, SPEC, cancel=CANCELLED)
    plain = _run(pipe, [(t, None, None, False, None) for t, *_ in SPEC])                    # every text's offline 24 kHz waveform
    unrated = _run(pipe, [(t, s, None, p, b) for t, s, _, p, b in SPEC], cancel=CANCELLED)  # the same schedule, no rate named anywhere
    return pipe, rated, plain, unrated


def test_resampled_exact_chunks_concatenate_to_the_resampled_offline_waveform(runs):
    from chatttsplus_amd.hip_models.vocoder import settled_samples
    pipe, rated, plain, _ = runs
    for u, (t, stream, rate, pcm, sb) in enumerate(SPEC):
        if stream != "exact" or rate is None or u == CANCELLED:
            continue
        rs, ch = pipe.resampler(rate), rated[u]["chunks"]
        wav24 = plain[u]["out"]
        assert wav24.shape == (256 * (2 * LIMS[t] - 1),) and int(rated[u]["res"].ids.shape[0]) == LIMS[t]
        got = _concat(ch, rate)
        print(f"utterance {u} at {rate} Hz (limit {LIMS[t]}, int16 {pcm}): chunks of {[int(c.wav.shape[0]) for c in ch]} output samples")
        assert got.shape[0] == rs.out_total(wav24.shape[0])
        want = rs.resample([wav24], pcm16=pcm)[0]
        assert got.dtype == want.dtype == (torch.int16 if pcm else torch.float32)
        assert torch.equal(got, want), f"utterance {u} at {rate} Hz: the chunks are not the resampling of its offline waveform"
        if LIMS[t] >= 120:
            assert len(ch) >= 3, f"utterance {u}: {len(ch) - 1} chunks before the final one"
        for c in ch[:-1]:
            assert c.start + int(c.wav.shape[0]) <= rs.out_settled(settled_samples(c.n_tokens, 256, pipe.synth.HALO_FRAMES))
    # the int16 ticket is the conversion of the float ticket of the same utterance
    f, p = _concat(rated[5]["chunks"], 8000), _concat(rated[4]["chunks"], 8000)
    assert p.dtype == torch.int16 and f.dtype == torch.float32
    assert torch.equal(p, torch.round(torch.clamp(f, -1, 1) * 32767).to(torch.int16))


def test_non_streaming_tickets_at_a_rate_are_the_resampling_of_their_waveform(runs):
    pipe, rated, plain, _ = runs
    for u in (2, 9):
        rs = pipe.resampler(48000)
        got, wav24 = rated[u]["out"], plain[u]["out"]
        assert not rated[u]["chunks"] and got.shape[0] == rs.out_total(wav24.shape[0]) == 2 * wav24.shape[0]
        assert torch.equal(got, rs.resample([wav24])[0])


def test_tickets_at_24k_are_what_they_are_with_no_rate_named(runs):
    pipe, rated, plain, unrated = runs
    for u in (7, 11):
        assert torch.equal(rated[u]["out"], unrated[u]["out"]) and torch.equal(rated[u]["out"], plain[u]["out"])
    a, b = rated[6]["chunks"], unrated[6]["chunks"]
    assert len(a) >= 2 and len(b) >= 2
    assert torch.equal(_concat(a, 24000), _concat(b, 24000)) and torch.equal(_concat(a, 24000), plain[6]["out"])
    # ... and a rate changes no token: every utterance's ids and hidden rows are the unrated run's
    for u in range(len(SPEC)):
        if u != CANCELLED:
            assert torch.equal(rated[u]["res"].ids, unrated[u]["res"].ids) and torch.equal(rated[u]["res"].hiddens, unrated[u]["res"].hiddens)


def test_a_cancel_ends_a_resampled_ticket_with_the_audio_of_the_tokens_written(runs):
    pipe, rated, _, _ = runs
    r = rated[CANCELLED]
    res, ch = r["res"], r["chunks"]
    n = int(res.ids.shape[0])
    assert res.cancelled and r["cancelled"] and len(ch) >= 2 and 0 < n < LIMS[SPEC[CANCELLED][0]]
    rs = pipe.resampler(16000)
    want = rs.resample([pipe._decode_to_wavs([res.hiddens])[0]])[0]
    got = _concat(ch, 16000)
    assert got.shape[0] == rs.out_total(256 * (2 * n - 1)) and torch.equal(got, want)


def test_refusals_leave_the_session_usable(tmp_path_factory):
    from chatttsplus_amd.pipeline import SessionChunk
    pipe = _pipe(tmp_path_factory)
    texts = _texts()
    with pipe.open_session(_params(), rows=4, seed=SEED, sample_rate=16000) as ses:
        with pytest.raises(_lib.HipBackendError, match="stream=\"eager\" with sample_rate=16000"):
            ses.submit(texts[2], utt_id=2, max_new_token=60, stream="eager")              # the session's default rate
        with pytest.raises(_lib.HipBackendError, match="stream=\"eager\" with sample_rate=8000"):
            ses.submit(texts[2], utt_id=2, max_new_token=60, stream="eager", sample_rate=8000)
        with pytest.raises(_lib.HipBackendError, match="sample_rate=7: .*65560 taps"):
            ses.submit(texts[2], utt_id=2, max_new_token=60, sample_rate=7)
        with pytest.raises(_lib.HipBackendError, match="positive integer"):
            ses.submit(texts[2], utt_id=2, max_new_token=60, sample_rate=-8000)
        assert ses.session.book.idle()
        a = ses.submit(texts[2], utt_id=2, max_new_token=LIMS[2])                          # the session's default: 16 kHz
        b = ses.submit(texts[2], utt_id=2, max_new_token=LIMS[2], sample_rate=24000)       # a submit overrides it
        c = ses.submit(texts[2], utt_id=2, max_new_token=LIMS[2], stream="eager", sample_rate=24000)
        got = {}
        for t, d, cn in ses.drain():
            got.setdefault(t, []).append(d)
    assert len(got[a]) == len(got[b]) == 1 and all(isinstance(d, SessionChunk) and d.sample_rate == 24000 for d in got[c])
    assert got[b][0].shape == (256 * (2 * LIMS[2] - 1),) and torch.equal(got[a][0], pipe.resampler(16000).resample([got[b][0]])[0])
    with pytest.raises(_lib.HipBackendError, match="sample_rate=7"):
        pipe.open_session(_params(), rows=4, sample_rate=7)
    with pytest.raises(_lib.HipBackendError, match=r"infer\(stream=True, sample_rate=16000\)"):
        list(pipe.infer([texts[0]], stream=True, skip_refine_text=True, params_infer_code=_params(), sample_rate=16000))
    with pytest.raises(_lib.HipBackendError, match=r"infer_sharded\(sample_rate=16000\)"):
        pipe.infer_sharded([texts[0]], params_infer_code=_params(), sample_rate=16000)
    assert pipe.resampler(16000) is pipe.resampler(16000)


def test_infer_continuous_at_a_rate_is_the_resampling_of_its_waveforms(tmp_path_factory):
    pipe = _pipe(tmp_path_factory)
    texts, lims = _texts()[:6], [60, 75, 64, 70, 88, 61]
    kw = dict(skip_refine_text=True, params_infer_code=_params(), continuous=True, slice_size=4, noise_seed=SEED, utt_ids=list(range(6)),
              max_new_tokens_per_utterance=lims)
    w24 = [w for ws in pipe.infer(texts, **kw) for w in ws]
    w16 = [w for ws in pipe.infer(texts, sample_rate=16000, **kw) for w in ws]
    same = [w for ws in pipe.infer(texts, sample_rate=24000, **kw) for w in ws]
    rs = pipe.resampler(16000)
    assert len(w24) == len(w16) == len(same) == 6
    for u in range(6):
        assert w24[u].shape == (256 * (2 * lims[u] - 1),) and torch.equal(same[u], w24[u])
        assert w16[u].shape[0] == rs.out_total(w24[u].shape[0]) and torch.equal(w16[u], rs.resample([w24[u]])[0]), f"utterance {u}"
    # the details path: winners only, resampled
    dkw = dict(skip_refine_text=True, params_infer_code=_params(), noise="device", noise_seed=SEED, utt_ids=[0, 1], max_new_tokens_per_utterance=lims[:2],
               return_details=True)
    d24, d16 = list(pipe.infer(texts[:2], **dkw)), list(pipe.infer(texts[:2], sample_rate=16000, **dkw))
    assert len(d16) == len(d24) == 1 and [int(w.shape[0]) for w in d16[0].wavs] == [rs.out_total(256 * (2 * n - 1)) for n in lims[:2]]
    for u in range(2):
        assert torch.equal(d16[0].ids[u], d24[0].ids[u]) and torch.equal(d16[0].wavs[u], rs.resample([d24[0].wavs[u]])[0])
