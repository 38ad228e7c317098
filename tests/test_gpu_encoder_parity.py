"""The clip encoder (csrc/encoder.hip, gemm_f32_kernel of conv_gemm.h: waveform -> STFT as a GEMM -> log-mel -> conv stack -> GFSQ codes) against the oracle in
FLOAT64, frame by frame.

Every case of tests/encoder_cases.py asserts, for the log-mel hook, the linear mel and the features,
    max_f per_frame_err(kernel, ref64) <= 8 * max(max_f per_frame_err(oracle_f32 "dft" form, ref64), 2^-23)
-- the yardstick on the right is computed here, on the CPU, from the reference alone -- and for the codes a teacher-forced digit check on the kernel's own
features: every digit within 0.5 + eps[r] of its float64 pre-round value, every id in [0, 625) (see encoder_cases).  tests/test_gpu_encoder.py keeps its one-length
2e-3 / 1e-3 checks and the 0.5 % code tests; this file looks at every frame and every digit at the frame edges: the smallest legal clip, odd and even frame counts,
T = 1 .. 7 under the dilated depthwise taps, both sides of the 64-row GEMM tile, lengths on and off a hop multiple, longest first on one handle so that every
short clip meets a dirty workspace; then input families (silence, int16-scale, DC, Nyquist, an impulse), stress checkpoints, other quantiser shapes, a clip of
exactly the handle's capacity, one shuffled batch bit-identical to the single-clip calls, and non-finite audio, which must come out as NaN mel frames and id -1,
never as plausible codes.  tools/encoder_parity.py records the same measurements (profiles/encoder_parity.jsonl)."""
import numpy as np
import pytest
import torch

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

_PLAIN = [c for c in E.CASES if c.variant == "plain" and c.id != "capacity-n24000"]             # the edge lengths, longest first, then the input families
_STRESS = [c for c in E.CASES if c.variant != "plain"]


@pytest.fixture(scope="module")
def enc():
    e = E.open_encoder()
    yield e
    E.close_encoder(e)


def _check(c, got, quant="g2r2"):
    ids, hook, feat = got
    m = E.measure(c, ids, hook, feat, quant)
    print(E.fmt(m))
    G, R, _ = E.QUANTS[quant]
    assert ids.shape == (G * R, c.codes) and hook.shape == (100, c.frames) and feat.shape == (c.codes, 1024)
    assert np.isfinite(hook).all() and np.isfinite(feat).all()
    assert m["linear_ratio"] <= E.FACTOR, E.fmt(m)
    if not c.linear_only:
        assert m["logmel_ratio"] <= E.FACTOR, E.fmt(m)
        assert m["feat_ratio"] <= E.FACTOR, E.fmt(m)
    assert m["ids_in_range"], "an id outside [0, 625)"
    assert m["digits"] == ids.size * 4 and m["digit_max_excess"] <= 0, f"{E.fmt(m)}; worst digit {m['digit_worst']}"


@pytest.mark.parametrize("c", _PLAIN, ids=lambda c: c.id)
def test_edges_and_input_families(enc, c):
    """One handle, longest clip first; then x 1e-3, silence, x 32768, a zeroed middle third, one impulse, DC (basis row 0) and Nyquist (basis row 512)."""
    _check(c, E.run_kernel(E.case_input(c), enc))


@pytest.mark.parametrize("c", _STRESS, ids=lambda c: c.id)
def test_stress_checkpoints(c):
    """gamma x 0 (only the conv GEMMs remain), gamma x 3.3, norm.weight outliers, coef x 0.05 and x 20 (the mel image x 20 and x 0.05 into the k3 conv)."""
    e = E.open_encoder(c.variant)
    try:
        _check(c, E.run_kernel(E.case_input(c), e))
    finally:
        E.close_encoder(e)


@pytest.mark.parametrize("quant", ["g2r2-nobound", "g4r4"])
def test_quantiser_shapes(quant):
    """gfsq_kernel without the initial bound, and with 4 groups of 256 channels x 4 residual levels (scale down to 4^-3), at every edge length."""
    e = E.open_encoder("plain", quant)
    try:
        for c in E.EDGES:
            _check(c, E.run_kernel(E.case_input(c), e), quant)
    finally:
        E.close_encoder(e)


def test_clip_of_exactly_the_capacity():
    """max_seconds = 1.0 and a clip of exactly 24000 samples: the last frames sit at the end of every workspace."""
    c = E.BY_ID["capacity-n24000"]
    e = E.open_encoder(max_seconds=1.0)
    try:
        assert e.cfg.max_samples == c.n
        _check(c, E.run_kernel(E.case_input(c), e))
    finally:
        E.close_encoder(e)


def test_shuffled_batch_is_bit_identical_to_the_single_clip_calls(enc):
    """One encode_batch call over the edge lengths in shuffled order (the early-return tiles of short clips beside long ones): ids, mel and features of every clip
    equal the single-clip call's bit for bit -- and those are the results the cases above hold against float64."""
    wavs = [torch.from_numpy(E.speech(n)) for n in E.BATCH_ORDER]
    single = [tuple(t.clone() for t in enc.encode(w, return_debug=True)) for w in wavs]
    got = enc.encode_batch(wavs, return_debug=True)
    assert len(got) == len(single)
    for n, g, s in zip(E.BATCH_ORDER, got, single):
        for name, a, b in zip(("ids", "mel", "feat"), g, s):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{n} samples: {name} differs from the single-clip call"


# ---- non-finite audio ------------------------------------------------------------------------------------------------------------------------------------------------

def _bad_clip(value):
    wav = E.speech(E.NONFINITE_N).copy()
    wav[E.NONFINITE_AT] = value
    return wav


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_sample_gives_nan_mel_frames_and_negative_ids(enc, value):
    """A NaN (+inf) at sample 8000 of 16384: the mel frames whose window covers it (30 .. 33) are NaN throughout, every other mel frame is bit-equal to the clean
    run, every code frame whose float64 reference features are not finite has id -1 in all G R rows, and the remaining frames pass the digit check."""
    clean_ids, clean_hook, _ = E.run_kernel(E.speech(E.NONFINITE_N), enc)
    wav = _bad_clip(value)
    ids, hook, feat = E.run_kernel(wav, enc)
    frames = E.nonfinite_mel_frames(E.NONFINITE_N, E.NONFINITE_AT)
    assert np.isnan(hook[:, frames]).all(), f"{int(np.isnan(hook[:, frames]).sum())} of {100 * len(frames)} values of mel frames {frames} are NaN"
    assert np.array_equal(np.delete(hook, frames, axis=1), np.delete(clean_hook, frames, axis=1)), "a mel frame outside the sample's windows changed"
    _, feat64 = E.oracle(E.encoder_sd(), wav, torch.float64)
    bad = ~np.isfinite(feat64).all(axis=0)                                                        # [T]
    assert bad.any()
    assert (ids[:, bad] == -1).all(), f"code frames {np.flatnonzero((ids[:, bad] != -1).any(0))} of the non-finite ones carry ids {np.unique(ids[:, bad])}"
    if (~bad).any():
        assert np.isfinite(feat[~bad]).all()
        d = E.digit_check(feat[~bad], ids[:, ~bad], E.encoder_sd(), "g2r2", E.quant_reference("n16384")["eps"])
        assert d["in_range"] and d["digits"] == 16 * int((~bad).sum()) and d["max_excess"] <= 0, d
    again = E.run_kernel(E.speech(E.NONFINITE_N), enc)                                            # the same handle afterwards
    assert np.array_equal(again[0], clean_ids) and np.array_equal(again[1], clean_hook)


def test_non_finite_clip_in_a_batch_leaves_its_neighbours_alone(enc):
    a, b = torch.from_numpy(E.speech(16640)), torch.from_numpy(E.speech(8448))
    single = [tuple(t.clone() for t in enc.encode(w, return_debug=True)) for w in (a, b)]
    got = enc.encode_batch([a, torch.from_numpy(_bad_clip(np.nan)), b], return_debug=True)
    for g, s in ((got[0], single[0]), (got[2], single[1])):
        for name, x, y in zip(("ids", "mel", "feat"), g, s):
            assert torch.equal(x, y), f"{name} of a clean clip changed beside a NaN clip"
    assert bool((got[1][0] == -1).all())                                                          # all 32 code frames lie inside the conv stack's reach
    assert bool(torch.isnan(got[1][1][:, 30:34]).all())


def test_clean_call_after_non_finite_clips_is_unchanged(enc):
    """Hygiene: nothing of a NaN or inf clip stays in the handle's workspaces (single-clip and batch path)."""
    wav = torch.from_numpy(E.speech(4095))                                                        # shorter: it runs over rows the bad clips wrote
    before = tuple(t.clone() for t in enc.encode(wav, return_debug=True))
    enc.encode(torch.from_numpy(_bad_clip(np.nan)))
    enc.encode(torch.from_numpy(_bad_clip(np.inf)))
    enc.encode_batch([torch.from_numpy(_bad_clip(np.nan)), torch.from_numpy(_bad_clip(-np.inf))])
    after = enc.encode(wav, return_debug=True)
    after_batch = enc.encode_batch([wav], return_debug=True)[0]
    for name, x, y, z in zip(("ids", "mel", "feat"), before, after, after_batch):
        assert torch.equal(x, y) and torch.equal(x, z), f"{name} differs after non-finite clips used the handle"
    assert np.isfinite(before[2].cpu().numpy()).all()
