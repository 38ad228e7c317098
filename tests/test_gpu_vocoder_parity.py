"""The synthesis kernels (vocoder.hip, conv_gemm.h, cnx_gemm.h: DVAE decoder, Vocos, ISTFT as a GEMM) against the oracle in FLOAT64, frame by frame.

Every case of tests/vocoder_cases.py asserts   max_f per_frame_err(kernel, ref64) <= 8 * max_f per_frame_err(oracle_f32, ref64):
the yardstick on the right is computed here, on the CPU, from the reference alone (see vocoder_cases for why 8).  tests/test_gpu_vocoder.py keeps its 1e-3
global-rms checks; this file is ~200 times tighter and looks at every frame, at the tile edges (16-frame fragment groups, 64-row tiles, the 4-frame dwconv
blocks, 128 / 130 frames), on the 256-wide DVAE_full decoder, through decode_batch against the float64 chain, and on stress checkpoints and input scales.
Then the documented range: the +-255 weight limit, the clamp of infinite inputs, and NaN, which must come out as NaN.  tools/vocoder_parity.py records the
same measurements (profiles/vocoder_parity.jsonl)."""
import numpy as np
import pytest
import torch

from tests import vocoder_cases as V

pytestmark = pytest.mark.gpu

_PLAIN = [c for c in V.CASES if c.variant == "plain" and c.kind in ("dvae", "vocos")]
_CODES = [c for c in V.CASES if c.kind == "codes"]
_BATCH = [c for c in V.CASES if c.kind == "chain"]
_STRESS = sorted((c for c in V.CASES if c.variant != "plain"), key=lambda c: c.variant)        # cases of one checkpoint run back to back on one handle


@pytest.fixture(scope="module")
def plain():
    s = V.open_synth("plain", max_frames=512, max_batch=8)
    yield s
    V.close_synth(s)


@pytest.fixture(scope="module")
def full():
    s = V.open_synth("plain", full=True, max_frames=512, max_batch=4)
    yield s
    V.close_synth(s)


@pytest.fixture(scope="module")
def stress():
    """One small handle per stress checkpoint, alive while consecutive cases use it."""
    held = {}

    def get(variant):
        if variant not in held:
            for s in held.values():
                V.close_synth(s)
            held.clear()
            held[variant] = V.open_synth(variant)
        return held[variant]
    yield get
    for s in held.values():
        V.close_synth(s)


def _check(c, got):
    m = V.measure(c, got)
    print(V.fmt(m))
    assert got.shape == V.reference(c.id)["ref64"].shape
    assert m["kernel_worst_frame"] <= V.FACTOR * m["f32_oracle_worst_frame"], V.fmt(m)


@pytest.mark.parametrize("c", _PLAIN, ids=lambda c: c.id)
def test_edges_and_input_scales(plain, c):
    """dvae_decode at 2n frames, vocos_decode at F frames around every tile edge; hidden x {1e-3, 30, 300}, mel x {0.01, 4}."""
    _check(c, V.run_kernel(c, plain))


@pytest.mark.parametrize("c", _CODES, ids=lambda c: c.id)
def test_decode_codes_on_the_256_wide_decoder(full, c):
    """dvae_decode_codes on DVAE_full's decoder: the CPL = 4 depthwise-conv path."""
    _check(c, V.run_kernel(c, full))


def test_decode_batch_against_the_float64_chain(plain):
    """Eight ragged utterances in one decode_batch call, each compared per hop segment with vocos_decode(dvae_decode(.)) in float64."""
    outs = V.run_batch(_BATCH, plain)
    for c, got in zip(_BATCH, outs):
        _check(c, got)


@pytest.mark.parametrize("c", _STRESS, ids=lambda c: c.id)
def test_stress_checkpoints(stress, c):
    """gamma x 0 (only the gemm_split_kernel stages remain), gamma x 3.3, norm.weight outliers at hidden x 30, head.out.weight x 8 (the clip(exp, 1e2) and
    phases of tens of radians: the device cosf / sinf range reduction), and a checkpoint holding the largest weight that loads (255.875)."""
    _check(c, V.run_kernel(c, stress(c.variant)))


def test_weight_outside_the_split_range_is_refused_at_load():
    with pytest.raises(Exception, match=r"outside the \+-255 range"):
        V.close_synth(V.open_synth("w256"))


def _hidden33():
    return V.case_input(V.BY_ID["dvae-n33"]).copy()


def test_infinite_input_is_clamped(plain):
    """+inf in hidden row 16 of 33: clamped to 65504 as documented; the call succeeds and the mel is finite."""
    hid = _hidden33()
    hid[16, :] = np.inf
    mel = plain.dvae_decode(torch.from_numpy(hid).cuda()).cpu().numpy()
    assert mel.shape == (100, 66) and np.isfinite(mel).all()


def test_nan_input_comes_out_as_nan(plain):
    """A NaN hidden row (an overflowed fp16 GPT) must not turn into plausible audio: mel frames 32 and 33 (= row 16) are NaN throughout and the chained
    waveform contains NaN; no error is raised.  The next call on the same handle is clean again."""
    clean = _hidden33()
    before = plain.dvae_decode(torch.from_numpy(clean).cuda()).cpu().numpy()
    hid = clean.copy()
    hid[16, 5] = np.nan
    mel = plain.dvae_decode(torch.from_numpy(hid).cuda()).cpu().numpy()
    assert np.isnan(mel[:, 32:34]).all(), f"{int(np.isnan(mel[:, 32:34]).sum())} of 200 values of frames 32, 33 are NaN"
    wav = plain.decode_batch([torch.from_numpy(hid).cuda()])[0].cpu().numpy()
    assert wav.shape == (256 * 65,) and np.isnan(wav).any()
    after = plain.dvae_decode(torch.from_numpy(clean).cuda()).cpu().numpy()
    assert np.array_equal(before, after), "a NaN utterance left something behind in the handle's workspaces"
