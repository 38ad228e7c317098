"""CPU side of the clip-encoder parity checks (tests/test_gpu_encoder_parity.py): the float64 oracle is right (its STFT agrees with an independent restatement, the
kernel's own DFT formulation), its float32 default did not move, and every case of tests/encoder_cases.py meets its conditions ON THE REFERENCE ALONE -- finite,
the float32 oracle within 1e-4 of float64 in its worst frame (all but the two declared linear-mel-only cases), at most 1 % of the float64 digits within eps of a
rounding boundary -- so that a GPU failure of such a case is the kernels', not the case's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chatttsplus_amd import synth
from oracle import ref_cpu
from oracle.ref_cpu import _t, fsq_bound, mel_filterbank
from tests import encoder_cases as E
from tests.helpers import per_frame_err
from tests.test_vocoder_parity_host import _frozen_convnext


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c.id)
def test_fft_and_dft_forms_agree_in_float64(c):
    """torch.stft against reflect-pad -> unfold -> matmul with the windowed [cos | -sin] basis: the independent restatement of the STFT.  Worst frame, on the
    log-mel and on the linear mel."""
    wav = torch.from_numpy(E.case_input(c))
    a = ref_cpu.mel_features(wav, dtype=torch.float64)
    b = ref_cpu.mel_features(wav, dtype=torch.float64, form="dft")
    assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape == (100, c.frames)
    worst = float(np.max(per_frame_err(b.numpy(), a.numpy(), 100)))
    worst_lin = float(np.max(per_frame_err(np.exp(b.numpy()), np.exp(a.numpy()), 100)))
    assert worst <= 1e-9 and worst_lin <= 1e-9, (worst, worst_lin)


def test_dft_basis_is_the_kernels():
    """Rows k < 513: w[n] cos(2 pi k n / 1024), rows 513 + k: -w[n] sin(...); angles from the exactly reduced (k n) % 1024 in float64, then cast."""
    w = torch.hann_window(1024, periodic=True)
    B = ref_cpu.dft_basis(1024, w, torch.float32)
    assert B.shape == (1026, 1024) and B.dtype == torch.float32
    for k, n in ((0, 5), (512, 3), (512, 4), (300, 1000), (1, 256)):
        ang = 2.0 * np.pi * ((k * n) % 1024) / 1024
        assert float(B[k, n]) == float(np.float32(float(w[n]) * np.cos(ang))) and float(B[513 + k, n]) == float(np.float32(-float(w[n]) * np.sin(ang)))
    assert not B[513].any() and float(B[512, 3]) == -float(w[3])                # sin row of DC is exactly zero; Nyquist alternates exactly


def test_float64_runs_in_float64_throughout():
    c = E.BY_ID["n2304"]
    sd = E.encoder_sd()
    wav = torch.from_numpy(E.case_input(c))
    mel = ref_cpu.mel_features(wav, dtype=torch.float64)
    feat = ref_cpu.dvae_encoder_features(sd, mel, dtype=torch.float64)
    ids, lat, pre = ref_cpu.gfsq_quantize(feat.t(), sd, dtype=torch.float64, return_pre=True)
    assert mel.dtype == feat.dtype == lat.dtype == pre.dtype == torch.float64 and ids.dtype == torch.int32
    assert feat.shape == (1024, c.codes) and pre.shape == (2, 2, c.codes, 4) and ids.shape == (4, c.codes)
    assert torch.equal(ids, ref_cpu.dvae_encode(sd, wav, dtype=torch.float64))
    r = E.reference(c.id)
    assert E.YARD_FLOOR < r["yard_logmel"] < 1e-5 and E.YARD_FLOOR < r["yard_feat"] < 1e-5          # float32 differs by float32 rounding, not by nothing
    # the pre-round values are what the digits are rounded from
    q = torch.round(pre)                                                                             # [G][R][T][4] in -2 .. 2
    assert torch.equal(((q + 2) * torch.tensor([1, 5, 25, 125], dtype=torch.float64)).sum(-1).to(torch.int32).view(4, -1), ids)


# ---- the float32 default is what it was: frozen copies of the function bodies as they stood before the `dtype` / `form` keywords -----------------------------

@torch.no_grad()
def _frozen_mel_features(wav, n_fft=1024, hop=256, n_mels=100, sample_rate=24000):
    wav = _t(wav).float()
    window = torch.hann_window(n_fft, periodic=True)
    spec = torch.stft(wav, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True).abs()
    mel = torch.matmul(spec.transpose(-1, -2), mel_filterbank(n_fft // 2 + 1, n_mels, sample_rate)).transpose(-1, -2)
    return torch.log(torch.clip(mel, min=1e-5))


def _frozen_gfsq_quantize(x, sd, levels=(5, 5, 5, 5), G=2, R=2, pre_bound=True):
    lv = torch.tensor(levels, dtype=torch.float32)
    hw = torch.tensor([l // 2 for l in levels], dtype=torch.float32)
    basis = torch.cumprod(torch.tensor([1] + list(levels[:-1]), dtype=torch.float32), 0)
    per = x.shape[-1] // G
    out, lat = [], []
    for g in range(G):
        w, b = _t(sd[f"vq_layer.quantizer.rvqs.{g}.project_in.weight"]).float(), _t(sd[f"vq_layer.quantizer.rvqs.{g}.project_in.bias"]).float()
        z = F.linear(x[..., g * per:(g + 1) * per], w, b)
        residual = fsq_bound(z, lv) if pre_bound else z
        acc = torch.zeros_like(z)
        for r in range(R):
            scale = (lv - 1) ** (-r)
            codes = torch.round(fsq_bound(residual / scale, lv)) / hw
            idx = ((codes * hw + hw) * basis).sum(-1).to(torch.int32)
            residual = residual - codes * scale
            acc = acc + codes * scale
            out.append(idx)
        lat.append(acc)
    return torch.stack(out, 0), torch.stack(lat, 0)


@torch.no_grad()
def _frozen_dvae_encoder_features(sd, mel):
    sd = {k: _t(v).float() for k, v in sd.items()}
    x = (_t(mel).float() / sd["coef"].view(-1, 1))[None]
    x = F.gelu(F.conv1d(x, sd["downsample_conv.0.weight"], sd["downsample_conv.0.bias"], stride=1, padding=1))
    x = F.gelu(F.conv1d(x, sd["downsample_conv.2.weight"], sd["downsample_conv.2.bias"], stride=2, padding=1))
    y = F.gelu(F.conv1d(x, sd["encoder.conv_in.0.weight"], sd["encoder.conv_in.0.bias"], padding=1))
    y = F.conv1d(y, sd["encoder.conv_in.2.weight"], sd["encoder.conv_in.2.bias"], padding=1)
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.decoder_block."))
    for i in range(n_layer):
        y = _frozen_convnext(sd, f"encoder.decoder_block.{i}.", y, dilation=2)
    return F.conv1d(y, sd["encoder.conv_out.weight"])[0]


@torch.no_grad()
def _frozen_dvae_encode(sd, wav, pre_bound=True):
    feat = _frozen_dvae_encoder_features(sd, _frozen_mel_features(wav))
    return _frozen_gfsq_quantize(feat.transpose(0, 1), {k: _t(v).float() for k, v in sd.items()}, pre_bound=pre_bound)[0]


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_float32_default_is_bit_identical_to_the_frozen_bodies():
    sd = synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234)
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    for n in (513, 3328, 16384):
        wav = torch.from_numpy(synth.speaker_wave(100 + n, n))
        mel = _frozen_mel_features(wav)
        _same(ref_cpu.mel_features(wav), mel)
        assert mel.dtype == torch.float32
        feat = _frozen_dvae_encoder_features(sd, mel)
        _same(ref_cpu.dvae_encoder_features(sd, mel), feat)
        for pb in (True, False):
            want = _frozen_gfsq_quantize(feat.t(), sdt, pre_bound=pb)
            got = ref_cpu.gfsq_quantize(feat.t(), sdt, pre_bound=pb)
            assert len(got) == 2
            _same(got[0], want[0]), _same(got[1], want[1])
            _same(ref_cpu.gfsq_indices(feat.t(), sdt, pre_bound=pb), want[0])
            _same(ref_cpu.dvae_encode(sd, wav, pre_bound=pb), _frozen_dvae_encode(sd, wav, pre_bound=pb))
            three = ref_cpu.gfsq_quantize(feat.t(), sdt, pre_bound=pb, return_pre=True)
            _same(three[0], want[0]), _same(three[1], want[1])
    sd4 = E.encoder_sd("plain", "g4r4")
    want = _frozen_gfsq_quantize(feat.t(), sd4, G=4, R=4)
    got = ref_cpu.gfsq_quantize(feat.t(), sd4, G=4, R=4)
    _same(got[0], want[0]), _same(got[1], want[1])


# ---- the cases meet their conditions on the reference alone ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c.id)
def test_case_meets_its_conditions(c):
    r = E.reference(c.id)
    assert r["finite"], "the float64 reference is not finite"
    assert r["hook64"].shape == (100, c.frames) and r["feat64"].shape == (1024, c.codes)
    print(f"{c.id}: yardsticks log-mel {r['yard_logmel']:.3e} linear mel {r['yard_linear']:.3e} features {r['yard_feat']:.3e}")
    assert E.YARD_FLOOR <= r["yard_linear"] <= E.YARD_LIMIT, r["yard_linear"]
    if not c.linear_only:
        assert E.YARD_FLOOR <= r["yard_logmel"] <= E.YARD_LIMIT, f"log-mel yardstick {r['yard_logmel']}: change the case, not the bound"
        assert E.YARD_FLOOR <= r["yard_feat"] <= E.YARD_LIMIT, f"feature yardstick {r['yard_feat']}: change the case, not the bound"
    quants = E.QUANTS if c in E.EDGES or c.id == "capacity-n24000" else ("g2r2",)
    for quant in quants:
        q = E.quant_reference(c.id, quant)
        print(f"{c.id} [{quant}]: |float32 - float64| pre-round per level {q['f32_f64_pre_diff']}, near ties {q['near_tie_share']:.5f}")
        assert len(q["eps"]) == E.QUANTS[quant][1] and all(0 < e < 0.02 for e in q["eps"]), q["eps"]
        assert q["near_tie_share"] <= E.TIE_SHARE_LIMIT, q["near_tie_share"]
        assert q["codes_equal"], "the float32 and float64 oracle codes differ: a digit sits on a tie"


def test_case_table_covers_what_it_must():
    assert [c.n for c in E.EDGES] == sorted((513, 767, 768, 1279, 1536, 2048, 2304, 3328, 4095, 8192, 8448, 16128, 16384, 16640, 32512, 33023, 33280), reverse=True)
    want = {513: (3, 1), 767: (3, 1), 768: (4, 2), 1279: (5, 2), 1536: (7, 3), 2048: (9, 4), 2304: (10, 5), 3328: (14, 7), 4095: (16, 8), 8192: (33, 16),
            8448: (34, 17), 16128: (64, 32), 16384: (65, 32), 16640: (66, 33), 32512: (128, 64), 33023: (129, 64), 33280: (131, 65)}
    assert {c.n: (c.frames, c.codes) for c in E.EDGES} == want
    assert [c.id for c in E.CASES if c.linear_only] == ["wave-dc", "wave-nyquist"]                  # no other case may be exempted
    assert {c.family for c in E.CASES} == {"speech", "x1e-3", "zeros", "x32768", "gap", "impulse", "dc", "nyquist"}
    assert {c.variant for c in E.CASES} == {"plain", "gamma0", "gamma3.3", "outliers", "coef0.05", "coef20"}
    assert all(c.n == 16640 for c in E.CASES if c.family != "speech" or c.variant != "plain")
    assert max(c.n for c in E.CASES) <= 1.4 * 24000
    x = E.case_input(E.BY_ID["wave-impulse"])
    assert x[16640 // 2 + 37] == 1.0 and np.count_nonzero(x) == 1
    assert np.array_equal(E.case_input(E.BY_ID["wave-nyquist"])[:4], np.float32([0.5, -0.5, 0.5, -0.5]))
    g = E.case_input(E.BY_ID["wave-gap"])
    assert not g[16640 // 3:2 * 16640 // 3].any() and g[:16640 // 3].any() and g[2 * 16640 // 3:].any()
    sd, plain = E.encoder_sd("outliers"), E.encoder_sd("plain")
    k = "encoder.decoder_block.3.norm.weight"
    assert np.array_equal(sd[k][::37], plain[k][::37] * np.float32(20.0)) and np.array_equal(sd[k][1:37], plain[k][1:37])
    assert np.array_equal(E.encoder_sd("coef20")["coef"], plain["coef"] * np.float32(20.0))
    assert len([k for k in E.encoder_sd("plain", "g4r4") if "project_in.weight" in k]) == 4
    assert E.encoder_sd("plain", "g4r4")["vq_layer.quantizer.rvqs.3.project_in.weight"].shape == (4, 256)


# ---- the digit check has teeth ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quant", list(E.QUANTS))
def test_digit_check_accepts_the_oracle_and_rejects_one_wrong_digit(quant):
    c = E.BY_ID["n8448"]
    G, R, pb = E.QUANTS[quant]
    sd = E.encoder_sd("plain", quant)
    feat = np.ascontiguousarray(E.reference(c.id)["feat64"].T.astype(np.float32))                  # [T][1024]
    eps = E.quant_reference(c.id, quant)["eps"]
    ids = ref_cpu.gfsq_indices(torch.from_numpy(feat), sd, G=G, R=R, pre_bound=pb).numpy()
    d = E.digit_check(feat, ids, sd, quant, eps)
    assert d["in_range"] and d["digits"] == ids.size * 4 and d["max_excess"] <= 0 and d["max_abs_dev"] <= 0.5 + max(eps)
    for row, t, j in ((0, 0, 0), (G * R - 1, c.codes - 1, 3), (R, 5, 2)):                          # first / last frame, last residual level, a middle group
        bad = ids.copy()
        digit = (bad[row, t] // 5 ** j) % 5
        bad[row, t] += (1 if digit < 4 else -1) * 5 ** j                                           # one digit off by one level
        w = E.digit_check(feat, bad, sd, quant, eps)
        # found in its frame and group, at its own level or (through the residual it leaves) a later one
        assert w["max_excess"] > 0 and (w["worst"]["g"], w["worst"]["t"]) == (row // R, t) and w["worst"]["r"] >= row % R, w
    out = ids.copy()
    out[1, 2] = 625
    assert not E.digit_check(feat, out, sd, quant, eps)["in_range"]
    out[1, 2] = -1
    assert not E.digit_check(feat, out, sd, quant, eps)["in_range"]


# ---- non-finite audio on the reference ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_reference_mel_of_a_non_finite_sample(value):
    """What the GPU test asks of the kernels is what the reference does: exactly the mel frames whose window covers the sample are non-finite (torch.clip keeps
    NaN), and -- twelve dilated blocks wide -- every one of this clip's 32 feature frames."""
    n, at = E.NONFINITE_N, E.NONFINITE_AT
    frames = E.nonfinite_mel_frames(n, at)
    assert frames == [30, 31, 32, 33]
    wav = E.speech(n).copy()
    wav[at] = value
    mel = ref_cpu.mel_features(torch.from_numpy(wav), dtype=torch.float64)
    bad = ~np.isfinite(mel.numpy())
    assert bad[:, frames].all() and not np.delete(bad, frames, axis=1).any()
    feat = ref_cpu.dvae_encoder_features(E.encoder_sd(), mel, dtype=torch.float64).numpy()
    assert (~np.isfinite(feat)).all(axis=0).all() and feat.shape == (1024, 32)
