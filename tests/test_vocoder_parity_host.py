"""CPU side of the vocoder parity checks (tests/test_gpu_vocoder_parity.py): the float64 oracle is right, its float32 default did not move, and every case of
tests/vocoder_cases.py stays inside the kernels' documented range ON THE REFERENCE ALONE -- finite, GEMM inputs at most 65504 / 4, and a float32 oracle
within 1e-5 of float64 in its worst frame -- so that a GPU failure of such a case is the kernels', not the case's."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chatttsplus_amd import synth
from oracle import ref_cpu
from oracle.ref_cpu import _t
from tests import vocoder_cases as V
from tests.helpers import per_frame_err
from tests.vocos_independent import vocos_decode_f64


def test_per_frame_err_definition():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((100, 7))
    ref[:, 3] = 0.0                                          # a silent frame
    got = ref.copy()
    got[:, 3] += 1e-3                                        # ... carrying an error
    got[10, 5] += 2e-3
    e = per_frame_err(got, ref, 100)
    g = math.sqrt(float(np.mean(ref ** 2)))
    assert e.shape == (7,) and np.allclose(e[3], 1e-3 / g) and np.allclose(e[5], 2e-3 / 10 / g) and not e[[0, 1, 2, 4, 6]].any()
    wav = rng.standard_normal(256 * 3)
    bad = wav.copy()
    bad[256:512] += 1e-4
    e = per_frame_err(bad.astype(np.float32), wav.astype(np.float32), 256)          # float32 in, float64 arithmetic
    assert e.shape == (3,) and e[0] == 0 and e[2] == 0 and abs(e[1] - 1e-4 / math.sqrt(float(np.mean(wav.astype(np.float32).astype(np.float64) ** 2)))) < 1e-8
    got[0, 0] = np.nan
    assert np.isnan(np.max(per_frame_err(got, ref, 100)))    # a NaN never passes an `<=`


@pytest.mark.parametrize("frames", [9, 65])
def test_float64_oracle_agrees_with_the_independent_restatement(frames):
    sd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    mel = np.random.Generator(np.random.Philox(key=200 + frames)).standard_normal((100, frames)).astype(np.float32)
    a = ref_cpu.vocos_decode(sd, torch.from_numpy(mel), dtype=torch.float64)
    assert a.dtype == torch.float64
    b = vocos_decode_f64(sd, mel)
    worst = float(np.max(per_frame_err(a.numpy(), b, 256)))
    assert worst <= 1e-9, worst


# ---- the float32 default is what it was: frozen copies of the function bodies as they stood before the `dtype` keyword -------------------------------------

def _frozen_convnext(sd, p, x, dilation, kernel=7):
    C = x.shape[1]
    y = F.conv1d(x, sd[p + "dwconv.weight"], sd[p + "dwconv.bias"], padding=dilation * (kernel // 2),
                 dilation=dilation, groups=C)
    y = y.transpose(1, 2)
    y = F.layer_norm(y, (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], eps=1e-6)
    y = F.linear(y, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])
    y = F.gelu(y)
    y = F.linear(y, sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"])
    y = y * sd[p + "gamma"]
    return y.transpose(1, 2) + x


@torch.no_grad()
def _frozen_dvae_decode(sd, hidden):
    sd = {k: _t(v).float() for k, v in sd.items()}
    inp = _t(hidden).float().permute(1, 0)[None]
    x = inp.view(inp.size(0), 2, inp.size(1) // 2, inp.size(2)).permute(0, 2, 3, 1).flatten(2)
    y = F.conv1d(x, sd["decoder.conv_in.0.weight"], sd["decoder.conv_in.0.bias"], padding=1)
    y = F.gelu(y)
    y = F.conv1d(y, sd["decoder.conv_in.2.weight"], sd["decoder.conv_in.2.bias"], padding=1)
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.decoder_block."))
    for i in range(n_layer):
        y = _frozen_convnext(sd, f"decoder.decoder_block.{i}.", y, dilation=2)
    y = F.conv1d(y, sd["decoder.conv_out.weight"])
    y = F.conv1d(y, sd["out_conv.weight"], padding=1)
    return (y * sd["coef"])[0]


def _frozen_gfsq_latent_from_indices(ids, levels=(5, 5, 5, 5), G=2, R=2):
    lv = torch.tensor(levels, dtype=torch.int64)
    hw = torch.tensor([l // 2 for l in levels], dtype=torch.float32)
    basis = torch.cumprod(torch.tensor([1] + list(levels[:-1]), dtype=torch.int64), 0)
    ids = _t(ids).to(torch.int64)
    lat = []
    for g in range(G):
        acc = 0
        for r in range(R):
            level = (ids[g * R + r][:, None] // basis[None, :]) % lv[None, :]
            acc = acc + ((level.float() - hw) / hw) * (lv.float() - 1) ** (-r)
        lat.append(acc)
    return torch.stack(lat, 0)


@torch.no_grad()
def _frozen_dvae_decode_codes(sd, ids, levels=(5, 5, 5, 5), G=2, R=2):
    ids = _t(ids).to(torch.int64)
    lat = _frozen_gfsq_latent_from_indices(ids.t().contiguous(), levels, G, R)
    feats = [F.linear(lat[g], _t(sd[f"vq_layer.quantizer.rvqs.{g}.project_out.weight"]).float(),
                      _t(sd[f"vq_layer.quantizer.rvqs.{g}.project_out.bias"]).float()) for g in range(G)]
    feat = torch.cat(feats, dim=-1)
    dec = {k: v for k, v in sd.items() if k.startswith("decoder.") or k in ("out_conv.weight", "coef")}
    return _frozen_dvae_decode(dec, feat)


@torch.no_grad()
def _frozen_vocos_backbone(sd, mel):
    x = F.conv1d(mel[None], sd["backbone.embed.weight"], sd["backbone.embed.bias"], padding=3)
    C = x.shape[1]
    x = F.layer_norm(x.transpose(1, 2), (C,), sd["backbone.norm.weight"], sd["backbone.norm.bias"], eps=1e-6).transpose(1, 2)
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.convnext."))
    for i in range(n_layer):
        x = _frozen_convnext(sd, f"backbone.convnext.{i}.", x, dilation=1)
    x = F.layer_norm(x.transpose(1, 2), (C,), sd["backbone.final_layer_norm.weight"], sd["backbone.final_layer_norm.bias"], eps=1e-6)
    return x[0]


@torch.no_grad()
def _frozen_vocos_head_spec(sd, feats):
    x = F.linear(feats, sd["head.out.weight"], sd["head.out.bias"]).transpose(0, 1)
    mag, p = x.chunk(2, dim=0)
    mag = torch.clip(torch.exp(mag), max=1e2)
    return mag * torch.cos(p), mag * torch.sin(p)


@torch.no_grad()
def _frozen_vocos_decode(sd, mel, n_fft=1024, hop=256):
    sd = {k: _t(v).float() for k, v in sd.items()}
    re, im = _frozen_vocos_head_spec(sd, _frozen_vocos_backbone(sd, _t(mel).float()))
    S = torch.complex(re, im)[None]
    return torch.istft(S, n_fft, hop, n_fft, sd["head.istft.window"], center=True)[0]


def _same(a, b):
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b)


def test_float32_default_is_bit_identical_to_the_frozen_bodies():
    rng = np.random.Generator(np.random.Philox(key=91))
    dsd = synth.dvae_state_dict(synth.DVAE_REAL, 1234)
    hid = torch.from_numpy(rng.standard_normal((11, 768)).astype(np.float32))
    _same(ref_cpu.dvae_decode(dsd, hid), _frozen_dvae_decode(dsd, hid))
    fsd = synth.dvae_full_decoder_state_dict(synth.DVAE_FULL_DEC, 1234)
    ids = torch.from_numpy(rng.integers(0, 625, size=(11, 4), dtype=np.int64))
    _same(ref_cpu.dvae_decode_codes(fsd, ids), _frozen_dvae_decode_codes(fsd, ids))
    _same(ref_cpu.gfsq_latent_from_indices(ids.t().contiguous()), _frozen_gfsq_latent_from_indices(ids.t().contiguous()))
    vsd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    vt = {k: _t(v).float() for k, v in vsd.items()}
    mel = torch.from_numpy(rng.standard_normal((100, 21)).astype(np.float32))
    _same(ref_cpu.vocos_decode(vsd, mel), _frozen_vocos_decode(vsd, mel))
    feats = _frozen_vocos_backbone(vt, mel)
    _same(ref_cpu.vocos_backbone(vt, mel), feats)
    for a, b in zip(ref_cpu.vocos_head_spec(vt, feats), _frozen_vocos_head_spec(vt, feats)):
        _same(a, b)
    x = mel[None, :, :].repeat(1, 6, 1)[:, :512].contiguous()                                   # [1, 512, 21]
    for p, d in (("backbone.convnext.3.", 1), ("backbone.convnext.0.", 2)):
        _same(ref_cpu._convnext(vt, p, x, dilation=d), _frozen_convnext(vt, p, x, dilation=d))


def test_float64_runs_in_float64_throughout():
    """The DVAE side has no second restatement: its float64 result is a float64 tensor (torch refuses mixed-dtype convolutions, so no float32 weight took
    part) and differs from the float32 one by float32 rounding, not by nothing."""
    c = V.BY_ID["codes-n9"]
    assert 1e-8 < V.reference(c.id)["yard"] < 1e-5
    assert ref_cpu.dvae_decode_codes(V.dvae_sd("plain", True), torch.from_numpy(V.case_input(c)), dtype=torch.float64).dtype == torch.float64
    d = V.BY_ID["dvae-n7"]
    assert 1e-8 < V.reference(d.id)["yard"] < 1e-5
    assert ref_cpu.dvae_decode(V.dvae_sd("plain"), torch.from_numpy(V.case_input(d)), dtype=torch.float64).dtype == torch.float64


# ---- the cases stay inside the documented range on the reference alone -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.id)
def test_case_is_inside_the_documented_range(c):
    r = V.reference(c.id)
    assert r["finite"], "the float64 reference is not finite"
    assert r["max_act"] <= V.ACT_LIMIT, f"|activation| {r['max_act']} entering a GEMM exceeds 65504 / 4"
    assert r["yard"] <= 1e-5, f"float32 oracle worst frame {r['yard']} against float64"
    assert r["yard"] > 0


def test_case_table_covers_what_it_must():
    ids = set(V.BY_ID)
    assert {f"dvae-n{n}" for n in (1, 7, 8, 9, 31, 32, 33, 64, 65)} <= ids
    assert {f"vocos-F{f}" for f in (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129)} <= ids
    assert {f"codes-n{n}" for n in (8, 9, 33)} <= ids
    assert [c.size for c in V.CASES if c.kind == "chain"] == [33, 8, 65, 1, 32, 9, 64, 7]
    assert max(c.size * (1 if c.kind == "vocos" else 2) for c in V.CASES) <= 130
    seen = V._Seen()
    V._oracle(V.BY_ID["vocos-head-x8"], V.case_input(V.BY_ID["vocos-head-x8"]), torch.float64, seen)
    assert 99.0 < seen.max_act <= 100.0                                                      # the spectrum is among the recorded GEMM inputs: clip(exp, 1e2) is reached
    big = V._Seen()
    V._oracle(V.BY_ID["dvae-hidden-x300"], V.case_input(V.BY_ID["dvae-hidden-x300"]), torch.float64, big)
    assert big.max_act >= float(np.abs(V.case_input(V.BY_ID["dvae-hidden-x300"])).max())     # ... and so are the input rows
