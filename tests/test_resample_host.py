"""Output sample rate, host side (no GPU): audio.resample_kernels against the function body audio.resample had before the table was factored out, the three
index rules of hip_models.resampler.ResampleGeometry (out_total, out_settled, in_range) against audio.resample and by index arithmetic, their C twins, the chunk
rule of SynthSession driven through a float64 tap evaluator, and SessionBook's stream_lookback against scripted row reports."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, audio
from chatttsplus_amd.hip_models.gpt import SessionBook, SessionWindow
from chatttsplus_amd.hip_models.resampler import ResampleGeometry, Resampler, rate_geometry

PAIRS = [(24000, 8000), (24000, 16000), (24000, 22050), (24000, 44100), (24000, 48000), (44100, 24000)]
GEOMETRY = {(24000, 8000): (3, 1, 19, 41), (24000, 16000): (3, 2, 10, 23), (24000, 22050): (160, 147, 7, 174), (24000, 44100): (80, 147, 7, 94),
            (24000, 48000): (1, 2, 7, 15)}


def _resample_before(wav, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """audio.resample as it was before resample_kernels existed, kept verbatim: the pin of `unchanged`"""
    if orig_freq == new_freq:
        return wav
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base / orig
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * window * scale
    kernels = kernels.to(torch.float32)                                         # [new, 1, 2 width + orig]
    shape = wav.shape
    x = wav.reshape(-1, shape[-1]).float()
    x = torch.nn.functional.pad(x, (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernels, stride=orig)            # [b, new, frames]
    y = y.transpose(1, 2).reshape(x.shape[0], -1)
    target = math.ceil(new * shape[-1] / orig)
    return y[..., :target].reshape(shape[:-1] + (target,)), kernels


def _wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * 2 - 1


@pytest.mark.parametrize("pair", PAIRS)
def test_resample_kernels_is_the_embedded_table_and_resample_is_unchanged(pair):
    of, nf = pair
    orig, new, width, kernels = audio.resample_kernels(of, nf)
    assert kernels.dtype == torch.float32 and tuple(kernels.shape) == (new, 2 * width + orig)
    assert (orig, new, width) == rate_geometry(of, nf)
    if pair in GEOMETRY:
        assert (orig, new, width, kernels.shape[1]) == GEOMETRY[pair]
    for shape in ((1,), (777,), (2, 3001)):
        x = _wave(int(np.prod(shape)), 5).reshape(shape)
        want, table = _resample_before(x, of, nf)
        assert torch.equal(kernels, table[:, 0])
        got = audio.resample(x, of, nf)
        assert got.shape == want.shape and torch.equal(got, want), f"{pair} {shape}: audio.resample changed"
    assert audio.resample(x, of, of) is x


def _taps64(g, kernels, x, j0, j1, src0=0, total=None, reads=None):
    """float64 tap evaluator: outputs [j0, j1) of the waveform whose samples [src0, src0 + len(x)) are `x` and whose length is `total` (None: unknown).
    Every tap inside [0, total) must be inside the buffer; `reads` collects the input indices touched."""
    out = torch.zeros(j1 - j0, dtype=torch.float64)
    k64, x64 = kernels.double().tolist(), x.double().tolist()
    for j in range(j0, j1):
        i, p = divmod(j, g.new)
        acc = 0.0
        for k in range(g.K):
            a = i * g.orig - g.width + k
            if a < 0 or (total is not None and a >= total):
                continue
            assert src0 <= a < src0 + x.shape[0], f"output {j} reads input {a}, outside the buffer [{src0}, {src0 + x.shape[0]})"
            if reads is not None:
                reads.add(a)
            acc += k64[p][k] * x64[a - src0]
        out[j - j0] = acc
    return out


@pytest.mark.parametrize("pair", PAIRS)
def test_index_rules_against_audio_resample(pair):
    of, nf = pair
    g = ResampleGeometry(of, nf)
    rng = np.random.Generator(np.random.Philox(key=21))
    worst = 0.0
    for trial in range(12):
        n = int(rng.integers(1, 5000)) if trial else g.width + g.orig
        x = _wave(n, 100 + trial)
        full = audio.resample(x, of, nf)
        assert full.shape[0] == g.out_total(n) == math.ceil(g.new * n / g.orig) and g.out_settled(n, True) == g.out_total(n) == g.out_settled(3, True, n)
        for S in sorted({0, 1, g.width - 1, g.width, g.width + g.orig - 1, g.width + g.orig, n, *[int(s) for s in rng.integers(0, n + 1, 4)]}):
            if S > n:
                continue
            J = g.out_settled(S)
            assert J == g.new * max(0, (S - g.width) // g.orig) and J % g.new == 0 and J <= g.out_total(S)
            if J:
                pre = audio.resample(x[:S], of, nf)
                err = float((pre[:J] - full[:J]).abs().max())
                worst = max(worst, err)
                assert err <= 4e-7, f"{pair} n={n} S={S}: the settled prefix differs from the whole waveform's by {err}"
                lo, hi = g.in_range(0, J)
                assert hi <= S and lo == -g.width, "a settled output reads an input at or beyond S"
            # tight to one frame, by index arithmetic: input S - 1 is a tap of output frame out_settled(S) // new, the first one NOT settled
            if S >= 1:
                f = J // g.new
                lo, hi = g.in_range(f * g.new, f * g.new + 1)
                assert lo <= S - 1 < hi and (lo, hi) == (f * g.orig - g.width, f * g.orig + g.orig + g.width)
                if f:
                    assert g.in_range((f - 1) * g.new, f * g.new)[1] <= S
    print(f"{pair}: settled prefix vs whole waveform, worst {worst:.3g}")
    # in_range: the union of the taps, exactly
    _, _, _, kernels = audio.resample_kernels(of, nf)
    x = _wave(4 * g.K + 50, 9)
    for j0, j1 in ((0, 1), (g.new + 1, g.new + 2), (1, 2 * g.new + 1), (g.new - 1, g.new)):
        reads = set()
        _taps64(g, kernels, x, j0, j1, reads=reads)
        lo, hi = g.in_range(j0, j1)
        assert reads == set(range(max(0, lo), hi)), f"{pair}: in_range({j0}, {j1}) = {(lo, hi)} is not the taps read"
    assert g.in_range(5, 5) == (0, 0) and g.lookback == 2 * g.width + g.orig - 1


def test_the_c_twins_equal_the_python_functions():
    lib = _lib.load()                                             # host code: loads without a GPU
    out = (C.c_int64 * 2)()
    for of, nf in PAIRS + [(24000, 11025), (7, 5)]:
        g = ResampleGeometry(of, nf)
        edge = [0, 1, g.width - 1, g.width, g.width + 1, g.width + g.orig - 1, g.width + g.orig, g.width + g.orig + 1, 30464, 2 ** 33 + 5]
        rng = np.random.Generator(np.random.Philox(key=22))
        for S in edge + [int(v) for v in rng.integers(0, 100000, 200)]:
            n = S + int(rng.integers(0, 1000))
            assert lib.ctts_resample_out_total(g.orig, g.new, n) == g.out_total(n)
            assert lib.ctts_resample_settled(g.orig, g.new, g.width, S, 0, n) == g.out_settled(S, False, n), f"{of}->{nf} S={S}"
            assert lib.ctts_resample_settled(g.orig, g.new, g.width, S, 1, n) == g.out_settled(S, True, n) == g.out_total(n)
        for j0 in [0, 1, g.new - 1, g.new, g.new + 1, 3 * g.new + g.new // 2, 2 ** 33 + 1] + [int(v) for v in rng.integers(0, 100000, 100)]:
            for cnt in (0, 1, g.new, g.new + 1, int(rng.integers(1, 5000))):
                assert lib.ctts_resample_in_range(g.orig, g.new, g.width, j0, j0 + cnt, out) == 0
                assert tuple(out) == g.in_range(j0, j0 + cnt), f"{of}->{nf} j0={j0} count={cnt}"
    assert lib.ctts_resample_in_range(3, 1, 19, -1, 4, out) == 1 and b"resample_in_range" in lib.ctts_last_error()
    names = {s[0] for s in _lib.SYMBOLS}
    assert {"ctts_resampler_create", "ctts_resampler_destroy", "ctts_resample_windows", "ctts_resample_settled", "ctts_resample_in_range"} <= names


@pytest.mark.parametrize("pair", PAIRS[:5])
def test_the_chunk_rule_covers_every_output_once_from_inside_its_window(pair):
    """SynthSession's rule for a resampled "exact" ticket, driven by a scripted sequence of settled counts: window (s0, s1, final) is vocoded from
    v0 = max(0, s0 - lookback) and yields outputs [J, J1), J1 = out_settled(s1, final, total).  The float64 evaluator refuses a tap outside [v0, s1)."""
    of, nf = pair
    g = ResampleGeometry(of, nf)
    _, _, _, kernels = audio.resample_kernels(of, nf)
    total = 2 * g.K + 7 * g.orig + 3
    x = _wave(total, 31)
    whole = _taps64(g, kernels, x, 0, g.out_total(total), 0, total)
    rng = np.random.Generator(np.random.Philox(key=23))
    for script in range(6):
        cuts = sorted({int(v) for v in rng.integers(1, total, 7)} | ({1, g.width, g.width + 1} if script == 0 else set()))
        J, s0, got, empty = 0, 0, [], 0
        for s1, final in [(c, False) for c in cuts] + [(total, True)]:
            v0 = max(0, s0 - g.lookback)
            J1 = g.out_settled(s1, final, total)
            assert J1 >= J
            if J1 > J or final:
                got.append((J, _taps64(g, kernels, x[v0:s1], J, J1, v0, total if final else None)))
            else:
                empty += 1
            J, s0 = J1, s1
        pos = 0
        for j, y in got:
            assert j == pos
            pos += y.shape[0]
        assert pos == g.out_total(total) and torch.equal(torch.cat([y for _, y in got]), whole)
    # the lookback is needed: one sample less and some window's first frame reads before its buffer
    short = False
    for s0 in range(g.lookback, g.lookback + 2 * g.orig + 2):
        J = g.out_settled(s0)
        short = short or g.in_range(J, J + 1)[0] < s0 - (g.lookback - 1)
        assert g.in_range(J, J + 1)[0] >= s0 - g.lookback
    assert short


def test_resampler_refuses_a_pair_beyond_the_limits_before_any_device_work():
    with pytest.raises(_lib.HipBackendError, match=r"24000 : 7 needs 65560 taps.*limits: 1024 taps"):
        Resampler(24000, 7, device="cpu")
    with pytest.raises(_lib.HipBackendError, match="identity"):
        Resampler(24000, 24000, device="cpu")


# ---- SessionBook: stream_lookback ---------------------------------------------------------------------------------------------------------------------------------------
def _replay(lookback):
    from tests.test_stream_session_host import Script, _book
    b = _book()
    kinds = ["exact", "eager", None, "exact", "exact"]
    lims = [150, 140, 90, 60, 3]
    ends, v0s = {}, {}
    for k, lim in zip(kinds, lims):
        kw = dict(stream_lookback=lookback) if (k == "exact" and lookback is not None) else {}
        tk = b.submit(10, 100 + len(ends), limit=lim, stream=k, stream_batch=None if k is None else 8, **kw)
        ends[tk] = (lim, 1)
    s = Script(b, ends)
    take = b.take_windows

    def spy():                                                    # v0 as DecodeSession._build_windows asks for it, window by window
        out = take()
        for tk, slot, n, s0, s1, final in out:
            v0s.setdefault(tk, []).append(b.window_v0(tk, s0, final))
        return out
    b.take_windows = spy
    s.run()
    assert not b._lookback, "a delivered ticket's lookback was kept"
    return s.windows, v0s, kinds


def test_session_book_lookback_keeps_the_windows_and_moves_v0():
    base, v_base, kinds = _replay(None)
    zero, v_zero, _ = _replay(0)
    assert zero == base and v_zero == v_base, "a lookback of 0 changed the windows"
    for tk, ws in base.items():
        assert v_base[tk] == [w[3] for w in ws]
    L = 173
    look, v_look, _ = _replay(L)
    assert look == base, "a lookback changed the (s0, s1) sequence"
    for tk, ws in base.items():
        want = [max(0, w[3] - L) if kinds[tk] == "exact" else w[3] for w in ws]
        assert v_look[tk] == want
    assert any(v < w[3] for tk in base for v, w in zip(v_look[tk], base[tk]))
    b = SessionBook(4, 6, 8, 400, 200)
    with pytest.raises(ValueError, match="stream_lookback"):
        b.submit(10, 1, stream="eager", stream_lookback=5)
    with pytest.raises(ValueError, match="stream_lookback"):
        b.submit(10, 1, stream_lookback=5)
    with pytest.raises(ValueError, match="stream_lookback"):
        b.submit(10, 1, stream="exact", stream_lookback=-1)
    assert not b.utts
    w = SessionWindow(0, 70, 512, 8448, False, 0, torch.zeros(70, 4, dtype=torch.int32))
    assert w.v0 == 512 and SessionWindow(0, 70, 512, 8448, False, 0, torch.zeros(70, 4, dtype=torch.int32), v0=339).v0 == 339
