"""The device resampler (hip_models.Resampler, ctts_resample_windows): whole ragged waveforms against a float64 evaluation of the same float32 table and input,
against audio.resample, and windows of them -- bit for bit -- against the whole-waveform call.

The accuracy bound is the textbook one for a K-term float32 sum in any order: |fl(sum) - sum| <= K u sum_k |h_k x_k| with u = 2^-24 (plus one rounding of the
float64 reference's own conversion: K + 1), evaluated per output sample from the same table and input.  Nothing in it is measured from the kernel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, audio

pytestmark = pytest.mark.gpu

PAIRS = [(24000, 8000), (24000, 16000), (24000, 22050), (24000, 44100), (24000, 48000), (44100, 24000)]
DEV = "cuda:0"
_cache = {}


def _case(pair):
    """one ragged batch per rate pair, resampled once (float and int16), with its references"""
    if pair in _cache:
        return _cache[pair]
    from chatttsplus_amd.hip_models import Resampler
    of, nf = pair
    rs = Resampler(of, nf, device=DEV)
    tile = rs.tile_outputs
    assert tile > 0 and tile % rs.new == 0
    long_n = math.ceil(3.3 * tile * rs.orig / rs.new) + 1                   # spans at least three tiles, whatever the tile is
    lens = [1, rs.width - 1, 0, rs.width + rs.orig, 40 * rs.orig, 40 * rs.orig + 1, 30464, long_n]
    g = torch.Generator().manual_seed(1000 + nf)
    xs = [torch.rand(n, generator=g) * 2 - 1 for n in lens]
    xs[4] = xs[4] * 1.6                                                     # leaves [-1, 1]: the int16 clamp is exercised
    xd = [x.to(DEV) for x in xs]
    ys = rs.resample(xd)
    ys16 = rs.resample(xd, pcm16=True)
    torch.cuda.synchronize()
    k64 = rs.kernels.double()[:, None]
    ref, bound = [], []
    for x in xs:
        xp = torch.nn.functional.pad(x.double(), (rs.width, rs.width + rs.orig))[None, None]
        y = torch.nn.functional.conv1d(xp, k64, stride=rs.orig)[0].t().reshape(-1)[:rs.out_total(x.shape[0])]
        s = torch.nn.functional.conv1d(xp.abs(), k64.abs(), stride=rs.orig)[0].t().reshape(-1)[:rs.out_total(x.shape[0])]
        ref.append(y)
        bound.append((rs.K + 1) * 2.0 ** -24 * s)
    _cache[pair] = dict(rs=rs, lens=lens, xs=xs, xd=xd, ys=ys, ys16=ys16, ref=ref, bound=bound, tile=tile)
    return _cache[pair]


@pytest.mark.parametrize("pair", PAIRS)
def test_whole_waveforms_against_float64_and_audio_resample(pair):
    c = _case(pair)
    rs = c["rs"]
    assert c["tile"] * 3 <= rs.out_total(c["lens"][-1])
    worst = worst_cpu = 0.0
    for u, n in enumerate(c["lens"]):
        y = c["ys"][u].cpu()
        assert y.dtype == torch.float32 and y.shape[0] == rs.out_total(n) == math.ceil(rs.new * n / rs.orig), f"{pair} n={n}: {y.shape[0]} outputs"
        if n == 0:
            continue
        err, b = (y.double() - c["ref"][u]).abs(), c["bound"][u]
        worst = max(worst, float((err / b.clamp_min(1e-300)).max()))
        assert bool((err <= b).all()), f"{pair} n={n}: sample {int((err - b).argmax())} is {float((err - b).max()):.3g} beyond its bound"
        cpu = audio.resample(c["xs"][u], *pair)
        assert cpu.shape == y.shape
        e2 = (y - cpu).abs().double()
        worst_cpu = max(worst_cpu, float((e2 / b.clamp_min(1e-300)).max()))
        assert bool((e2 <= 2 * b).all()), f"{pair} n={n}: differs from audio.resample by {float(e2.max()):.3g}"
    print(f"{pair}: K={rs.K} tile={c['tile']} outputs; worst |gpu - f64| / bound = {worst:.3f}, worst |gpu - audio.resample| / bound = {worst_cpu:.3f}")


@pytest.mark.parametrize("pair", PAIRS)
def test_int16_is_the_conversion_of_the_kernels_own_float_output(pair):
    c = _case(pair)
    clipped = False
    for y, p in zip(c["ys"], c["ys16"]):
        assert p.dtype == torch.int16 and p.shape == y.shape
        assert torch.equal(p, torch.round(torch.clamp(y, -1, 1) * 32767).to(torch.int16))
        clipped = clipped or bool((y.abs() > 1).any())
    assert clipped, "no sample left [-1, 1]: the clamp was never exercised"


def _windows(c, u):
    """(src, src0, total, j0, count) windows of waveform u (a long one); src is cut to in_range exactly unless noted"""
    rs, x, n, tile = c["rs"], c["xd"][u], c["lens"][u], c["tile"]
    J = rs.out_total(n)

    def cut(j0, cnt, total):
        lo, hi = rs.in_range(j0, j0 + cnt)
        lo, hi = max(0, lo), (min(hi, n) if total is not None else hi)      # total unknown: every right tap must be in the buffer
        assert 0 <= lo < hi <= n
        return (x[lo:hi], lo, total, j0, cnt)
    odd = tile + (1 if rs.new > 1 else 0) + rs.new * 3
    wins = [cut(odd, 2 * rs.new + 5, None),                                 # j0 % new != 0 (where new > 1), interior, the waveform's end unknown
            cut(tile - 5, 11, n),                                           # straddles the first tile boundary
            cut(2 * tile - rs.new - 1, tile + 2 * rs.new + 3, None),        # ... and covers a whole tile and both its boundaries
            cut(0, 37, None),                                               # the waveform's start: left zeros
            cut(J - 50, 50, n),                                             # its end, total known: right zeros
            cut(tile + 3, 301, None),                                       # interior, src0 > 0, total = -1
            (x[:0], 0, n, 5, 0),                                            # nothing asked
            (x, 0, n, 7, 64)]                                               # a window given the whole waveform as its buffer
    assert wins[0][3] % rs.new != 0 or rs.new == 1
    assert wins[5][1] > 0 and wins[0][1] > 0
    return wins


@pytest.mark.parametrize("pair", PAIRS)
def test_windows_are_bit_identical_to_the_whole_waveform_call(pair):
    c = _case(pair)
    rs = c["rs"]
    for u in (6, 7):                                                        # 30464 samples and the three-tile one
        whole = c["ys"][u]
        wins = _windows(c, u)
        alone = [rs.resample_windows([w[0]], [w[1]], [w[2]], [w[3]], [w[4]])[0] for w in wins[:7]]      # B = 1
        order = [4, 0, 6, 2, 5, 1, 3]                                       # B = 7, shuffled
        sel = [wins[i] for i in order]
        both = rs.resample_windows([w[0] for w in sel], [w[1] for w in sel], [w[2] for w in sel], [w[3] for w in sel], [w[4] for w in sel])
        mixed = rs.resample_windows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins], [w[3] for w in wins], [w[4] for w in wins])
        torch.cuda.synchronize()
        for i, w in enumerate(wins):
            want = whole[w[3]:w[3] + w[4]]
            assert want.shape[0] == w[4]
            got = [mixed[i]] + ([alone[i], both[order.index(i)]] if i < 7 else [])
            for k, y in enumerate(got):
                assert y.shape == want.shape and torch.equal(y, want), \
                    f"{pair} waveform {u} window {i} (j0={w[3]}, count={w[4]}, src0={w[1]}, total={w[2]}) call {k}: max diff {float((y - want).abs().max()):.3g}"
        p16 = rs.resample_windows([w[0] for w in sel], [w[1] for w in sel], [w[2] for w in sel], [w[3] for w in sel], [w[4] for w in sel], pcm16=True)
        for i, y in zip(order, p16):
            assert torch.equal(y, c["ys16"][u][wins[i][3]:wins[i][3] + wins[i][4]])


def _raw(rs, wins, out, offs, fmt=0):
    """ctts_resample_windows itself, into a buffer and at offsets of the test's choosing"""
    k = len(wins)
    arr = lambda v, t: np.ascontiguousarray(v, dtype=t)
    sp = (C.c_void_p * k)(*[w[0].data_ptr() if w[0].numel() else None for w in wins])
    s0, sn = arr([w[1] for w in wins], np.int64), arr([w[0].numel() for w in wins], np.int32)
    tt, jj = arr([-1 if w[2] is None else w[2] for w in wins], np.int64), arr([w[3] for w in wins], np.int64)
    ct, oo = arr([w[4] for w in wins], np.int32), arr(offs, np.int64)
    st = C.c_void_p(torch.cuda.current_stream(rs.device).cuda_stream)
    return rs._lib.ctts_resample_windows(rs._h, sp, s0.ctypes.data, sn.ctypes.data, tt.ctypes.data, jj.ctypes.data, ct.ctypes.data, k, C.c_void_p(out.data_ptr()),
                                         oo.ctypes.data, fmt, st)


@pytest.mark.parametrize("pair", [PAIRS[1], PAIRS[2]])
def test_no_store_outside_the_windows_and_refused_calls_write_nothing(pair):
    c = _case(pair)
    rs, u = c["rs"], 7
    x, n, whole = c["xd"][u], c["lens"][u], c["ys"][u]
    wins = _windows(c, u)[:6]
    SENT = -777.0
    offs, pos = [], 13
    for w in wins:
        offs.append(pos)
        pos += w[4] + 29                                                    # gaps between the windows, a margin before the first and behind the last
    out = torch.full((pos + 64,), SENT, device=DEV)
    assert _raw(rs, wins, out, offs) == 0
    torch.cuda.synchronize()
    keep = torch.ones_like(out, dtype=torch.bool)
    for w, o in zip(wins, offs):
        assert torch.equal(out[o:o + w[4]], whole[w[3]:w[3] + w[4]])
        keep[o:o + w[4]] = False
    assert bool((out[keep] == SENT).all()), "a store outside [out_off, out_off + count)"
    # refused calls: the window is named, nothing is written, and the next valid call is right
    j0, cnt = c["tile"] + 3, 301
    lo, hi = rs.in_range(j0, j0 + cnt)
    good = (x[lo:hi], lo, None, j0, cnt)
    bad = {"left": ((x[lo + 1:hi], lo + 1, None, j0, cnt), "window 2.*read input samples"),
           "right, total unknown": ((x[lo:hi - 1], lo, None, j0, cnt), "window 2.*total = -1"),
           "right, total known": ((x[lo:hi - 1], lo, n, j0, cnt), "window 2.*its buffer holds"),
           "beyond the waveform": ((x, 0, n, rs.out_total(n) - 3, 4), "window 2.*lie outside")}
    for what, (w, msg) in bad.items():
        out.fill_(SENT)
        assert _raw(rs, [good, wins[1], w], out, [0, 400, 800]) == 1, what
        with pytest.raises(_lib.HipBackendError, match=msg):
            _lib.check(1, "resample_windows")
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), f"{what}: the refused call wrote something"
        with pytest.raises(_lib.HipBackendError, match="window 0"):
            rs.resample_windows([w[0]], [w[1]], [w[2]], [w[3]], [w[4]])
        y = rs.resample_windows([good[0]], [lo], [None], [j0], [cnt])[0]
        assert torch.equal(y, whole[j0:j0 + cnt]), f"after a refused call ({what}) a valid one is wrong"


def test_a_rate_pair_beyond_the_limits_is_refused():
    from chatttsplus_amd.hip_models import Resampler
    with pytest.raises(_lib.HipBackendError, match="65560 taps"):
        Resampler(24000, 7, device=DEV)
    lib, h = _lib.load(), C.c_void_p()
    tab = np.zeros(7 * 65560, dtype=np.float32)
    assert lib.ctts_resampler_create(24000, 7, 20780, tab.ctypes.data, C.byref(h)) == 1 and not h.value
    assert b"65560 taps" in lib.ctts_last_error() and b"1024" in lib.ctts_last_error()
    c = _case(PAIRS[0])
    y = c["rs"].resample([c["xd"][6]])[0]
    assert torch.equal(y, c["ys"][6])
