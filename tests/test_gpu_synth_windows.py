"""ctts_synth_windows: the DVAE + Vocos stack of ctts_synth_batch with a last kernel that overlap-adds only a sample window per utterance into one packed buffer
(float32 or int16 PCM), and the settled-sample rule (vocoder.settled_samples) it serves: samples of a prefix waveform that no later token changes."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.hip_models import vocoder as vmod

pytestmark = pytest.mark.gpu

LENS = (130, 37, 60, 1)
SENT = -777.0


@pytest.fixture(scope="module")
def voc():
    from chatttsplus_amd.hip_models import Synth
    s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 140 + 64, max_batch=4)
    s.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    s.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    rng = np.random.Generator(np.random.Philox(key=4401))
    hs = [torch.from_numpy(rng.standard_normal((n, 768)).astype(np.float32)).cuda() for n in LENS]
    full = s.decode_batch(hs)                        # the reference of every test here: computed once, never written
    return s, hs, full


def _raw(s, srcs, skips, counts, offs, out, fmt, codes=0):
    k = len(srcs)
    hp = (C.c_void_p * k)(*[h.data_ptr() for h in srcs])
    arr = [(C.c_int32 * k)(*[int(x) for x in v]) for v in ([h.shape[0] for h in srcs], skips, counts, offs)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = s._lib.ctts_synth_windows(s._h, hp, arr[0], arr[1], arr[2], k, out.data_ptr(), arr[3], fmt, codes, st)
    torch.cuda.synchronize()
    return rc


# windows per utterance (skip, count): at the start, in the interior, at the end, ragged, a count of 0
CASES = [
    [(0, 5000), (0, 300), (0, 1), (0, 256)],
    [(20000, 7000), (9000, 1111), (15000, 513), (100, 100)],
    [(256 * 259 - 4000, 4000), (256 * 73 - 999, 999), (256 * 119 - 1, 1), (0, 256)],
    [(0, 256 * 259), (5, 0), (30000, 77), (255, 1)],
    [(12345, 0), (0, 256 * 73), (0, 0), (0, 0)],
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_float_windows_are_slices_packed_back_to_back(voc, case):
    s, hs, full = voc
    win = CASES[case]
    gap = 3                                           # sentinel samples in front of, between and behind the windows
    offs, pos = [], gap
    for _, c in win:
        offs.append(pos)
        pos += c + gap
    out = torch.full((pos,), SENT, device="cuda")
    assert _raw(s, hs, [a for a, _ in win], [c for _, c in win], offs, out, 0) == 0, s._lib.ctts_last_error()
    keep = torch.ones(pos, dtype=torch.bool, device="cuda")
    for u, ((a, c), o) in enumerate(zip(win, offs)):
        assert torch.equal(out[o:o + c], full[u][a:a + c]), f"utterance {u}, samples [{a}, {a + c}): max diff {float((out[o:o + c] - full[u][a:a + c]).abs().max())}"
        keep[o:o + c] = False
    assert bool((out[keep] == SENT).all()), "a store outside the windows"
    # the Python entry: one allocation, views of it, the same samples
    got = s.synth_windows(hs, [a for a, _ in win], [c for _, c in win])
    base = got[0].untyped_storage().data_ptr()
    for u, (a, c) in enumerate(win):
        assert got[u].untyped_storage().data_ptr() == base and torch.equal(got[u], full[u][a:a + c])


def test_pcm16_is_the_rounded_clamped_float_result(voc):
    s, hs, full = voc
    win = CASES[1]
    offs = np.cumsum([0] + [c for _, c in win])
    f32 = torch.full((int(offs[-1]) + 1,), SENT, device="cuda")
    i16 = torch.full((int(offs[-1]) + 1,), -5, dtype=torch.int16, device="cuda")
    for out, fmt in ((f32, 0), (i16, 1)):
        assert _raw(s, hs, [a for a, _ in win], [c for _, c in win], offs[:-1], out, fmt) == 0
    want = torch.clamp(f32[:-1], -1, 1).mul(32767).round().to(torch.int16)
    assert torch.equal(i16[:-1], want) and int(i16[-1]) == -5 and float(f32[-1]) == SENT
    got = s.synth_windows(hs, [a for a, _ in win], [c for _, c in win], pcm16=True)
    assert all(g.dtype == torch.int16 for g in got) and torch.equal(torch.cat(got), want)


def test_pcm16_clamps(voc):
    """The synthetic checkpoint's waveforms stay below 0.1 (the stack's LayerNorms undo any scaling of the input), so this handle's ISTFT head gets +5 on its
    log-magnitude biases: the waveform leaves [-1, 1] and the PCM saturates at +-32767."""
    from chatttsplus_amd.hip_models import Synth
    _, hs, _ = voc
    vsd = synth.vocos_state_dict(synth.VOCOS_REAL, 1234)
    vsd["head.out.bias"] = vsd["head.out.bias"].copy()
    vsd["head.out.bias"][:513] += 5.0
    s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 40 + 64, max_batch=1)
    s.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    s.load("vocos.", vsd)
    big = [hs[1]]
    f = s.synth_windows(big, [0], [256 * 73])[0]
    p = s.synth_windows(big, [0], [256 * 73], pcm16=True)[0]
    print(f"|wav| max {float(f.abs().max()):.3f}; {int((f.abs() > 1).sum())} of {f.numel()} samples outside [-1, 1]")
    assert torch.equal(p, torch.clamp(f, -1, 1).mul(32767).round().to(torch.int16))
    assert bool((f.abs() > 1).any()) and int(p.abs().max()) == 32767, "the input never left [-1, 1]: the clamp was not exercised"


def test_refusals(voc):
    s, hs, full = voc
    out = torch.full((64,), SENT, device="cuda")
    for skips, counts, what in (([256 * 259 - 10], [11], "outside"), ([-1], [4], "outside"), ([0], [-1], "outside")):
        assert _raw(s, hs[:1], skips, counts, [0], out, 0) == 1 and what.encode() in s._lib.ctts_last_error()
    assert _raw(s, hs[:1], [0], [4], [0], out, 2) == 1 and b"fmt" in s._lib.ctts_last_error()
    assert _raw(s, hs[:1], [0], [4], [0], out, 0, codes=1) == 1 and b"quantiser" in s._lib.ctts_last_error()
    assert bool((out == SENT).all())


def test_codes_mode_equals_synth_batch_codes():
    from chatttsplus_amd.hip_models import Synth
    cfg = synth.DVAE_FULL_DEC
    s = Synth(dict(cfg), dict(synth.VOCOS_REAL), max_frames=2 * 140 + 64, max_batch=4, vq_cfg=dict(dim=1024, levels=[5, 5, 5, 5], G=2, R=2))
    s.load("dvae.", synth.dvae_full_decoder_state_dict(cfg, 1234))
    s.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    rng = np.random.Generator(np.random.Philox(key=4402))
    ids = [torch.from_numpy(rng.integers(0, 625, size=(n, 4)).astype(np.int32)).cuda() for n in LENS]
    full = s.decode_batch(ids)                        # ctts_synth_batch_codes
    for win in (CASES[1], CASES[3]):
        got = s.synth_windows(ids, [a for a, _ in win], [c for _, c in win])
        for u, (a, c) in enumerate(win):
            assert torch.equal(got[u], full[u][a:a + c]), f"codes mode, utterance {u}, samples [{a}, {a + c})"
    w = s.decode_window(ids, [1000, 0, 60000, 0], [3000, 256 * 73, 66000, 256])
    assert torch.equal(w[0], full[0][1000:3000]) and torch.equal(w[1], full[1]) and w[2].numel() == 0 and torch.equal(w[3], full[3])


@pytest.mark.parametrize("n", [53, 54, 60, 97, 139])
def test_settled_samples_do_not_change_when_tokens_follow(n):
    """THE property "exact" streaming rests on: the first settled_samples(n) samples of the n-token prefix waveform are those of the whole utterance, bit for
    bit.  If this fails at the derived bound the bound is wrong (HALO_FRAMES misses a dependency) -- it is not a matter of tolerance."""
    s, h, whole = _long()
    st = vmod.settled_samples(n, 256, s.HALO_FRAMES)
    assert st == 256 * max(0, 2 * n - s.HALO_FRAMES - 2)
    pre = s.decode_batch([h[:n]])[0]
    d = (pre - whole[:pre.shape[0]]).abs()
    first = int(torch.nonzero(d > 0)[0]) if bool((d > 0).any()) else -1
    print(f"n = {n}: {st} settled samples of {pre.shape[0]}; the prefix waveform first differs from the whole utterance's at sample {first}")
    assert torch.equal(pre[:st], whole[:st])
    assert first >= st                               # (and the tail does differ: the test can see a change)
    if st > 0:
        # the settled window vocoded from its own token range -- not from the n-token prefix -- is the same
        a, b, off, s0, s1 = vmod.settled_token_range(n, max(0, st - 3000), st, 256, s.HALO_FRAMES)
        assert b <= n
        w = s.synth_windows([h[a:b]], [s0 - off], [s1 - s0])[0]
        assert torch.equal(w, whole[s0:s1])


_long_cache = []


def _long():
    if not _long_cache:
        from chatttsplus_amd.hip_models import Synth
        s = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 140 + 64, max_batch=1)
        s.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
        s.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
        h = torch.from_numpy(np.random.Generator(np.random.Philox(key=4403)).standard_normal((140, 768)).astype(np.float32)).cuda()
        _long_cache.append((s, h, s.decode_batch([h])[0]))
    return _long_cache[0]
