"""ctts_dvae_encode_batch (DVAEEncoder.encode_batch): B clips in one launch sequence.  The contract is bit identity with the single-clip call
(ctts_dvae_encode, pinned by tests/test_gpu_encoder.py) whatever the batch, its order or its chunking -- every GEMM output element accumulates its K
range in the same order whatever M or the batch (conv_gemm.h), and the keyed kernels repeat the single-clip arithmetic term for term."""
import pytest
import torch

from chatttsplus_amd import _lib, synth
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

LENGTHS = [600, 16128, 16384, 12800, 50001]          # F = 3 / T = 1; F = 64 and 65 around a 64-row tile edge; two interior sizes
ORACLE_LENGTHS = [600, 12800, 50001, 191999]          # the inputs, seeds and bound of test_gpu_encoder.py::test_encode_vs_oracle_lengths


def _wave(n):
    return torch.from_numpy(synth.speaker_wave(100 + n, n))


def _encoder(max_seconds=8.0):
    from chatttsplus_amd.hip_models import DVAEEncoder
    e = DVAEEncoder(dim=512, max_seconds=max_seconds, pre_bound=True)
    return e.load_state_dict(synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234))


@pytest.fixture(scope="module")
def single():
    """length -> (ids, mel, feat) of the single-clip call, each on a fresh pass of one encoder that has served nothing else (computed once, never written)"""
    e = _encoder()
    return {n: tuple(t.clone() for t in e.encode(_wave(n), return_debug=True)) for n in sorted(set(LENGTHS + ORACLE_LENGTHS))}


def _same(got, single, lengths):
    assert len(got) == len(lengths)
    for u, (n, g) in enumerate(zip(lengths, got)):
        for name, a, b in zip(("ids", "mel", "feat"), g, single[n]):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"utterance {u} ({n} samples): {name} differs from the single-clip call"


def test_batch_is_bit_identical_to_the_single_clip_calls(single):
    e = _encoder()
    _same(e.encode_batch([_wave(n) for n in LENGTHS], return_debug=True), single, LENGTHS)
    rev = LENGTHS[::-1]                                   # same object: a short clip lands where a long one left data (stale guard rows would show)
    _same(e.encode_batch([_wave(n) for n in rev], return_debug=True), single, rev)
    for n in (600, 16384):                                # B = 1 through the batch entry
        _same(e.encode_batch([_wave(n)], return_debug=True), single, [n])
    ids = e.encode_batch([_wave(n) for n in LENGTHS])     # without the hooks: the codes alone
    assert all(torch.equal(i, single[n][0]) for i, n in zip(ids, LENGTHS))
    assert torch.equal(e.encode(_wave(12800)), single[12800][0])        # the single-clip call on the same object, after batches used its workspaces


def test_results_do_not_depend_on_the_chunking(single):
    # max_samples 50400: the batch workspace holds four regions of the longest clip, so the five clips are served as 4 + 1 (and, reversed, as 4 + 1 with
    # other members and another stride); the roomy encoder of the first test serves them in one chunk
    e = _encoder(max_seconds=2.1)
    _same(e.encode_batch([_wave(n) for n in LENGTHS], return_debug=True), single, LENGTHS)
    rev = LENGTHS[::-1]
    _same(e.encode_batch([_wave(n) for n in rev], return_debug=True), single, rev)
    twice = LENGTHS + rev                                 # ten clips: three chunks
    _same(e.encode_batch([_wave(n) for n in twice], return_debug=True), single, twice)


def test_batch_vs_oracle(single):
    sd = synth.dvae_encoder_state_dict(synth.DVAE_ENC_REAL, 1234)
    got = _encoder().encode_batch([_wave(n) for n in ORACLE_LENGTHS])
    for n, g in zip(ORACLE_LENGTHS, got):
        ref = ref_cpu.dvae_encode(sd, _wave(n)).numpy()
        g = g.cpu().numpy()
        assert g.shape == ref.shape == (4, ((1 + n // 256) - 2) // 2 + 1)
        assert (g != ref).mean() <= 0.005, f"n={n}: {(g != ref).sum()} of {ref.size} codes differ"


def test_a_refused_batch_names_the_clip_and_launches_nothing(single):
    e = _encoder()
    good = [_wave(n) for n in LENGTHS]
    with pytest.raises(_lib.HipBackendError, match="utterance 2"):
        e.encode_batch([good[1], good[3], torch.zeros(400), good[0]])              # reflect padding needs more than n_fft / 2 samples
    with pytest.raises(_lib.HipBackendError, match="utterance 1"):
        e.encode_batch([good[1], torch.zeros(8 * 24000 + 1), good[0]])             # longer than max_seconds
    with pytest.raises(_lib.HipBackendError):
        e.encode_batch([])                                                          # B < 1
    _same(e.encode_batch(good, return_debug=True), single, LENGTHS)
