"""hip_models.Resampler -- the output sample rate of the engine: torchaudio.functional.resample (sinc_interp_hann, width 6, roll-off 0.99; restated
on the CPU by chatttsplus_amd.audio.resample) as one HIP launch over ragged waveforms or streaming windows (csrc/resample.hip).

`ResampleGeometry` is the host-only part -- pure Python, no library, no GPU: the rate pair, its filter width, and the three index rules a streaming
integrator needs.  Output sample j = i new + p of an n-sample waveform x is sum_k kernels[p][k] x[i orig - width + k], k = 0 .. 2 width + orig - 1,
with x = 0 outside [0, n): output FRAME i (its `new` samples) reads inputs [i orig - width, i orig + orig + width)."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib


def rate_geometry(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[int, int, int]:
    """(orig, new, width) exactly as audio.resample_kernels computes them, without building the table"""
    if int(orig_freq) < 1 or int(new_freq) < 1:
        raise ValueError(f"resample: rates {orig_freq} -> {new_freq} (positive integers)")
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    return orig, new, math.ceil(lowpass_filter_width * orig / base)


class ResampleGeometry:
    """orig : new, width, K = 2 width + orig taps, and the index rules (ctts_resample_out_total / _settled / _in_range are their C twins)."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.orig, self.new, self.width = rate_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.K = 2 * self.width + self.orig
        # what a settled window [s0, s1) of a stream needs before s0: the left taps of its first new output frame
        self.lookback = 2 * self.width + self.orig - 1

    def out_total(self, n: int) -> int:
        """outputs of an n-sample waveform: ceil(new n / orig)"""
        n = int(n)
        return (self.new * n + self.orig - 1) // self.orig if n > 0 else 0

    def out_settled(self, S: int, finished: bool = False, n: Optional[int] = None) -> int:
        """Leading outputs that no input sample at or beyond S can change: every output frame whose last tap, input i orig + orig + width - 1, lies
        below S -- new * max(0, (S - width) // orig).  A finished n-sample waveform is settled to its end (the taps beyond n are the zeros of the
        result itself): out_total(n)."""
        if finished:
            return self.out_total(int(S) if n is None else int(n))
        return self.new * max(0, (int(S) - self.width) // self.orig)

    def in_range(self, j0: int, j1: int) -> Tuple[int, int]:
        """[lo, hi): the input samples outputs [j0, j1) can read, before clipping to [0, n); (0, 0) for an empty range"""
        j0, j1 = int(j0), int(j1)
        if j1 <= j0:
            return 0, 0
        return (j0 // self.new) * self.orig - self.width, ((j1 - 1) // self.new) * self.orig + self.orig + self.width


class Resampler(ResampleGeometry):
    """Owner of one native resampler handle (ctts_resampler: the filter table of one rate pair on the device)."""

    def __init__(self, orig_freq: int, new_freq: int, device="cuda"):
        super().__init__(orig_freq, new_freq)
        self.device = torch.device(device)
        self._h = C.c_void_p()
        if self.orig == self.new:
            raise _lib.HipBackendError(f"Resampler: {orig_freq} -> {new_freq} Hz is the identity; nothing to resample")
        # refused before the table is built: a pair far outside the limits would ask torch for gigabytes
        if self.K > _lib.RESAMPLE_MAX_TAPS or self.K * self.new * 4 > _lib.RESAMPLE_MAX_TABLE_BYTES:
            raise _lib.HipBackendError(f"Resampler: {orig_freq} -> {new_freq} Hz is outside the device resampler: the pair {self.orig} : {self.new} needs "
                                       f"{self.K} taps per output sample and a filter table of {self.K * self.new * 4} bytes "
                                       f"(limits: {_lib.RESAMPLE_MAX_TAPS} taps, {_lib.RESAMPLE_MAX_TABLE_BYTES} bytes)")
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipBackendError("infer_type='hip' needs a visible MI355X; no CPU fallback")
        from ..audio import resample_kernels
        orig, new, width, kernels = resample_kernels(orig_freq, new_freq)
        assert (orig, new, width) == (self.orig, self.new, self.width) and tuple(kernels.shape) == (self.new, self.K)
        self.kernels = kernels.contiguous()                # [new, K] float32, host: the table the device holds
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_resampler_create(self.orig, self.new, self.width, C.c_void_p(self.kernels.data_ptr()), C.byref(self._h)),
                       "ctts_resampler_create")
        self.tile_outputs = self.new * int(self._lib.ctts_resampler_tile_frames(self._h))      # outputs [t, t + 1) * tile_outputs share a workgroup

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._lib.ctts_resampler_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def resample_windows(self, srcs: Sequence[torch.Tensor], src0s, totals, j0s, counts, pcm16: bool = False) -> List[torch.Tensor]:
        """Outputs [j0s[u], j0s[u] + counts[u]) of window u, whose waveform's input samples [src0s[u], src0s[u] + len(srcs[u])) are srcs[u] (float32, on
        the device) and whose length is totals[u] (-1 or None: not known yet).  One launch (per RESAMPLE_MAX_WINDOWS windows), one output allocation;
        views of it are returned, float32 or -- `pcm16` -- int16 PCM (rintf(clamp(y, -1, 1) * 32767)).  A count of 0 yields an empty view."""
        B = len(srcs)
        counts = [int(c) for c in counts]
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + max(0, c))
        out = torch.empty(offs[-1], dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        xs = [s.to(self.device, dtype=torch.float32).contiguous() for s in srcs]
        M = _lib.RESAMPLE_MAX_WINDOWS
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for c0 in range(0, B, M):
                idx = list(range(c0, min(B, c0 + M)))
                k = len(idx)
                sp = (C.c_void_p * k)(*[xs[u].data_ptr() if xs[u].numel() else None for u in idx])
                s0 = np.ascontiguousarray([int(src0s[u]) for u in idx], dtype=np.int64)
                sn = np.ascontiguousarray([int(xs[u].numel()) for u in idx], dtype=np.int32)
                tt = np.ascontiguousarray([-1 if totals[u] is None else int(totals[u]) for u in idx], dtype=np.int64)
                jj = np.ascontiguousarray([int(j0s[u]) for u in idx], dtype=np.int64)
                ct = np.ascontiguousarray([counts[u] for u in idx], dtype=np.int32)
                oo = np.ascontiguousarray([offs[u] for u in idx], dtype=np.int64)
                try:
                    _lib.check(self._lib.ctts_resample_windows(self._h, sp, s0.ctypes.data, sn.ctypes.data, tt.ctypes.data, jj.ctypes.data, ct.ctypes.data, k,
                                                               C.c_void_p(out.data_ptr()), oo.ctypes.data, 1 if pcm16 else 0, st), "resample_windows")
                except _lib.HipBackendError as e:
                    if c0:                                 # (the message names the window of THIS launch)
                        raise _lib.HipBackendError(f"{e} (windows are numbered from {c0} of the call)") from None
                    raise
        return [out[offs[u]:offs[u + 1]] for u in range(B)]

    def resample(self, wavs: Sequence[torch.Tensor], pcm16: bool = False) -> List[torch.Tensor]:
        """Every whole waveform of `wavs` ([n_u] float32 on the device, ragged, empty ones allowed) at the new rate: out_total(n_u) samples each."""
        ns = [int(w.numel()) for w in wavs]
        return self.resample_windows([w.reshape(-1) for w in wavs], [0] * len(ns), ns, [0] * len(ns), [self.out_total(n) for n in ns], pcm16)
