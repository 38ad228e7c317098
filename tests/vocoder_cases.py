"""The case table of the vocoder parity checks and the helpers every user of it shares (test infrastructure): tests/test_vocoder_parity_host.py (CPU: the
cases stay inside the kernels' documented range on the reference alone), tests/test_gpu_vocoder_parity.py (the kernels against float64) and
tools/vocoder_parity.py (the record, profiles/vocoder_parity.jsonl).

A case = one entry point (`kind`), one size, one checkpoint variant, one input scale.  Its reference is the oracle in float64; its YARDSTICK is the worst-frame
error of the float32 oracle against that reference -- computed on the CPU from the reference alone, never from a kernel's output.  The kernels have to stay
within FACTOR times the yardstick in every frame (tests.helpers.per_frame_err).

FACTOR = 8: the split product drops only the tail x tail term (<= 2^-22 per product) and accumulates in fp32 like the oracle; two correct fp32
implementations that differ in summation order and in erff / expf / cosf rounding differ by a small multiple of the f32-vs-f64 error; three bits of
headroom cover that and the bound stays ~200 times tighter than the 1e-3 global rms of tests/test_gpu_vocoder.py."""
import functools
from dataclasses import dataclass
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F_real

from chatttsplus_amd import synth
from oracle import ref_cpu
from tests.helpers import per_frame_err

FACTOR = 8.0
ACT_LIMIT = 65504.0 / 4          # largest |activation| a case may feed a GEMM in the float64 reference: a factor 4 below the kernels' clamp
SEED = 1234
N_MELS, HOP = 100, 256
VQ_CFG = dict(dim=1024, levels=[5, 5, 5, 5], G=2, R=2)


@dataclass(frozen=True)
class Case:
    id: str
    kind: str                    # "dvae": hidden [n, 768] -> mel; "vocos": mel [100, F] -> wav; "codes": ids [n, 4] -> mel (DVAE_full decoder, 256 wide);
    size: int                    # "chain": hidden -> wav through decode_batch.  size = tokens n (frames 2n), or frames F for "vocos"
    variant: str = "plain"       # checkpoint pair, see VARIANTS
    scale: float = 1.0           # multiplier of the N(0, 1) input
    key: int = 0                 # Philox key of the input


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------------------------------

def _scaled(sd, suffix, factor):
    return {k: (v * np.float32(factor)).astype(np.float32) if k.endswith(suffix) else v for k, v in sd.items()}


def _norm_outliers(sd):
    out = dict(sd)
    for k, v in sd.items():
        if ".decoder_block." in k and k.endswith("norm.weight"):
            w = v.copy()
            w[::37] *= np.float32(20.0)
            out[k] = w
    return out


def _one_weight(sd, value):
    out = dict(sd)
    w = out["decoder.conv_in.0.weight"].copy()
    w[0, 0, 0] = np.float32(value)
    out["decoder.conv_in.0.weight"] = w
    return out


# variant -> (DVAE transform, Vocos transform) of the seed-1234 synthetic checkpoints.  Each stress handle carries one DVAE and one Vocos stress at once
# (a "dvae" case never runs the Vocos half and the other way round), so three handles serve the six stress checkpoints.
VARIANTS = {
    "plain": (lambda d: d, lambda v: v),
    "gamma0": (lambda d: _scaled(d, "gamma", 0.0), lambda v: _scaled(v, "gamma", 0.0)),          # ConvNeXt blocks off: only the gemm_split_kernel stages (and the LayerNorms) remain
    "gamma3.3": (lambda d: _scaled(d, "gamma", 3.3), lambda v: _scaled(v, "gamma", 3.3)),        # gamma up to ~1.0: the blocks dominate the stream
    "outliers+headx8": (lambda d: _norm_outliers(_scaled(d, "gamma", 3.3)),                      # DVAE: every 37th norm.weight x 20 with gamma x 3.3 (run at hidden x 30)
                        lambda v: _scaled(v, "head.out.weight", 8.0)),                           # Vocos: many bins in the clip(exp, 1e2), phases of tens of radians
    "w255.875": (lambda d: _one_weight(d, 255.875), lambda v: v),                                # the largest weight the split images hold: 256 * 255.875 = 65504
    "w256": (lambda d: _one_weight(d, 256.0), lambda v: v),                                      # refused at load
}


@functools.lru_cache(maxsize=None)
def dvae_sd(variant, full=False):
    base = synth.dvae_full_decoder_state_dict(synth.DVAE_FULL_DEC, SEED) if full else synth.dvae_state_dict(synth.DVAE_REAL, SEED)
    return VARIANTS[variant][0](base)


@functools.lru_cache(maxsize=None)
def vocos_sd(variant):
    return VARIANTS[variant][1](synth.vocos_state_dict(synth.VOCOS_REAL, SEED))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------------
# Edge lengths: 16-frame fragment groups, 64-row GEMM tiles / 64 x 64 cnx blocks, the 4-frame dwconv blocks, the 128 / 130 edge.
DVAE_EDGES = (1, 7, 8, 9, 31, 32, 33, 64, 65)                    # tokens: frames 2n
VOCOS_EDGES = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129)      # frames
CODES_EDGES = (8, 9, 33)
BATCH_TOKENS = (33, 8, 65, 1, 32, 9, 64, 7)                      # one decode_batch call on the 8-lane handle

CASES = (
    [Case(f"dvae-n{n}", "dvae", n, key=3000 + n) for n in DVAE_EDGES]
    + [Case(f"vocos-F{f}", "vocos", f, key=4000 + f) for f in VOCOS_EDGES]
    + [Case(f"codes-n{n}", "codes", n, key=5000 + n) for n in CODES_EDGES]
    + [Case(f"batch-u{u}-n{n}", "chain", n, key=6000 + u) for u, n in enumerate(BATCH_TOKENS)]
    # stress: DVAE at n = 33, Vocos at F = 65
    + [Case(f"dvae-hidden-x{s:g}", "dvae", 33, scale=s, key=7001) for s in (1e-3, 30.0, 300.0)]
    + [Case("dvae-gamma-x0", "dvae", 33, "gamma0", key=7001), Case("dvae-gamma-x3.3", "dvae", 33, "gamma3.3", key=7001),
       Case("dvae-norm-outliers", "dvae", 33, "outliers+headx8", scale=30.0, key=7001)]
    + [Case(f"vocos-mel-x{s:g}", "vocos", 65, scale=s, key=7002) for s in (0.01, 4.0)]
    + [Case("vocos-gamma-x0", "vocos", 65, "gamma0", key=7002), Case("vocos-gamma-x3.3", "vocos", 65, "gamma3.3", key=7002),
       Case("vocos-head-x8", "vocos", 65, "outliers+headx8", key=7002)]
    # range: the largest weight that loads
    + [Case("dvae-weight-255.875", "dvae", 8, "w255.875", key=7003)]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def case_input(c):
    """The case's input: hidden [n, 768] / mel [100, F] float32 = scale x N(0, 1), or ids [n, 4] int64 in [0, 625)."""
    rng = np.random.Generator(np.random.Philox(key=c.key))
    if c.kind == "codes":
        return rng.integers(0, 625, size=(c.size, 4), dtype=np.int64)
    shape = (N_MELS, c.size) if c.kind == "vocos" else (c.size, 768)
    return (rng.standard_normal(shape).astype(np.float32) * np.float32(c.scale)).astype(np.float32)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------------------

class _Seen:
    """Largest |activation| entering a GEMM of the oracle: the input of every dense Conv1d (depthwise convs are not GEMMs) and every Linear -- the DVAE input rows, the
    GELU output of conv_in.0, each block's LayerNorm and GELU output, the inputs of conv_out and out_conv, the mel, the final LayerNorm output -- plus the
    spectrum (the ISTFT GEMM's input) and the produced mel."""

    def __init__(self):
        self.max_act = 0.0

    def see(self, x):
        m = float(x.abs().max())
        self.max_act = m if (m != m or m > self.max_act) else self.max_act          # a NaN sticks


class _FShim:
    def __init__(self, seen):
        self._seen = seen

    def __getattr__(self, name):
        return getattr(F_real, name)

    def conv1d(self, x, w, b=None, **kw):
        if kw.get("groups", 1) == 1:
            self._seen.see(x)
        return F_real.conv1d(x, w, b, **kw)

    def linear(self, x, w, b=None):
        self._seen.see(x)
        return F_real.linear(x, w, b)


def _oracle(c, x, dtype, seen=None):
    """The oracle's output for case c in `dtype` (numpy float64 array); with `seen`, records the GEMM inputs on the way."""
    def run():
        if c.kind == "vocos":
            return ref_cpu.vocos_decode(vocos_sd(c.variant), torch.from_numpy(x), dtype=dtype)
        if c.kind == "codes":
            mel = ref_cpu.dvae_decode_codes(dvae_sd(c.variant, True), torch.from_numpy(x), dtype=dtype)
        else:
            mel = ref_cpu.dvae_decode(dvae_sd(c.variant), torch.from_numpy(x), dtype=dtype)
        if seen is not None:
            seen.see(mel)
        return ref_cpu.vocos_decode(vocos_sd(c.variant), mel, dtype=dtype) if c.kind == "chain" else mel
    if seen is None:
        return run().double().numpy()
    head = ref_cpu.vocos_head_spec

    def head_seen(*a, **k):
        re, im = head(*a, **k)
        seen.see(re), seen.see(im)
        return re, im
    with mock.patch.object(ref_cpu, "F", _FShim(seen)), mock.patch.object(ref_cpu, "vocos_head_spec", head_seen):
        return run().double().numpy()


def axis_len(c):
    return N_MELS if c.kind in ("dvae", "codes") else HOP


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """Computed once per process and shared (treat as read-only): the float64 reference, the float32 oracle's worst-frame and global error against it (the
    yardstick) and the largest activation the float64 run fed a GEMM."""
    c = BY_ID[case_id]
    x = case_input(c)
    seen = _Seen()
    ref64 = _oracle(c, x, torch.float64, seen)
    ref32 = _oracle(c, x, torch.float32)
    ref64.setflags(write=False)
    return dict(ref64=ref64, yard=float(np.max(per_frame_err(ref32, ref64, axis_len(c)))), f32_global=global_err(ref32, ref64), max_act=seen.max_act,
                finite=bool(np.isfinite(ref64).all()))


def global_err(got, ref64):
    d = np.asarray(got, dtype=np.float64) - ref64
    return float(np.sqrt(np.mean(np.square(d))) / np.sqrt(np.mean(np.square(ref64))))


def measure(c, got):
    """What the test asserts on and the tool records for one kernel output."""
    r = reference(c.id)
    worst = float(np.max(per_frame_err(got, r["ref64"], axis_len(c))))
    return dict(case=c.id, kind=c.kind, size=c.size, variant=c.variant, scale=c.scale, kernel_worst_frame=worst, f32_oracle_worst_frame=r["yard"],
                ratio=worst / r["yard"], kernel_global_rms=global_err(got, r["ref64"]), f32_oracle_global_rms=r["f32_global"], max_act_f64=r["max_act"])


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------------------

def open_synth(variant="plain", full=False, max_frames=192, max_batch=1):
    """A loaded native handle for a checkpoint variant (`full`: the 256-wide DVAE_full decoder taking code ids)."""
    from chatttsplus_amd.hip_models import Synth
    s = Synth(dict(synth.DVAE_FULL_DEC if full else synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=max_frames, max_batch=max_batch,
              vq_cfg=dict(VQ_CFG) if full else None)
    try:
        s.load("dvae.", dvae_sd(variant, full))
        s.load("vocos.", vocos_sd(variant))
    except Exception:
        close_synth(s)
        raise
    return s


def close_synth(s):
    s.__del__()          # frees the native handle now (idempotent)


def run_kernel(c, s):
    """Case c through its single-utterance entry point on handle s -> numpy."""
    x = torch.from_numpy(case_input(c)).cuda()
    if c.kind == "dvae":
        out = s.dvae_decode(x)
    elif c.kind == "vocos":
        out = s.vocos_decode(x)
    elif c.kind == "codes":
        out = s.dvae_decode_codes(x)
    else:
        out = s.decode_batch([x])[0]
    return out.cpu().numpy()


def run_batch(cases, s):
    """The "chain" cases in ONE decode_batch call -> [numpy]."""
    outs = s.decode_batch([torch.from_numpy(case_input(c)).cuda() for c in cases])
    return [o.cpu().numpy() for o in outs]


def fmt(m):
    return (f"{m['case']}: kernel worst frame {m['kernel_worst_frame']:.3e}, float32 oracle {m['f32_oracle_worst_frame']:.3e}, ratio {m['ratio']:.2f} "
            f"(bound {FACTOR:g}); global rms {m['kernel_global_rms']:.3e}; max |activation| {m['max_act_f64']:.3g}")
