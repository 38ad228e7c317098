"""The case table of the clip-encoder parity checks and the helpers every user of it shares (test infrastructure): tests/test_encoder_parity_host.py (CPU: the
float64 oracle, and every case inside its conditions on the reference alone), tests/test_gpu_encoder_parity.py (csrc/encoder.hip against float64) and
tools/encoder_parity.py (the record, profiles/encoder_parity.jsonl).

A case = one waveform, one checkpoint variant.  Its reference (`ref64`) is the oracle in float64 from the waveform.  Three quantities are compared frame by frame
(tests.helpers.per_frame_err), each against a YARDSTICK computed on the CPU from the reference alone, never from a kernel's output: the worst-frame error of the
FLOAT32 oracle in its "dft" form (ref_cpu.mel_features(form="dft"): the kernel's formulation of the STFT, a 1024-term fp32 dot product -- an fp32 FFT rounds
differently by design and its yardstick is up to 6 times smaller) against ref64, floored at 2^-23 (one fp32 ulp relative to the rms: the all-zeros clip's own
yardstick only says that the oracle rounded luckily).
  log-mel / coef   the debug hook [100][F]
  linear mel       exp(coef * hook) of both sides, evaluated in float64: well conditioned where the log form is not (leakage bins at the 1e-5 floor)
  features         [T][1024], compared as [1024][T]
The kernel has to stay within FACTOR = 8 times the yardstick in every frame (the constant and its rationale: tests/vocoder_cases.py; gemm_f32_kernel accumulates
in fp32 like the oracle).  A case takes part in the log-mel and feature checks only if those yardsticks are <= YARD_LIMIT = 1e-4 (ten times inside the old 1e-3
global rms); `dc` and `nyquist` do not, and are declared linear-mel-only here.

Codes: a teacher-forced digit check on the kernel's OWN features (digit_check) with eps[r] = FACTOR x the largest |float32 - float64| pre-round difference at
residual level r of the oracle's GFSQ, both on ref64's features rounded to float32 (quant_reference)."""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from chatttsplus_amd import synth
from oracle import ref_cpu
from tests.helpers import per_frame_err
from tests.vocoder_cases import FACTOR, _norm_outliers, _scaled

SEED = 1234
N_MELS, HOP, N_FFT, ODIM = 100, 256, 1024, 1024
YARD_FLOOR = 2.0 ** -23
YARD_LIMIT = 1e-4
TIE_SHARE_LIMIT = 0.01           # at most this share of a case's float64 digits may lie within eps of a rounding boundary (the digit check is blind there)
HALF_L = 2.002                   # (levels - 1) * (1 + 1e-3) / 2


@dataclass(frozen=True)
class Case:
    id: str
    n: int                       # samples
    family: str = "speech"       # the waveform, see case_input
    variant: str = "plain"       # the checkpoint, see VARIANTS
    linear_only: bool = False    # takes part in the linear-mel check only (its log-mel / feature yardsticks exceed YARD_LIMIT)

    @property
    def frames(self):
        return 1 + self.n // HOP

    @property
    def codes(self):
        return (self.frames - 2) // 2 + 1


# quantiser shapes: name -> (G, R, pre_bound).  The conv stack does not depend on them: one set of reference features serves all three.
QUANTS = {"g2r2": (2, 2, True), "g2r2-nobound": (2, 2, False), "g4r4": (4, 4, True)}

# checkpoint variants of the seed-1234 synthetic encoder (the helpers of the vocoder table)
VARIANTS = {
    "plain": lambda d: d,
    "gamma0": lambda d: _scaled(d, "gamma", 0.0),                                  # ConvNeXt blocks off: only the conv GEMMs remain
    "gamma3.3": lambda d: _scaled(d, "gamma", 3.3),                                # the blocks dominate the stream
    "outliers": lambda d: _norm_outliers(_scaled(d, "gamma", 3.3)),                # ... plus every 37th norm.weight x 20
    "coef0.05": lambda d: _scaled(d, "coef", 0.05),                                # the mel image x 20 into downsample_conv.0
    "coef20": lambda d: _scaled(d, "coef", 20.0),                                  # ... and x 0.05
}


@functools.lru_cache(maxsize=None)
def encoder_sd(variant="plain", quant="g2r2"):
    G, R, _ = QUANTS[quant]
    cfg = dict(synth.DVAE_ENC_REAL, vq_G=G, vq_R=R)
    return VARIANTS[variant](synth.dvae_encoder_state_dict(cfg, SEED))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------------
# n (F, T): the smallest legal clip; odd and even F (whether the stride-2 k4 conv's last window reads the guard row); T = 1 .. 7 (the dilated depthwise taps
# leave the clip on both sides); the 4-frame dwconv blocks; both sides of the 64-row tile at F and at T; n on and off a hop multiple (the reflect tail).
EDGE_LENGTHS = (513, 767, 768, 1279, 1536, 2048, 2304, 3328, 4095, 8192, 8448, 16128, 16384, 16640, 32512, 33023, 33280)
STRESS_N = 16640
CAPACITY_N = 24000               # exactly max_seconds = 1.0
FAMILIES = ("x1e-3", "zeros", "x32768", "gap", "impulse", "dc", "nyquist")
NONFINITE_N, NONFINITE_AT = 16384, 8000

CASES = (
    [Case(f"n{n}", n) for n in sorted(EDGE_LENGTHS, reverse=True)]              # longest first: on one handle every short clip meets a dirty workspace
    + [Case(f"wave-{f}", STRESS_N, family=f, linear_only=f in ("dc", "nyquist")) for f in FAMILIES]
    + [Case(f"ckpt-{v}", STRESS_N, variant=v) for v in VARIANTS if v != "plain"]
    + [Case("capacity-n24000", CAPACITY_N)]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
EDGES = [c for c in CASES if c.family == "speech" and c.variant == "plain" and c.n in EDGE_LENGTHS]
BATCH_ORDER = (2048, 33280, 513, 16384, 768, 8448, 33023, 1279, 16128, 3328, 767, 32512, 1536, 4095, 16640, 2304, 8192)      # the edge lengths, shuffled
assert sorted(BATCH_ORDER) == sorted(EDGE_LENGTHS)


def speech(n):
    return synth.speaker_wave(100 + n, n)


def case_input(c):
    """The case's waveform, float32 [n]."""
    n = c.n
    if c.family == "zeros":
        return np.zeros(n, dtype=np.float32)
    if c.family == "dc":
        return np.full(n, 0.5, dtype=np.float32)                                  # DFT basis row 0
    if c.family == "nyquist":
        return (0.5 * (-1.0) ** np.arange(n)).astype(np.float32)                  # basis row 512, and mag columns 513 .. 527 beside it
    if c.family == "impulse":
        x = np.zeros(n, dtype=np.float32)
        x[n // 2 + 37] = 1.0
        return x
    x = speech(n)
    if c.family == "x1e-3":
        return (x * np.float32(1e-3)).astype(np.float32)
    if c.family == "x32768":
        return (x * np.float32(32768.0)).astype(np.float32)                       # the mistake of passing int16-scale floats
    if c.family == "gap":
        x = x.copy()
        x[n // 3:2 * n // 3] = 0.0
        return x
    assert c.family == "speech", c.family
    return x


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------------------

def _coef64(sd):
    return np.asarray(sd["coef"], dtype=np.float64).reshape(-1, 1)


def linear_mel(hook, sd):
    """exp(coef * hook) in float64: the clipped linear mel the hook (log-mel / coef) stands for."""
    return np.exp(_coef64(sd) * np.asarray(hook, dtype=np.float64))


def oracle(sd, wav, dtype, form="fft"):
    """(hook = log-mel / coef [100][F], features [1024][T]) of the oracle in `dtype`, as float64 numpy arrays."""
    mel = ref_cpu.mel_features(torch.from_numpy(np.asarray(wav)), dtype=dtype, form=form)
    hook = mel / ref_cpu._t(sd["coef"]).to(dtype).view(-1, 1)
    feat = ref_cpu.dvae_encoder_features(sd, mel, dtype=dtype)
    return hook.double().numpy(), feat.double().numpy()


def _worst(got, ref64, axis_len):
    return float(np.max(per_frame_err(got, ref64, axis_len)))


def yardstick(got32, ref64, axis_len):
    return max(_worst(got32, ref64, axis_len), YARD_FLOOR)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """Computed once per process and shared (read-only): ref64 of the three quantities and the float32 "dft"-form oracle's worst frame against each."""
    c = BY_ID[case_id]
    sd = encoder_sd(c.variant)
    wav = case_input(c)
    hook64, feat64 = oracle(sd, wav, torch.float64)
    hook32, feat32 = oracle(sd, wav, torch.float32, form="dft")
    lin64 = linear_mel(hook64, sd)
    for a in (hook64, feat64, lin64):
        a.setflags(write=False)
    return dict(hook64=hook64, feat64=feat64, lin64=lin64, finite=bool(np.isfinite(hook64).all() and np.isfinite(feat64).all()),
                yard_logmel=yardstick(hook32, hook64, N_MELS), yard_linear=yardstick(linear_mel(hook32, sd), lin64, N_MELS),
                yard_feat=yardstick(feat32, feat64, ODIM))


def _project(feat, sd, g, G, dtype=torch.float64):
    """project_in of group g on features [T][1024] -> z [T][4]."""
    per = ODIM // G
    x = torch.as_tensor(np.asarray(feat)).to(dtype)
    return F.linear(x[:, g * per:(g + 1) * per], ref_cpu._t(sd[f"vq_layer.quantizer.rvqs.{g}.project_in.weight"]).to(dtype),
                    ref_cpu._t(sd[f"vq_layer.quantizer.rvqs.{g}.project_in.bias"]).to(dtype))


@functools.lru_cache(maxsize=None)
def quant_reference(case_id, quant="g2r2"):
    """From the oracle alone, on ref64's features rounded to float32: eps[r] = FACTOR x max |pre-round float32 - pre-round float64| at residual level r; the share
    of float64 digits whose margin to the nearest rounding boundary is below eps[r]; whether the float32 and float64 oracle codes agree."""
    c = BY_ID[case_id]
    G, R, pre_bound = QUANTS[quant]
    sd = encoder_sd(c.variant, quant)
    x = torch.from_numpy(np.ascontiguousarray(reference(case_id)["feat64"].T.astype(np.float32)))        # [T][1024]
    ids32, _, pre32 = ref_cpu.gfsq_quantize(x, sd, G=G, R=R, pre_bound=pre_bound, dtype=torch.float32, return_pre=True)
    ids64, _, pre64 = ref_cpu.gfsq_quantize(x, sd, G=G, R=R, pre_bound=pre_bound, dtype=torch.float64, return_pre=True)
    diff = (pre32.double() - pre64).abs().numpy()                                                         # [G][R][T][4]
    raw = [float(diff[:, r].max()) for r in range(R)]
    eps = [FACTOR * v for v in raw]
    p = pre64.numpy()
    margin = 0.5 - np.abs(p - np.round(p))                                                                # distance to the nearest half-integer
    near = sum(int((margin[:, r] < eps[r]).sum()) for r in range(R))
    return dict(eps=eps, f32_f64_pre_diff=raw, near_tie_share=near / margin.size, codes_equal=bool(torch.equal(ids32, ids64)))


def digit_check(feat, ids, sd, quant, eps):
    """Teacher-forced check of the kernel's ids [G*R][T] against GFSQ in float64 on the kernel's own features [T][1024].  The ids are decoded into digits
    q = (id // 5^j) % 5 - 2; at each residual level r the float64 pre-round value p = tanh(res / 4^-r) * 2.002 is computed from the residual the KERNEL's earlier
    digits leave (a legitimate near-tie flip at r does not cascade into r + 1), and the excess is |p - q| - 0.5 - eps[r].  Frames whose features are not finite are
    left out (the caller checks their ids).  -> dict(max_excess = the largest excess over all digits (<= 0 passes), in_range, digits, worst = where)."""
    G, R, pre_bound = QUANTS[quant]
    feat = np.asarray(feat)
    ids = np.asarray(ids).astype(np.int64)
    assert ids.shape == (G * R, feat.shape[0]) and feat.shape[1] == ODIM, (ids.shape, feat.shape)
    ok = np.isfinite(feat).all(axis=1)
    out = dict(max_excess=-np.inf, in_range=bool(((ids[:, ok] >= 0) & (ids[:, ok] < 625)).all()), digits=0, worst=None, max_abs_dev=0.0)
    if not ok.any() or not out["in_range"]:
        return out
    pow5 = 5 ** np.arange(4)
    for g in range(G):
        z = _project(feat[ok], sd, g, G).numpy()                                                          # [T'][4] float64
        res = np.tanh(z) * HALF_L if pre_bound else z
        for r in range(R):
            scale = 4.0 ** -r
            p = np.tanh(res / scale) * HALF_L
            q = (ids[g * R + r][ok][:, None] // pow5[None, :]) % 5 - 2
            dev = np.abs(p - q)
            exc = dev - 0.5 - eps[r]
            i = np.unravel_index(np.argmax(exc), exc.shape)
            if exc[i] > out["max_excess"]:
                out["max_excess"], out["worst"] = float(exc[i]), dict(g=g, r=r, t=int(np.flatnonzero(ok)[i[0]]), j=int(i[1]), p=float(p[i]), q=int(q[i]))
            out["max_abs_dev"] = max(out["max_abs_dev"], float(dev.max()))
            out["digits"] += q.size
            res = res - (q / 2.0) * scale
    return out


def nonfinite_mel_frames(n, at):
    """The mel frames whose 1024-sample window (centred, hop 256) covers sample `at`: 256 f - 512 <= at < 256 f + 512."""
    return [f for f in range(1 + n // HOP) if HOP * f - N_FFT // 2 <= at < HOP * f + N_FFT // 2]


def measure(c, ids, hook, feat, quant="g2r2"):
    """What the test asserts on and the tool records for one kernel result: (ids [G*R][T], hook [100][F], feat [T][1024]) as numpy arrays."""
    r, qr = reference(c.id), quant_reference(c.id, quant)
    sd = encoder_sd(c.variant, quant)
    hook, feat = np.asarray(hook), np.asarray(feat)
    m = dict(case=c.id, n=c.n, frames=c.frames, codes=c.codes, family=c.family, variant=c.variant, quant=quant, linear_only=c.linear_only)
    for name, got, ref64, axis in (("logmel", hook, r["hook64"], N_MELS), ("linear", linear_mel(hook, sd), r["lin64"], N_MELS), ("feat", feat.T, r["feat64"], ODIM)):
        worst = _worst(got, ref64, axis)
        m[f"{name}_kernel_worst_frame"], m[f"{name}_yardstick"], m[f"{name}_ratio"] = worst, r[f"yard_{name}"], worst / r[f"yard_{name}"]
    d = digit_check(feat, ids, sd, quant, qr["eps"])
    m.update(eps=qr["eps"], f32_f64_pre_diff=qr["f32_f64_pre_diff"], near_tie_share=qr["near_tie_share"], digit_max_excess=d["max_excess"],
             digit_max_abs_dev=d["max_abs_dev"], digits=d["digits"], ids_in_range=d["in_range"], digit_worst=d["worst"])
    return m


def fmt(m):
    return (f"{m['case']} [{m['quant']}] F={m['frames']} T={m['codes']}: ratio to the float32 oracle's worst frame (bound {FACTOR:g}): "
            f"log-mel {m['logmel_ratio']:.2f} ({m['logmel_kernel_worst_frame']:.2e} / {m['logmel_yardstick']:.2e}), "
            f"linear mel {m['linear_ratio']:.2f} ({m['linear_kernel_worst_frame']:.2e} / {m['linear_yardstick']:.2e}), "
            f"features {m['feat_ratio']:.2f} ({m['feat_kernel_worst_frame']:.2e} / {m['feat_yardstick']:.2e}); "
            f"digits: max |p - q| {m['digit_max_abs_dev']:.6f}, excess over 0.5 + eps {m['digit_max_excess']:.2e}, eps {['%.1e' % e for e in m['eps']]}, "
            f"near ties {100 * m['near_tie_share']:.3f} %")


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------------------

def open_encoder(variant="plain", quant="g2r2", max_seconds=1.5):
    """A loaded native encoder for a checkpoint variant and a quantiser shape."""
    from chatttsplus_amd.hip_models import DVAEEncoder
    G, R, pre_bound = QUANTS[quant]
    e = DVAEEncoder(dim=512, vq_config=dict(dim=ODIM, levels=(5, 5, 5, 5), G=G, R=R), max_seconds=max_seconds, pre_bound=pre_bound)
    try:
        return e.load_state_dict(encoder_sd(variant, quant))
    except Exception:
        close_encoder(e)
        raise


def close_encoder(e):
    e.__del__()                  # frees the native handle now (idempotent)


def run_kernel(wav, e):
    """One clip through the single-clip entry point with the debug hooks -> (ids, hook, feat) numpy."""
    return tuple(t.cpu().numpy() for t in e.encode(torch.from_numpy(np.asarray(wav)), return_debug=True))
