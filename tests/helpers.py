"""Shared helpers for the parity tests (test infrastructure)."""
import os

import numpy as np

from chatttsplus_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = {k[5:]: z[k] for k in z.files if k.startswith("meta_")}
    return z, meta


def per_frame_err(got, ref64, axis_len):
    """Per-frame error of a vocoder output against its float64 reference, relative to the rms of the WHOLE reference.
    A mel [axis_len = 100][F]: per frame f the rms over the channels of got - ref64.  A waveform [S]: the same per segment of axis_len (= hop = 256)
    consecutive samples.  Dividing by the global rms (not the frame's own) keeps a silent frame from blowing the ratio up, and taking the maximum over
    the result lets no frame's absolute error hide in an average.  A NaN anywhere in `got` gives a NaN entry (np.max then returns NaN)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    if d.ndim == 2:
        assert d.shape[0] == axis_len, (d.shape, axis_len)
        e = np.sqrt(np.mean(np.square(d), axis=0))
    else:
        assert d.ndim == 1 and d.size and d.size % axis_len == 0, (d.shape, axis_len)
        e = np.sqrt(np.mean(np.square(d.reshape(-1, axis_len)), axis=1))
    return e / np.sqrt(np.mean(np.square(ref)))


def gen_case_inputs(meta, cfg):
    """Regenerates weights / prompt / speaker of a generate() golden from its stored seeds."""
    sd = synth.gpt_state_dict(cfg, int(meta["weight_seed"]))
    if "eos_boost" in meta:
        for i in range(4):
            sd[f"head_code.{i}.parametrizations.weight.original0"][625] *= float(meta["eos_boost"])
    B, T = int(meta["B"]), int(meta["T"])
    pad = [int(x) for x in np.atleast_1d(meta["pad_left"])]
    ids, mask = synth.prompt_ids(B, T, cfg["num_text_tokens"], int(meta["prompt_seed"]), pad_left=pad)
    spk = None
    if "spk_pos" in meta and int(meta["spk_pos"]) >= 0:
        ids[:, int(meta["spk_pos"]), :] = int(meta["spk_id"])
        spk = synth.speaker_vector(int(meta["spk_seed"]))
    return sd, ids, mask, spk
