"""Per-utterance sampling knobs (ctts_row_sampling, include/ctts_hip.h; GPT sampling_per_row; ChatTTSPlusPipeline params_per_utterance).

The sampler reads temperature, top-p, top-k, min_tokens_to_keep, the repetition penalty and min_new_token per decode row.  Checked here: the
stand-alone per-sequence sampler against the oracle run per sequence (bit-exact ids); under batch_invariant an utterance's ids and hidden rows equal
those of its batch-1 run with the same knobs as plain scalars, whatever the batch, the service order, admissions and compaction; on the default
engine a mixed batch equals, row for row, same-layout batches of uniform knobs; callers who do not use the feature get bit-identical results; bad
entries are errors; the pipeline hands every utterance its own knobs, prompt included.  Synthetic weights at real widths, 4 decoder layers."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth
from chatttsplus_amd.pipeline import gen_logits
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

CFG4 = dict(synth.GPT_REAL, num_hidden_layers=4)
LLAMA4 = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=4)
INV = {"batch_invariant": 1}
T_MAX, NEW_MAX, SEED = 40, 32, 777
_engines = {}


def engine(max_batch=16, options=None, dtype="fp32", fresh=False):
    from chatttsplus_amd.hip_models import GPT
    key = (max_batch, tuple(sorted((options or {}).items())), dtype)
    if fresh or key not in _engines:
        g = GPT(LLAMA4, max_batch=max_batch, max_seq_len=T_MAX + NEW_MAX + 8, weight_dtype=dtype, options=dict(options or {}))
        g.load_state_dict(synth.gpt_state_dict(CFG4, 4321))
        if fresh:
            return g
        _engines[key] = g
    return _engines[key]


# ---- 1. the stand-alone per-sequence sampler against the oracle -------------------------------------------------------------------------
def _knob(temp, top_p, top_k, rep, min_new, past_window=16, min_keep=3):
    r = _lib.RowSampling()
    t = list(temp) if isinstance(temp, (list, tuple)) else [temp] * 4
    for i in range(4):
        r.temperature[i] = float(np.float32(t[i]))
    r.top_p_threshold = float(np.float32(1 - top_p)) if top_p is not None else -1.0
    r.top_k = max(int(top_k), min_keep) if top_k else 0
    r.min_tokens_to_keep = min_keep
    r.use_penalty = 1 if rep != 1 else 0
    tab = torch.pow(float(rep), torch.arange(0, 17, dtype=torch.int64))
    for i in range(17):
        r.penalty_table[i] = float(tab[i])
    r.past_window, r.min_new_token = past_window, int(min_new)
    return r


def _scalar_cfg(k: _lib.RowSampling):
    sc = _lib.SamplerCfg()
    for i in range(4):
        sc.temperature[i] = k.temperature[i]
    sc.top_p_threshold, sc.top_k, sc.min_tokens_to_keep, sc.use_penalty = k.top_p_threshold, k.top_k, k.min_tokens_to_keep, k.use_penalty
    for i in range(17):
        sc.penalty_table[i] = k.penalty_table[i]
    sc.past_window, sc.max_input_ids, sc.eos_token, sc.min_new_token, sc.max_new_token = k.past_window, 625, 625, k.min_new_token, 4096
    return sc


def _run_rows(sc, knobs, logits, history, q, step):
    lib = _lib.load()
    rows, V = logits.shape
    dev = torch.device("cuda")
    lg, hs, qq = torch.from_numpy(logits).to(dev), torch.from_numpy(history.astype(np.int32)).to(dev).contiguous(), torch.from_numpy(q).to(dev)
    idx = torch.zeros(rows, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if knobs is None:
        _lib.check(lib.ctts_sampler_run(C.byref(sc), lg.data_ptr(), hs.data_ptr(), history.shape[1], qq.data_ptr(), rows, V, int(step), idx.data_ptr(), st), "sampler_run")
    else:
        arr = (_lib.RowSampling * len(knobs))(*knobs)
        _lib.check(lib.ctts_sampler_run_rows(C.byref(sc), arr, lg.data_ptr(), hs.data_ptr(), history.shape[1], qq.data_ptr(), rows, V, int(step),
                                             idx.data_ptr(), st), "sampler_run_rows")
    torch.cuda.synchronize()
    return idx.cpu().numpy()


SPECS = [  # (temperature, top_P, top_K (0 = disabled), penalty, min_new, case)
    (1e-4, 0.7, 20, 1.05, 0, "normal"), (0.3, None, 3, 1.3, 30, "normal"), (0.7, 0.95, 64, 1.0, 0, "normal"), (1.5, 0.3, 200, 1.05, 30, "normal"),
    ([0.2, 0.5, 0.9, 1.3], 0.95, 0, 1.3, 0, "normal"), (1.0, None, 0, 1.0, 30, "normal"), (0.7, 0.7, 20, 1.05, 0, "quantized"),
    (0.7, 0.7, 20, 1.05, 0, "all_equal"), (0.7, 0.7, 20, 1.05, 0, "two_levels"), (0.7, 0.7, 20, 1.05, 0, "few_valid_large"),
    (0.7, 0.98, 64, 1.05, 0, "normal"), (0.7, 0.7, 20, 1.05, 30, "neg_inf"), (0.3, 0.3, 3, 1.0, 0, "normal"), (1.2, None, None, 1.3, 0, "normal"),
]


def _rows_of(case, rng, scale=1.0):
    x = (rng.standard_normal((4, 626)) * scale).astype(np.float32)
    if case == "quantized":
        x = np.round(x * 2.0) / 2.0
    elif case == "all_equal":
        x[:] = 0.25
    elif case == "two_levels":
        x = np.where(rng.random((4, 626)) < 0.3, 1.0, -1.0).astype(np.float32)
    elif case == "few_valid_large":
        x[:] = -30.0
        for r in range(4):
            x[r, rng.integers(0, 626, size=1 + r)] = 2.0 + rng.standard_normal(1 + r).astype(np.float32)
    elif case == "neg_inf":
        x[:, ::3] = -np.inf
    return x


def test_sampler_rows_per_sequence_knobs_vs_oracle():
    rng = np.random.Generator(np.random.Philox(key=2024))
    specs = SPECS * 3                                              # 42 sequences, 168 rows
    logits = np.concatenate([_rows_of(s[5], rng, 0.5 + 0.5 * (i % 4)) for i, s in enumerate(specs)])
    rows = logits.shape[0]
    history = rng.integers(0, 626, size=(rows, 23), dtype=np.int64)
    history[:, -4:] = history[:, -5:-4]
    q = (-np.log1p(-rng.random((rows, 626)))).astype(np.float32).clip(min=1e-30)
    knobs = [_knob(t, p, k, r, m) for t, p, k, r, m, _ in specs]
    base = _scalar_cfg(_knob(0.3, 0.7, 20, 1.05, 0))
    idx = _run_rows(base, knobs, logits, history, q, 23)
    for s, (t, p, k, r, m, case) in enumerate(specs):
        tl = list(t) if isinstance(t, list) else [t] * 4
        sp = ref_cpu.SamplerParams(temperature=tl, top_p=p, top_k=(k if k else None), repetition_penalty=r, min_new_token=m, max_input_ids=625)
        sl = slice(4 * s, 4 * s + 4)
        ref = ref_cpu.sample_step(torch.from_numpy(logits[sl]), torch.from_numpy(history[sl]), torch.from_numpy(q[sl]), 23, sp,
                                  torch.tensor([[float(np.float32(v))] for v in tl], dtype=torch.float32),
                                  stable_sort=case in ("all_equal", "two_levels")).numpy()
        assert np.array_equal(idx[sl], ref.astype(np.int32)), f"sequence {s} {specs[s]}: {idx[sl]} vs {ref}"
    # every entry equal to the scalars: exactly ctts_sampler_run
    for spec in (SPECS[0], SPECS[3], SPECS[5]):
        k = _knob(*spec[:5])
        assert np.array_equal(_run_rows(_scalar_cfg(k), [k] * (rows // 4), logits, history, q, 23), _run_rows(_scalar_cfg(k), None, logits, history, q, 23))


# ---- helpers of the engine tests ---------------------------------------------------------------------------------------------------------
def _request(n, seed=99):
    rng = np.random.Generator(np.random.Philox(key=seed))
    lens = [int(x) for x in rng.integers(6, T_MAX + 1, size=n)]
    lims = [int(x) for x in rng.integers(8, NEW_MAX + 1, size=n)]
    ids, mask = synth.prompt_ids(n, T_MAX, CFG4["num_text_tokens"], seed=seed, pad_left=[T_MAX - x for x in lens])
    return lens, lims, ids, mask


def _knob_sets(n, min_new_too=True):
    rng = np.random.Generator(np.random.Philox(key=55))
    out = []
    for u in range(n):
        d = dict(temperature=[0.1, 0.3, 0.7, 1.2][u % 4] * (1.0 + 0.05 * (u // 4)), top_P=[0.7, None, 0.95, 0.3][(u // 2) % 4],
                 top_K=[20, 3, 64, None, 200][u % 5], repetition_penalty=[1.05, 1.0, 1.3][u % 3])
        if min_new_too:
            d["min_new_token"] = int(rng.integers(0, 6))
        out.append(d)
    return out


def _scalar_args(d, base_min_new):
    w, p = gen_logits(625, top_P=d.get("top_P", 0.7), top_K=d.get("top_K", 20), repetition_penalty=d.get("repetition_penalty", 1.05))
    return torch.tensor([float(d.get("temperature", 0.3))]), w, p, int(d.get("min_new_token", base_min_new))


def _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, min_new, per_row=None, max_new=NEW_MAX, trim=True):
    T = max(lens[u] for u in us) if trim else T_MAX
    ii = torch.as_tensor(us, dtype=torch.long)
    out = list(g.generate(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(ids[us][:, T_MAX - T:]), temp, 625,
                          attention_mask=torch.from_numpy(mask[us][:, T_MAX - T:]), max_new_token=max_new, min_new_token=min_new, logits_warpers=w,
                          logits_processors=p, return_hidden=True, noise="device", seed=SEED, utt_ids=list(us),
                          max_new_tokens_per_row=[lims[u] for u in us], sampling_per_row=per_row))[-1]
    return {u: (out.ids[j].cpu(), out.hiddens[j].cpu()) for j, u in enumerate(us)}


BASE = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05)


def _same(ref, got, what):
    for u, (i, h) in got.items():
        ri, rh = ref[u]
        assert torch.equal(i, ri), f"{what}: utterance {u} token ids differ"
        assert torch.equal(h, rh), f"{what}: utterance {u} hidden rows differ"


# ---- 2. batch_invariant: per-row knobs are the utterance's own inputs ---------------------------------------------------------------------
def test_invariant_engine_knobs_follow_the_utterance():
    g = engine(16, INV)
    N = 16
    lens, lims, ids, mask = _request(N)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    knobs = _knob_sets(N)
    ref = {}
    for u in range(N):
        temp, w, p, mn = _scalar_args(knobs[u], 1)
        ref.update(_gen(g, [u], emb, ids, mask, lens, lims, temp, w, p, mn))
    temp, w, p, mn = _scalar_args(BASE, 1)
    _same(ref, _gen(g, list(range(N)), emb, ids, mask, lens, lims, temp, w, p, mn, per_row=knobs), "one generate() with sampling_per_row")
    for rows in (4, 8):
        for sched in ("fifo", "longest_first"):
            g.schedule = sched
            try:
                out = g.generate_many(emb, torch.from_numpy(ids), temp, 625, attention_mask=torch.from_numpy(mask), max_new_token=NEW_MAX, min_new_token=mn,
                                      logits_warpers=w, logits_processors=p, return_hidden=True, seed=SEED, utt_ids=list(range(N)),
                                      max_new_tokens_per_row=lims, rows=rows, sampling_per_row=knobs)
            finally:
                g.schedule = "fifo"
            assert g.admissions, f"{rows} rows {sched}: no admission happened"
            _same(ref, {u: (out.ids[u].cpu(), out.hiddens[u].cpu()) for u in range(N)}, f"generate_many {rows} rows {sched}")


class _NoAdmitSampling:
    """the library with ctts_gpt_admit_sampling dropped: generate_many then seats its queued utterances without naming their knobs"""
    def __init__(self, lib):
        self._l = lib

    def __getattr__(self, name):
        return (lambda *a: 0) if name == "ctts_gpt_admit_sampling" else getattr(self._l, name)


def test_admitted_row_not_named_takes_the_call_values():
    """An admitted row that ctts_gpt_admit_sampling did not name samples with the call's knobs -- never with those of the finished utterance
    whose row it takes: the first 4 utterances (seated by begin) carry their own knobs, the 8 queued ones are admitted unnamed."""
    g = engine(16, INV)
    N, R = 12, 4
    lens, lims, ids, mask = _request(N, seed=21)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    own = [dict(temperature=1.4, top_P=None, top_K=None, repetition_penalty=1.3), dict(temperature=0.05, top_P=0.95, top_K=3, repetition_penalty=1.0),
           dict(temperature=1.1, top_P=0.3, top_K=64, repetition_penalty=1.05), dict(temperature=0.9, top_P=None, top_K=200, repetition_penalty=1.3)]
    knobs = own + [None] * (N - R)
    ref = {}
    for u in range(N):
        temp, w, p, mn = _scalar_args(knobs[u] or BASE, 1)
        ref.update(_gen(g, [u], emb, ids, mask, lens, lims, temp, w, p, mn))
    temp, w, p, mn = _scalar_args(BASE, 1)
    lib = g._lib
    g._lib = _NoAdmitSampling(lib)
    try:
        out = g.generate_many(emb, torch.from_numpy(ids), temp, 625, attention_mask=torch.from_numpy(mask), max_new_token=NEW_MAX, min_new_token=mn,
                              logits_warpers=w, logits_processors=p, return_hidden=True, seed=SEED, utt_ids=list(range(N)), max_new_tokens_per_row=lims,
                              rows=R, sampling_per_row=knobs)
    finally:
        g._lib = lib
    assert sum(k for _, k in g.admissions) >= N - R
    _same(ref, {u: (out.ids[u].cpu(), out.hiddens[u].cpu()) for u in range(N)}, "admitted without admit_sampling")


# ---- 3. default engine, fixed schedule: a mixed batch equals uniform batches row for row --------------------------------------------------
@pytest.mark.parametrize("B", [4, 12])
def test_default_engine_mixed_batch_equals_uniform_batches(B):
    g = engine(16)
    lens, lims, ids, mask = _request(B, seed=7 + B)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    knobs = _knob_sets(B, min_new_too=False)          # min_new_token = max_new_token for the call: rows end at their limits, the schedule is fixed
    us = list(range(B))
    temp, w, p, _ = _scalar_args(BASE, 0)
    mixed = _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, NEW_MAX, per_row=knobs, trim=False)
    for u in us:
        tu, wu, pu, _ = _scalar_args(knobs[u], 0)
        uni = _gen(g, us, emb, ids, mask, lens, lims, tu, wu, pu, NEW_MAX, trim=False)
        _same({u: uni[u]}, {u: mixed[u]}, f"B={B}, row {u} of the mixed batch vs a batch of its knobs")


# ---- 4. callers who do not use the feature -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B", [("fp32", 1), ("fp32", 5), ("fp32", 12), ("fp16", 1)])
def test_scalar_equal_entries_are_bit_identical(dtype, B):
    g = engine(16, dtype=dtype)
    lens, lims, ids, mask = _request(B, seed=3 + B)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    us = list(range(B))
    temp, w, p, mn = _scalar_args(BASE, 2)
    plain = _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn)
    same = [dict(BASE, min_new_token=2)] * B
    _same(plain, _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn, per_row=same), f"{dtype} B={B}: entries equal to the scalars")


def test_plain_call_after_a_per_row_call_matches_a_fresh_engine():
    g = engine(16)
    B = 5
    lens, lims, ids, mask = _request(B, seed=11)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    us = list(range(B))
    temp, w, p, mn = _scalar_args(BASE, 1)
    _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn, per_row=_knob_sets(B))
    after = _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn)
    f = engine(16, fresh=True)
    try:
        _same(_gen(f, us, emb, ids, mask, lens, lims, temp, w, p, mn), after, "plain call after a per-row call vs a fresh engine")
    finally:
        f.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------------
def test_bad_entries_are_errors_and_the_engine_recovers():
    g = engine(16)
    B = 3
    lens, lims, ids, mask = _request(B, seed=13)
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    us = list(range(B))
    temp, w, p, mn = _scalar_args(BASE, 1)
    plain = _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn)
    bad = [(dict(past_window=17), "past_window"), (dict(top_K=-1), "top_K"), (dict(temperature=0.0), "temperature")]
    for entry, word in bad:
        with pytest.raises(_lib.HipBackendError, match=word.replace("_K", "_[Kk]")):
            _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn, per_row=[None, entry, None])
        _same(plain, _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn), f"plain call after the {word} error")
    with pytest.raises(_lib.HipBackendError, match="entries"):
        _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn, per_row=[None, None])
    with pytest.raises(_lib.HipBackendError, match="code mode"):
        next(g.generate(emb[:1], torch.from_numpy(ids[:1]), torch.tensor([0.7]), 21177, max_new_token=4, logits_warpers=w, infer_text=True,
                        sampling_per_row=[None]))
    _same(plain, _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn), "plain call after the binding's errors")
    # the same entries straight through the C ABI: the engine's own begin refuses them with a message
    from chatttsplus_amd.hip_models.gpt import row_sampling_from_values, sampler_cfg_from_objects
    sc = sampler_cfg_from_objects(temp, 625, NEW_MAX, mn, w, p)
    raw = []
    for field, val in (("past_window", 17), ("top_k", -1), ("temperature", 0.0), ("min_tokens_to_keep", 0), ("min_new_token", NEW_MAX + 1)):
        r = row_sampling_from_values(sc)
        if field == "temperature":
            r.temperature[2] = val
        else:
            setattr(r, field, val)
        raw.append((field, r))
    mdev = torch.ones(1, 4, dtype=torch.int32, device="cuda")
    out = [torch.zeros(1, NEW_MAX, 4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
    io = _lib.GenIO(ids=out[0].data_ptr(), hiddens=None, finish=out[1].data_ptr(), end_idx=out[2].data_ptr(), noise=None, n_draws=NEW_MAX, seed=1)
    st = g._stream()
    lib = g._lib
    try:
        for field, r in raw:
            _lib.check(lib.ctts_gpt_set_row_sampling(g._h, (_lib.RowSampling * 1)(r), 1), "set_row_sampling")
            with pytest.raises(_lib.HipBackendError, match=field):
                _lib.check(lib.ctts_gpt_begin(g._h, 1, 4, mdev.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
        good = row_sampling_from_values(sc)
        _lib.check(lib.ctts_gpt_set_row_sampling(g._h, (_lib.RowSampling * 1)(good), 1), "set_row_sampling")
        tsc = sampler_cfg_from_objects(torch.tensor([0.7]), 21177, NEW_MAX, 0, w, [], infer_text=True)
        with pytest.raises(_lib.HipBackendError, match="code mode"):
            _lib.check(lib.ctts_gpt_begin(g._h, 1, 4, mdev.data_ptr(), C.byref(tsc), C.byref(io), st), "begin")
    finally:
        _lib.check(lib.ctts_gpt_set_row_sampling(g._h, None, 0), "set_row_sampling")
    torch.cuda.synchronize()
    _same(plain, _gen(g, us, emb, ids, mask, lens, lims, temp, w, p, mn), "plain call after the engine's errors")


# ---- 6. the pipeline: every utterance gets its own knobs (invariant engine, world 1) ------------------------------------------------------
def test_pipeline_params_per_utterance(tmp_path):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams
    g = GPT(LLAMA4, max_batch=4, max_seq_len=160, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(synth.gpt_state_dict(CFG4, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * 48 + 64, device="cuda:0", max_batch=8)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    pipe = ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(str(tmp_path / "tok")), torch.device("cuda:0"))
    texts = synth.toy_texts(6, 8, 40, seed=66)
    spk = torch.from_numpy(synth.speaker_vector(1234)).float()
    sets = [InferCodeParams(prompt="[speed_5]", temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, max_new_token=48, min_new_token=4, show_tqdm=False),
            InferCodeParams(prompt="", temperature=0.9, top_P=None, top_K=64, repetition_penalty=1.3, max_new_token=48, min_new_token=12, show_tqdm=False),
            InferCodeParams(prompt="[uv_break]", temperature=0.1, top_P=0.95, top_K=None, repetition_penalty=1.0, max_new_token=48, min_new_token=0, show_tqdm=False)]
    for k in sets:
        k.spk_emb = spk
    P = [sets[u % 3] for u in range(6)]

    def run(params, per_utt=None):
        ids = []
        mine, wavs, _ = pipe.infer_sharded(list(texts), params_infer_code=params, noise_seed=4242, slice_size=4, continuous=True, ids_out=ids,
                                           **({"params_per_utterance": per_utt} if per_utt is not None else {}))
        assert mine == list(range(6))
        return [i.cpu() for i in ids], [w.cpu() for w in wavs]

    try:
        ref = [run(k) for k in sets]
        ids, wavs = run(sets[0], P)
        for u in range(6):
            ri, rw = ref[u % 3][0][u], ref[u % 3][1][u]
            assert torch.equal(ids[u], ri), f"utterance {u}: token ids differ from the run with its own knob set"
            a, b = wavs[u].numpy(), rw.numpy()
            assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-4, f"utterance {u}: waveform"
    finally:
        g.close()
