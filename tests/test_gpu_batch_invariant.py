"""The batch-invariant mode of the fp32 engine (option "batch_invariant", include/ctts_hip.h).

With the option on and device noise, an utterance's hidden rows and token ids are a function of its own inputs only: served alone, in
slices of 2 .. 32 next to other prompts (other left padding), through finished-row compaction, seated by ctts_gpt_begin or by
ctts_gpt_admit, in arrival or longest-first order, on one rank or two -- bit for bit (torch.equal), not merely token for token.
Real widths (synth.GPT_REAL, synthetic weights)."""
import os
import socket

import numpy as np
import pytest
import torch

from chatttsplus_amd import synth
from tests.helpers import gen_case_inputs, load_golden

pytestmark = pytest.mark.gpu

LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
INV = {"batch_invariant": 1}

N_UTT, T_MAX, NEW_MAX, SEED = 40, 96, 96, 31337
_engines = {}


def engine(max_batch=32, max_seq=T_MAX + NEW_MAX + 8, boost=None, options=INV, seed=1234):
    from chatttsplus_amd.hip_models import GPT
    key = (max_batch, max_seq, boost, tuple(sorted(options.items())), seed)
    if key not in _engines:
        sd = synth.gpt_state_dict(synth.GPT_REAL, seed)
        if boost is not None:
            for i in range(4):
                sd[f"head_code.{i}.parametrizations.weight.original0"][625] *= float(boost)
        g = GPT(LLAMA, max_batch=max_batch, max_seq_len=max_seq, weight_dtype="fp32", options=dict(options))
        g.load_state_dict(sd)
        _engines[key] = g
    return _engines[key]


def _request():
    """N_UTT utterances: prompts U{8..96} tokens, limits U{16..96}; left-padded to T_MAX"""
    rng = np.random.Generator(np.random.Philox(key=4711))
    lens = [int(x) for x in rng.integers(8, T_MAX + 1, size=N_UTT)]
    lims = [int(x) for x in rng.integers(16, NEW_MAX + 1, size=N_UTT)]
    ids, mask = synth.prompt_ids(N_UTT, T_MAX, synth.GPT_REAL["num_text_tokens"], seed=99, pad_left=[T_MAX - n for n in lens])
    return lens, lims, ids, mask


_ref = {}


def _emb(g):
    lens, lims, ids, mask = _request()
    return lens, lims, ids, mask, g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))


def _generate(g, us, emb, ids, mask, lens, lims, trim=True):
    """the utterances `us` as ONE generate() call (left padding: to the longest of them, or the full T_MAX)"""
    T = max(lens[u] for u in us) if trim else T_MAX
    ii = torch.as_tensor(us, dtype=torch.long)
    out = list(g.generate(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(ids[us][:, T_MAX - T:]), torch.tensor([0.3] * 4), 625,
                          attention_mask=torch.from_numpy(mask[us][:, T_MAX - T:]), max_new_token=NEW_MAX, min_new_token=1, logits_warpers=LW,
                          logits_processors=LP, return_hidden=True, noise="device", seed=SEED, utt_ids=list(us), max_new_tokens_per_row=[lims[u] for u in us]))[-1]
    return {u: (out.ids[j].cpu(), out.hiddens[j].cpu()) for j, u in enumerate(us)}


def batch1_reference():
    """every utterance served alone (batch 1): the yardstick of the tests below"""
    if "b1" not in _ref:
        g = engine()
        lens, lims, ids, mask, emb = _emb(g)
        res = {}
        for u in range(N_UTT):
            res.update(_generate(g, [u], emb, ids, mask, lens, lims))
        _ref["b1"] = res
    return _ref["b1"]


def _same(ref, got, what):
    for u, (i, h) in got.items():
        ri, rh = ref[u]
        assert torch.equal(i, ri), f"{what}: utterance {u} token ids differ from its batch-1 run"
        assert torch.equal(h, rh), f"{what}: utterance {u} hidden rows differ from its batch-1 run (max {float((h - rh).abs().max()) if h.shape == rh.shape else h.shape})"


def test_option_surface():
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models import GPT
    g = engine()
    assert g.get_option("batch_invariant") == 1
    # effective values of the choices the option pins (the stored tuning values stay for when it is switched off)
    assert g.get_option("persistent_rows") == 0 and g.get_option("valu_rows") == 0 and g.get_option("split_decode_rows") == 1
    assert g.get_option("decode_splits") == 1 and g.get_option("prefill_splitk_rows") == 0 and g.get_option("split_rows") == 0
    g.set_option("batch_invariant", 0)
    try:
        assert g.get_option("batch_invariant") == 0
        assert g.get_option("split_decode_rows") == 9 and g.get_option("prefill_splitk_rows") == 2048
    finally:
        g.set_option("batch_invariant", 1)
    assert g.get_option("batch_invariant") == 1
    # default 0; set / get round trip on a plain engine (before finalize)
    d = GPT(LLAMA, max_batch=2, max_seq_len=64, weight_dtype="fp32")
    assert d.get_option("batch_invariant") == 0
    d.set_option("batch_invariant", 1)
    assert d.get_option("batch_invariant") == 1
    d.close()
    # fp16 engines: an error
    with pytest.raises(_lib.HipBackendError, match="batch_invariant"):
        GPT(LLAMA, max_batch=2, max_seq_len=64, weight_dtype="fp16", options=INV)
    # per-utterance adapters: refused by the binding and by the engine itself
    with pytest.raises(_lib.HipBackendError, match="batch_invariant"):
        g.set_row_adapters([0, -1])
    import ctypes as C
    arr = np.ascontiguousarray([0, -1], dtype=np.int32)
    _lib.check(g._lib.ctts_gpt_set_row_adapters(g._h, arr.ctypes.data_as(C.c_void_p), 2), "set_row_adapters")
    try:
        lens, lims, ids, mask, emb = _emb(g)
        with pytest.raises(_lib.HipBackendError, match="batch_invariant"):
            _generate(g, [0, 1], emb, ids, mask, lens, lims)
    finally:
        g.set_row_adapters(None)
    _generate(g, [0, 1], emb, ids, mask, lens, lims)          # the engine serves again


def test_row_count_and_padding_invariance():
    """slices of 1 / 2 / 4 / 8 / 9 / 16 / 17 / 32 utterances (compaction crosses 9 -> 8 and 17 -> 16 inside the larger ones), and an utterance
    padded to the full 96 tokens next to the longest prompts: hidden rows and ids equal the batch-1 run bit for bit"""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    for size in (2, 4, 8, 9, 16, 17, 32):
        got = {}
        for s0 in range(0, N_UTT, size):
            got.update(_generate(g, list(range(s0, min(s0 + size, N_UTT))), emb, ids, mask, lens, lims))
        _same(ref, got, f"slices of {size}")
    shortest = min(range(N_UTT), key=lambda u: lens[u])
    longest = sorted(range(N_UTT), key=lambda u: -lens[u])[:5]
    _same(ref, _generate(g, [shortest] + longest, emb, ids, mask, lens, lims, trim=False), "short prompt beside the longest ones")
    assert lens[shortest] < 20 and max(lens) > 80


@pytest.mark.parametrize("rows", [8, 32])
@pytest.mark.parametrize("schedule", ["fifo", "longest_first"])
def test_continuous_batching_and_compaction_invariance(rows, schedule):
    """generate_many (begin + admissions mid-run + compaction) equals the batch-1 runs bit for bit, per utterance -- also in the longest-first
    order, whose outputs must land at their utterance's index"""
    ref = batch1_reference()
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    g.schedule = schedule
    try:
        out = g.generate_many(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=NEW_MAX,
                              min_new_token=1, logits_warpers=LW, logits_processors=LP, return_hidden=True, seed=SEED, utt_ids=list(range(N_UTT)),
                              max_new_tokens_per_row=lims, rows=rows)
    finally:
        g.schedule = "fifo"
    assert g.admissions
    _same(ref, {u: (out.ids[u].cpu(), out.hiddens[u].cpu()) for u in range(N_UTT)}, f"generate_many on {rows} rows, {schedule}")


@pytest.mark.parametrize("name", ["gpt_real_b1", "gpt_real_b2_pad", "gpt_real_b4_ragged", "gpt_real_b32_ragged"])
def test_reference_goldens_hold_under_the_option(name):
    z, meta = load_golden(name)
    sd, ids, mask, spk = gen_case_inputs(meta, synth.GPT_REAL)
    boost = float(meta["eos_boost"]) if "eos_boost" in meta else None
    g = engine(max_batch=32, max_seq=840 if boost is None else 128, boost=boost, seed=int(meta["weight_seed"]))
    ids_t = torch.from_numpy(ids)
    emb = g(ids_t, torch.ones(ids.shape[:2], dtype=torch.bool))
    if spk is not None:
        from oracle import ref_cpu
        emb = ref_cpu.OracleGPT.apply_spk_emb(emb.cpu(), torch.from_numpy(spk), ids_t, int(meta["spk_id"])).cuda()
    np.testing.assert_allclose(emb[:, -1].cpu().numpy(), z["emb_last"], atol=0, rtol=0)
    torch.manual_seed(int(meta["torch_seed"]))
    out = list(g.generate(emb, ids_t, torch.tensor([float(meta["temperature"]) if "temperature" in meta else 0.3] * 4), 625,
                          attention_mask=torch.from_numpy(mask), max_new_token=int(meta["max_new"]), min_new_token=int(meta["min_new"]),
                          logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="torch"))[-1]
    lens = z["lens"]
    assert [int(i.shape[0]) for i in out.ids] == lens.tolist()
    for b, n in enumerate(lens):
        assert np.array_equal(out.ids[b].cpu().numpy(), z["ids"][b, :n].astype(np.int64)), f"row {b}: token ids differ"
    rows = [int(x) for x in meta["hidden_rows"]] if "hidden_rows" in meta else list(range(len(lens)))
    for k, r in enumerate(rows):
        n = int(lens[r])
        ref = z["hiddens"][k if "hidden_rows" in meta else r, :n]
        assert np.abs(out.hiddens[r].cpu().numpy() - ref).max() <= 1e-4, r


def test_device_noise_golden_under_the_option():
    z, meta = load_golden("gpt_real_device_noise")
    sd, ids, mask, _ = gen_case_inputs(meta, synth.GPT_REAL)
    seed, uids, N = int(meta["noise_seed"]), [int(u) for u in meta["utt_ids"]], int(meta["max_new"])
    g = engine(max_batch=16, max_seq=128, boost=float(meta["eos_boost"]) if "eos_boost" in meta else None, seed=int(meta["weight_seed"]))
    emb = g(torch.from_numpy(ids), torch.ones(ids.shape[:2], dtype=torch.bool))
    kw = dict(max_new_token=N, min_new_token=int(meta["min_new"]), logits_warpers=LW, logits_processors=LP, return_hidden=True)

    def check(out_ids, out_h, what):
        assert [int(i.shape[0]) for i in out_ids] == z["lens"].tolist(), what
        for b, n in enumerate(z["lens"]):
            assert np.array_equal(out_ids[b].cpu().numpy(), z["ids"][b, :n].astype(np.int64)), (what, b)
        for k, r in enumerate(int(x) for x in meta["hidden_rows"]):
            n = int(z["lens"][r])
            assert float(np.abs(out_h[r].cpu().numpy() - z["hiddens"][k, :n]).max()) <= 1e-4, (what, r)

    oi, oh = [], []
    for s0 in range(0, len(uids), 4):
        sl = slice(s0, s0 + 4)
        out = list(g.generate(emb[sl].contiguous(), torch.from_numpy(ids[sl]), torch.tensor([0.3] * 4), 625, noise="device", seed=seed, utt_ids=uids[sl],
                              attention_mask=torch.from_numpy(mask[sl]), **kw))[-1]
        oi += out.ids
        oh += out.hiddens
    check(oi, oh, "slices of 4")
    out = g.generate_many(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, seed=seed, utt_ids=uids, rows=3, attention_mask=torch.from_numpy(mask), **kw)
    check(out.ids, out.hiddens, "continuous batching on 3 rows")


def test_refine_text_pass_invariance():
    """infer_text=True runs the same layer stack (exact-f32 text head, one 16-row chunk per launch): one batch of 4 against batch 1"""
    g = engine()
    lens, lims, ids, mask, emb = _emb(g)
    us = [0, 1, 2, 3]

    def run(sel):
        T = max(lens[u] for u in sel)
        ii = torch.as_tensor(sel, dtype=torch.long)
        out = list(g.generate(emb[ii.cuda()][:, T_MAX - T:].contiguous(), torch.from_numpy(ids[sel][:, T_MAX - T:]), torch.tensor([0.7]), 21177,
                              attention_mask=torch.from_numpy(mask[sel][:, T_MAX - T:]), max_new_token=24, min_new_token=1, logits_warpers=LW,
                              infer_text=True, return_hidden=True, noise="device", seed=SEED, utt_ids=sel))[-1]
        return {u: (out.ids[j].cpu(), out.hiddens[j].cpu()) for j, u in enumerate(sel)}

    ref = {}
    for u in us:
        ref.update(run([u]))
    _same(ref, run(us), "refine-text pass, batch of 4")


# -- the full-size request (BASELINE configs[3] per GPU): 256 ragged utterances through infer_sharded(continuous=True) --------------------------------
N_REQ, MAX_NEW_REQ = 256, 512


def _req_pipeline(td, rows):
    from chatttsplus_amd.hip_models import GPT, Synth
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    g = GPT(LLAMA, max_batch=rows, max_seq_len=128 + MAX_NEW_REQ, weight_dtype="fp32", options=dict(INV))
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    syn = Synth(dict(synth.DVAE_REAL), dict(synth.VOCOS_REAL), max_frames=2 * MAX_NEW_REQ + 64, device="cuda:0", max_batch=32)
    syn.load("dvae.", synth.dvae_state_dict(synth.DVAE_REAL, 1234))
    syn.load("vocos.", synth.vocos_state_dict(synth.VOCOS_REAL, 1234))
    return ChatTTSPlusPipeline.from_components(g, syn, synth.toy_tokenizer(td), torch.device("cuda:0"))


def _req_run(pipe, rank, rows, order):
    from chatttsplus_amd.pipeline import InferCodeParams
    texts = synth.toy_texts(N_REQ, 11, 91, seed=256)
    rng = np.random.Generator(np.random.Philox(key=2560))
    limits = [int(x) for x in rng.integers(128, MAX_NEW_REQ + 1, size=N_REQ)]
    table = torch.from_numpy(np.stack([synth.speaker_vector(1234 + i) for i in range(4)])) if rank == 0 else None
    params = InferCodeParams(prompt="[speed_5]", max_new_token=MAX_NEW_REQ, min_new_token=MAX_NEW_REQ, show_tqdm=False)
    pipe.throughput_order = order
    ids = []
    mine, wavs, lens = pipe.infer_sharded(list(texts), speaker_index=[i % 4 for i in range(N_REQ)], speaker_table=table, params_infer_code=params,
                                          noise_seed=4242, slice_size=rows, continuous=True, max_new_tokens_per_utterance=limits, ids_out=ids)
    return mine, [w.cpu() for w in wavs], lens, [i.cpu() for i in ids]


def test_full_request_rows_and_order_invariance(tmp_path):
    res = {}
    for rows in (32, 16, 8):
        pipe = _req_pipeline(str(tmp_path / f"tok{rows}"), rows)
        for order in ("longest_first", "input"):
            mine, wavs, lens, ids = _req_run(pipe, 0, rows, order)
            assert mine == list(range(N_REQ))
            res[(rows, order)] = (wavs, ids)
        pipe.models_dict["gpt"].close()
    w0, i0 = res[(32, "longest_first")]
    for key, (w, i) in res.items():
        for u in range(N_REQ):
            assert torch.equal(i[u], i0[u]), f"{key}: utterance {u} token ids differ from 32 rows longest-first"
            a, b = w[u].numpy(), w0[u].numpy()
            assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-4, (key, u)
    torch.save({u: i0[u] for u in range(N_REQ)}, str(tmp_path / "w1_ids.pt"))


def _w2_worker(rank, world, port, td, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pipe = _req_pipeline(os.path.join(td, f"tok{rank}"), 32)
        mine, _, lens, ids = _req_run(pipe, rank, 32, "longest_first")
        torch.save(dict(mine=mine, lens=lens, ids=ids), os.path.join(out_dir, f"r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_full_request_world2_equals_world1(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out_dir = str(tmp_path / "out")
    os.makedirs(out_dir)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_w2_worker, args=(r, 2, port, str(tmp_path), out_dir)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=400)
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    pipe = _req_pipeline(str(tmp_path / "tok_w1"), 32)
    mine1, _, lens1, ids1 = _req_run(pipe, 0, 32, "longest_first")
    pipe.models_dict["gpt"].close()
    seen = []
    for r in range(2):
        got = torch.load(os.path.join(out_dir, f"r{r}.pt"), weights_only=True)
        assert got["lens"] == lens1
        for j, u in enumerate(got["mine"]):
            assert torch.equal(got["ids"][j], ids1[u]), f"utterance {u} on rank {r}: token ids differ from world 1"
        seen += got["mine"]
    assert sorted(seen) == list(range(N_REQ))
