"""Per-utterance sampling knobs on the host side (no GPU): the per-row conversion against the per-call one, the ABI struct, the validation
messages of the binding and of the engine, and the pipeline plumbing of params_per_utterance with a stub engine (slices, continuous="throughput"
ordering, a world-2 gloo infer_sharded)."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import row_sampling_array, row_sampling_from_values, sampler_cfg_from_objects
from chatttsplus_amd.pipeline import InferCodeParams, gen_logits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["top_p_threshold", "top_k", "min_tokens_to_keep", "use_penalty", "past_window", "min_new_token"]


def _cfg(temp, top_P, top_K, rep, min_new):
    w, p = gen_logits(625, top_P=top_P, top_K=top_K, repetition_penalty=rep)
    return sampler_cfg_from_objects(torch.tensor(temp if isinstance(temp, list) else [temp]), 625, 2048, min_new, w, p, 4)


def _fields(x):
    return ([x.temperature[i] for i in range(4)], [getattr(x, f) for f in FIELDS], [x.penalty_table[i] for i in range(17)])


@pytest.mark.parametrize("temp,top_P,top_K,rep,min_new", [(0.3, 0.7, 20, 1.05, 0), (1e-4, None, 3, 1.3, 7), ([0.2, 0.4, 0.8, 1.6], 0.95, None, 1.0, 2),
                                                          (1.5, 0.3, 200, 1.1, 0), (0.7, None, None, None, 1), (0.9, 0.5, 1, 1.05, 3)])
def test_per_row_conversion_equals_the_call_conversion(temp, top_P, top_K, rep, min_new):
    base = _cfg(0.55, 0.6, 30, 1.2, 5)            # a different call: every field must come from the entry
    want = _cfg(temp, top_P, top_K, rep, min_new)
    got = row_sampling_from_values(base, dict(temperature=temp, top_P=top_P, top_K=top_K, repetition_penalty=rep, min_new_token=min_new))
    assert _fields(got) == _fields(want)
    # no entry / missing keys: the call's values
    assert _fields(row_sampling_from_values(want)) == _fields(want)
    assert _fields(row_sampling_from_values(want, dict(top_K=top_K))) == _fields(want)


def test_row_sampling_struct_matches_header():
    assert C.sizeof(_lib.RowSampling) == 4 * 4 + 4 + 3 * 4 + 17 * 4 + 3 * 4 == 112
    hdr = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} ctts_row_sampling;", hdr).group(1)
    names = re.findall(r"^\s*(?:float|int32_t)\s+(\w+)", body, re.M)
    assert names == [n for n, _ in _lib.RowSampling._fields_]


def test_binding_validation_messages():
    base = _cfg(0.3, 0.7, 20, 1.05, 0)
    with pytest.raises(_lib.HipBackendError, match=r"top_K = -1 < 0"):
        row_sampling_array(base, [dict(top_K=-1)], 1)
    with pytest.raises(_lib.HipBackendError, match=r"2 entries for 3 sequences"):
        row_sampling_array(base, [None, None], 3)
    with pytest.raises(_lib.HipBackendError, match=r"code mode only"):
        row_sampling_array(base, [None], 1, infer_text=True)
    with pytest.raises(_lib.HipBackendError, match=r"unknown key\(s\) \['top_p'\]"):
        row_sampling_array(base, [dict(top_p=0.5)], 1)
    with pytest.raises(_lib.HipBackendError, match=r"temperature has 3 values"):
        row_sampling_array(base, [dict(temperature=[0.1, 0.2, 0.3])], 1)


@pytest.mark.parametrize("field,value,msg", [("past_window", 17, r"past_window = 17 outside 1\.\.16"), ("past_window", 0, r"past_window = 0 outside"),
                                             ("top_k", -1, r"top_k = -1 < 0"), ("temperature", 0.0, r"temperature\[1\] = 0 \(must be finite and > 0\)"),
                                             ("temperature", float("nan"), r"temperature\[1\] = nan"), ("min_tokens_to_keep", 0, r"min_tokens_to_keep = 0 < 1"),
                                             ("min_new_token", 2049, r"min_new_token = 2049 > max_new_token = 2048")])
def test_engine_validation_messages(field, value, msg):
    """ctts_sampler_run_rows checks its entries before it touches the device: the engine's own messages, on any machine"""
    lib = _lib.load()
    sc = _cfg(0.3, 0.7, 20, 1.05, 0)
    sc.max_new_token = 2048
    entries = row_sampling_array(sc, [None, None], 2)
    if field == "temperature":
        entries[1].temperature[1] = value
    else:
        setattr(entries[1], field, value)
    if torch.cuda.is_available():
        # real (small) device buffers where a device exists: nothing here may hand the library an address it could touch
        lg, q, idx = torch.zeros(8, 626, device="cuda"), torch.ones(8, 626, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
        ptrs = (lg.data_ptr(), q.data_ptr(), idx.data_ptr())
    else:
        ptrs = (64, 64, 64)       # no device: the library cannot reach one; the entries are checked on the host first
    rc = lib.ctts_sampler_run_rows(C.byref(sc), entries, C.c_void_p(ptrs[0]), None, 0, C.c_void_p(ptrs[1]), 8, 626, 0, C.c_void_p(ptrs[2]), None)
    assert rc != 0
    err = lib.ctts_last_error().decode()
    assert re.search(r"sampler_run_rows: entry 1: " + msg, err), err


# ---- the pipeline with a stub engine -------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[Stts]", "[Ptts]", "[spk_emb]", "[empty_spk]", "[uv_break]", "[break_0]",
         "[Ebreak]", "[speed_5]", "a", "b", "c", "d"]


class _RecGPT:
    """hip_models.GPT stand-in: records, per global utterance id, the sampling entry, the token limit, the prompt length and the speaker row it
    was handed -- a knob that reaches the wrong utterance shows up as a wrong record."""
    num_vq, model_dim, max_batch = 4, 8, 3

    def __init__(self):
        self.emb_code = [type("E", (), dict(num_embeddings=626))() for _ in range(4)]
        self.seen = {}

    def __call__(self, input_ids, text_mask, spk_emb=None, spk_emb_ids=None):
        B, T = input_ids.shape[:2]
        emb = torch.zeros(B, T, self.model_dim)
        if spk_emb is not None:
            emb[:, 0, 1] = torch.as_tensor(spk_emb, dtype=torch.float32).reshape(-1, self.model_dim).expand(B, -1)[:, 0]
        return emb

    def _record(self, emb, attention_mask, max_new_token, kw):
        B = emb.shape[0]
        per = kw.get("sampling_per_row") or [None] * B
        lim = kw.get("max_new_tokens_per_row") or [max_new_token] * B
        assert len(per) == B and len(lim) == B and len(kw["utt_ids"]) == B
        for b, u in enumerate(kw["utt_ids"]):
            self.seen[int(u)] = (per[b], int(lim[b]), int(attention_mask[b].sum()), float(emb[b, 0, 1]), int(max_new_token))
        return [3 + b for b in range(B)]

    def generate(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, max_new_token=2048, return_hidden=False, **kw):
        n = self._record(emb, attention_mask, max_new_token, kw)
        yield type("O", (), dict(ids=[torch.zeros(k, 4, dtype=torch.long) for k in n], attentions=[], hiddens=[torch.full((k, 768), 1.0) for k in n]))

    def generate_many_iter(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, max_new_token=2048, return_hidden=False, **kw):
        n = self._record(emb, attention_mask, max_new_token, kw)
        ids = [torch.zeros(k, 4, dtype=torch.long) for k in n]
        hid = [torch.full((k, 768), 1.0) for k in n]
        yield [(b, ids[b], hid[b] if return_hidden else None) for b in range(len(n))]
        return type("O", (), dict(ids=ids, attentions=[], hiddens=hid))


class _FakeSynth:
    def decode_batch(self, hiddens):
        return [torch.full((256 * (2 * h.shape[0] - 1),), float(h.shape[0])) for h in hiddens]


def _pipe(tmpdir):
    from transformers import BertTokenizerFast
    from chatttsplus_amd.pipeline import ChatTTSPlusPipeline
    from chatttsplus_amd.tokenizer import Tokenizer
    vf = os.path.join(tmpdir, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(VOCAB))
    bt = BertTokenizerFast(vocab_file=vf, do_lower_case=False)
    bt.add_special_tokens({"additional_special_tokens": [v for v in VOCAB if v.startswith("[") and v not in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")]})
    pipe = object.__new__(ChatTTSPlusPipeline)
    pipe.device = torch.device("cpu")
    pipe.normalizer = lambda t, *a, **k: t
    pipe.text_splitter = None
    pipe.models_dict = dict(gpt=_RecGPT(), tokenizer=Tokenizer(tokenizer=bt))
    pipe.synth = _FakeSynth()
    pipe._lora_models, pipe._lora_cache = {}, 1
    pipe.std = pipe.mean = None
    return pipe


TEXTS = ["a b c", "a b c d a b", "a", "b c d a", "c c c c c c c", "d a", "a b"]
BASE = InferCodeParams(prompt="", max_new_token=64, show_tqdm=False, spk_emb=torch.ones(8))


def _entries():
    return [None, dict(temperature=0.9, top_K=64), InferCodeParams(prompt="[speed_5]", temperature=0.1, top_P=None, max_new_token=40, show_tqdm=False),
            dict(repetition_penalty=1.3, min_new_token=5, max_new_token=50), dict(prompt="[speed_5]"), dict(spk_emb=torch.full((8,), 5.0), top_P=0.3),
            dict(temperature=[0.1, 0.2, 0.3, 0.4])]


def _check(seen, base_len, utts):
    for u in utts:
        e = _entries()[u]
        vals = {} if e is None else ({k: getattr(e, k) for k in ("temperature", "top_P", "top_K", "repetition_penalty", "min_new_token", "max_new_token", "prompt")}
                                     if isinstance(e, InferCodeParams) else dict(e))
        want = {k: v for k, v in vals.items() if k in ("temperature", "top_P", "top_K", "repetition_penalty", "min_new_token") and v != getattr(BASE, k)}
        per, lim, plen, spk0, max_new = seen[u]
        assert (per or {}) == want, (u, per, want)
        assert lim == vals.get("max_new_token", 64) and max_new == 64, (u, lim, max_new)
        assert plen == base_len[u] + (1 if vals.get("prompt") == "[speed_5]" else 0), (u, plen, base_len[u])
        assert spk0 == (5.0 if u == 5 else 1.0), (u, spk0)


def _base_lengths(tmpdir, **kw):
    pipe = _pipe(tmpdir)
    for _ in pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", noise_seed=1, **kw):
        pass
    return {u: v[2] for u, v in pipe.models_dict["gpt"].seen.items()}


@pytest.mark.parametrize("mode", ["slices", "throughput"])
def test_pipeline_params_per_utterance_reach_their_rows(tmp_path, mode):
    kw = dict(slice_size=3) if mode == "slices" else dict(slice_size=3, continuous="throughput")
    base_len = _base_lengths(str(tmp_path), **kw)
    pipe = _pipe(str(tmp_path))
    for _ in pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", noise_seed=1, params_per_utterance=_entries(), **kw):
        pass
    _check(pipe.models_dict["gpt"].seen, base_len, range(len(TEXTS)))


def test_pipeline_params_per_utterance_errors(tmp_path):
    pipe = _pipe(str(tmp_path))
    with pytest.raises(_lib.HipBackendError, match=r"params_per_utterance: 2 entries for 7 utterances \(after text splitting\)"):
        list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", params_per_utterance=[None, None]))
    with pytest.raises(_lib.HipBackendError, match=r"'stream_batch'"):
        list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", params_per_utterance=[dict(stream_batch=3)] + [None] * 6))
    with pytest.raises(_lib.HipBackendError, match=r"exclusive"):
        list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", params_per_utterance=_entries(), max_new_tokens_per_utterance=[8] * 7))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, td, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pipe = _pipe(os.path.join(td, f"r{rank}"))
        table = torch.ones(1, 8) if rank == 0 else None
        mine, _, _ = pipe.infer_sharded(list(TEXTS), speaker_index=[0] * len(TEXTS), speaker_table=table, params_infer_code=BASE, noise_seed=3,
                                        slice_size=2, params_per_utterance=_entries())
        q.put((rank, mine, pipe.models_dict["gpt"].seen))
    finally:
        dist.destroy_process_group()


def test_pipeline_params_per_utterance_world2_gloo(tmp_path):
    import torch.multiprocessing as mp
    os.makedirs(str(tmp_path / "r0")); os.makedirs(str(tmp_path / "r1")); os.makedirs(str(tmp_path / "b"))
    base_len = _base_lengths(str(tmp_path / "b"), slice_size=2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    seen_all = []
    for rank, mine, seen in res:
        assert sorted(seen) == sorted(mine) and mine
        _check(seen, base_len, mine)
        seen_all += mine
    assert sorted(seen_all) == list(range(len(TEXTS)))


# ---- entries are resolved against the params the CALLER passed, not against the speaker the pipeline fills in ------------------------------
def test_infer_sharded_entries_keep_their_speaker_index_row(tmp_path):
    """speaker_index over two table rows + InferCodeParams entries derived from the call's params (they carry its spk_emb): every utterance keeps
    its own table row; only an entry that really sets another spk_emb changes its speaker"""
    import dataclasses
    pipe = _pipe(str(tmp_path))
    table = torch.stack([torch.full((8,), 1.0), torch.full((8,), 2.0)])
    index = [u % 2 for u in range(len(TEXTS))]
    entries = [dataclasses.replace(BASE, temperature=0.5 + 0.1 * u) for u in range(len(TEXTS))]
    entries[5] = dict(spk_emb=torch.full((8,), 5.0), temperature=0.3)
    for continuous in (False, True):
        pipe.models_dict["gpt"].seen = {}
        mine, _, _ = pipe.infer_sharded(list(TEXTS), speaker_index=index, speaker_table=table, params_infer_code=BASE, noise_seed=3, slice_size=3,
                                        continuous=continuous, params_per_utterance=entries)
        seen = pipe.models_dict["gpt"].seen
        assert sorted(seen) == sorted(mine) == list(range(len(TEXTS)))
        for u in range(len(TEXTS)):
            want = 5.0 if u == 5 else float(index[u] + 1)
            assert seen[u][3] == want, (continuous, u, seen[u][3], want)
            assert seen[u][0] == ({"temperature": 0.5 + 0.1 * u} if u != 5 else None), (continuous, u, seen[u][0])


def test_infer_speaker_emb_path_with_derived_entries(tmp_path):
    """infer(speaker_emb_path=...) fills in the speaker after the caller's params were taken: entries derived from those params keep that speaker"""
    import dataclasses
    pipe = _pipe(str(tmp_path))
    path = str(tmp_path / "spk.pt")
    torch.save(torch.full((8,), 9.0), path)
    entries = [dataclasses.replace(BASE, temperature=0.9, top_K=64) for _ in TEXTS]
    for _ in pipe.infer(list(TEXTS), skip_refine_text=True, speaker_emb_path=path, params_infer_code=BASE, noise="device", noise_seed=1,
                        slice_size=3, params_per_utterance=entries):
        pass
    seen = pipe.models_dict["gpt"].seen
    assert sorted(seen) == list(range(len(TEXTS)))
    for u in range(len(TEXTS)):
        assert seen[u][3] == 9.0 and seen[u][0] == {"temperature": 0.9, "top_K": 64}, (u, seen[u])
