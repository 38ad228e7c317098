"""Characterisation of ChatTTSPlusPipeline._infer / infer_sharded on a fake engine (no GPU): which engine calls a request turns into, with which rows, in which
order -- and when the request seed is drawn from torch's CPU generator.  Every case runs the pipeline with torch.manual_seed(0) and compares the trace of
calls and yields with the one recorded in test_infer_request_host.json (python -m tests.test_infer_request_host rewrites that file: only to record a deliberate
change of behaviour).  The fake's generate() and _refine_text() consume one torch.rand(1) each when they run under torch noise, so the `seed` the later calls
receive pins both whether and when the seed was drawn."""
import dataclasses
import json
import os

import pytest
import torch

from chatttsplus_amd import pipeline as pl
from chatttsplus_amd.pipeline import ChatTTSPlusPipeline, InferCodeParams, InferDetails, RefineTextParams

GOLDEN = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
DIM = 8


def _plain(v):
    """tensors, tuples and objects -> plain lists and scalars"""
    if torch.is_tensor(v):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class _Tok:
    """character-level tokenizer: id = ord(char); the control ids sit above the characters as in the real vocabulary"""
    break_0_ids, eos_token, spk_emb_ids, len = 1000, 1001, 999, 1100

    def encode(self, text, num_vq, prompt_str=None, device="cpu"):
        T = max(len(t) for t in text)
        ids, att = torch.zeros(len(text), T, dtype=torch.long), torch.zeros(len(text), T, dtype=torch.long)
        for b, t in enumerate(text):
            ids[b, T - len(t):] = torch.tensor([ord(c) for c in t], dtype=torch.long)
            att[b, T - len(t):] = 1
        return ids.unsqueeze(-1).expand(-1, -1, num_vq).clone(), att, att.bool()

    def decode(self, ids_list):
        return ["".join(chr(int(i)) for i in ids) for ids in ids_list]


class _Out:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Engine:
    """hip_models.GPT stand-in that records every call into `trace`"""
    num_vq, model_dim, max_batch = 4, DIM, 3

    def __init__(self, trace):
        self.trace = trace
        self.emb_code = [_Out(num_embeddings=626) for _ in range(4)]
        self.staged = None

    def __call__(self, input_ids, text_mask, spk_emb=None, spk_emb_ids=None):
        B = input_ids.shape[0]
        texts = ["".join(chr(int(i)) for i, m in zip(input_ids[b, :, 0], text_mask[b]) if m) for b in range(B)]
        spk = None if spk_emb is None else torch.as_tensor(spk_emb, dtype=torch.float32).reshape(-1, DIM).expand(B, -1).sum(1).tolist()
        self.staged = (texts, spk)
        return torch.zeros(B, input_ids.shape[1], DIM)

    def _rows(self, name, emb, kw):
        texts, spk = self.staged
        if name == "generate" and kw.get("noise") is None:
            torch.rand(1)                                             # torch noise: the call draws from the CPU generator
        # (a keyword passed as None is recorded like one left out: None is the engine's default for every keyword the pipeline passes that way)
        self.trace.append([name, texts, {k: _plain(v) for k, v in sorted(kw.items()) if v is not None}, spk])
        B = len(kw["prompt_of"]) if kw.get("prompt_of") is not None else emb.shape[0]
        uids = [int(u) for u in (kw.get("utt_ids") or range(B))]
        lim = kw.get("max_new_tokens_per_row") or [kw["max_new_token"]] * B
        n = [min(int(lim[b]), 3 + (u & 0xFFFF) * 5 % 7) for b, u in enumerate(uids)]
        ids = [torch.full((k, 4), (u & 0xFFFF) + 100 * (u >> 48), dtype=torch.long) for k, u in zip(n, uids)]
        hid = [torch.full((k, DIM), 1.0) for k in n]
        lps = [torch.full((k, 4), -(1.0 + ((u & 0xFFFF) + 3 * (u >> 48)) % 4 / 4)) for k, u in zip(n, uids)]
        return n, _Out(ids=ids, attentions=[], hiddens=hid, logprobs=lps, sampled_logprobs=[l / 2 for l in lps], final_logprobs=[None] * B)

    def generate(self, emb, inputs_ids, **kw):
        n, out = self._rows("generate", emb, kw)
        if kw.get("stream"):
            for s in range(2, max(n), 2):
                yield _Out(ids=[i[:s] for i in out.ids], attentions=[], hiddens=[h[:s] for h in out.hiddens])
        yield out

    def generate_many_iter(self, emb, inputs_ids, **kw):
        n, out = self._rows("generate_many_iter", emb, kw)
        hid = out.hiddens if kw.get("return_hidden") else [None] * len(n)
        for s in range(1, max(n) + 1):
            if kw.get("progress") and s % 2 == 0:
                yield ("progress", [(k, s, out.ids[k][:s], None if hid[k] is None else hid[k][:s]) for k in range(len(n)) if n[k] > s])
            done = [(k, out.ids[k], hid[k]) for k in range(len(n)) if n[k] == s]
            if done:
                yield done
        return out

    def set_row_adapters(self, slots):
        self.trace.append(["set_row_adapters", _plain(slots)])

    def load_adapter(self, slot, adapters):
        self.trace.append(["load_adapter", slot, adapters])


class _Synth:
    def decode_batch(self, items):
        return [torch.full((256 * (2 * h.shape[0] - 1) if h.shape[0] else 0,), float(h.shape[0])) for h in items]

    def decode_window(self, items, s0, s1):
        return [torch.arange(a, max(a, min(b, 256 * (2 * h.shape[0] - 1) if h.shape[0] else 0)), dtype=torch.float32) for h, a, b in zip(items, s0, s1)]


def _make_pipe(monkeypatch):
    trace = []
    pipe = object.__new__(ChatTTSPlusPipeline)
    pipe.device = torch.device("cpu")
    pipe.normalizer = lambda t, *a, **k: t
    pipe.text_splitter = None
    pipe.models_dict = dict(gpt=_Engine(trace), tokenizer=_Tok())
    pipe.synth = pipe.synth_codes = _Synth()
    pipe._lora_models, pipe._lora_cache = {}, 1
    pipe.std = pipe.mean = None
    monkeypatch.setattr(pl, "load_lora_adapter", lambda path: f"adapter:{path}")

    def refine(text, params, continuous_rows=0, seed=None, utt_ids=None):
        if continuous_rows == 0:
            torch.rand(1)
        trace.append(["_refine_text", list(text), dict(continuous_rows=continuous_rows, seed=seed, utt_ids=_plain(utt_ids), prompt=params.prompt)])
        ids = []
        for t in text:                                                 # the refined text between control ids that the pipeline filters out
            r = t if t.endswith("[uv_break]") else t + "!"
            ids.append(torch.tensor([1002] + [ord(c) for c in r] + [1000, 1001], dtype=torch.long))
        return _Out(ids=ids)

    decode = pipe._decode_to_wavs

    def decode_to_wavs(items, use_decoder=True):
        trace.append(["_decode_to_wavs", [list(i.shape) for i in items], bool(use_decoder)])
        return decode(items, use_decoder)

    pipe._refine_text, pipe._decode_to_wavs = refine, decode_to_wavs
    return pipe, trace


def _summary(y):
    if isinstance(y, InferDetails):
        return dict(wavs=[int(w.shape[0]) for w in y.wavs], ids=[[int(i.shape[0]), int(i[0, 0])] for i in y.ids], mean_logprob=y.mean_logprob,
                    candidate=y.candidate, scores=_plain(y.candidate_scores), n_candidates=None if y.candidates is None else [len(c) for c in y.candidates])
    if torch.is_tensor(y):
        return dict(shape=list(y.shape), sum=float(y.double().sum()))
    if isinstance(y, (list, tuple)):
        return [_summary(x) for x in y]
    return y


TEXTS = ["a b c", "a b c d a b [uv_break]", "a", "b c d a", "c c c c c c c", "d a", "a b"]
BASE = InferCodeParams(prompt="[speed_5]", max_new_token=64, show_tqdm=False, spk_emb=torch.arange(float(DIM)), stream_batch=2, stream_speed=700, pass_first_n_batches=1)
LIMITS = [5, 9, 3, 7, 4, 8, 6]
TABLE = torch.arange(7.0 * DIM).reshape(7, DIM)
LORA = ["A", None, "B", "A", None, "B", "A"]
DEV = dict(skip_refine_text=True, noise="device", noise_seed=11)


def _entries():
    return [None, dict(temperature=0.9, top_K=64), dataclasses.replace(BASE, prompt="[oral_2]", temperature=0.1, top_P=None, max_new_token=40),
            dict(repetition_penalty=1.3, min_new_token=2, max_new_token=5), dict(prompt=""), dict(spk_emb=torch.full((DIM,), 5.0), top_P=0.3),
            dict(temperature=[0.1, 0.2, 0.3, 0.4])]


def _cases():
    cases = {}
    for path, kw in (("sliced", {}), ("continuous", dict(continuous=True)), ("throughput", dict(continuous="throughput"))):
        kw = dict(kw, slice_size=3)
        cases[f"{path}-base"] = dict(DEV, **kw, _ids_sink=True)
        cases[f"{path}-limits"] = dict(DEV, **kw, max_new_tokens_per_utterance=LIMITS)
        cases[f"{path}-per-utterance"] = dict(DEV, **kw, params_per_utterance=_entries())
        cases[f"{path}-per-utterance-limits-table"] = dict(DEV, **kw, params_per_utterance=[e if isinstance(e, dict) and "max_new_token" not in e else None for e in _entries()],
                                                          max_new_tokens_per_utterance=LIMITS, spk=TABLE)
        cases[f"{path}-table"] = dict(DEV, **kw, spk=TABLE)
        cases[f"{path}-table-one-text"] = dict(DEV, **kw, spk=TABLE[3:4], texts=TEXTS[:1])
        cases[f"{path}-lora"] = dict(DEV, **kw, lora_paths=LORA, _ids_sink=True)
        for noise in ("device", "auto"):
            cases[f"{path}-{noise}-seed"] = dict(kw, skip_refine_text=True, noise=noise, noise_seed=7)
            cases[f"{path}-{noise}-draw"] = dict(kw, skip_refine_text=True, noise=noise)
        cases[f"{path}-auto-draw-wide-refine"] = dict(kw, slice_size=5, noise="auto")
        cases[f"{path}-refine"] = dict(kw, noise="device")
        cases[f"{path}-refine-only"] = dict(kw, refine_text_only=True, return_details=True, num_candidates=2)
        cases[f"{path}-codes"] = dict(DEV, **kw, use_decoder=False)
    cases["sliced-stream"] = dict(DEV, slice_size=3, stream=True, lora_paths=LORA)
    cases["continuous-stream"] = dict(DEV, slice_size=3, stream=True, continuous=True, spk=TABLE)
    cases["throughput-stream-codes"] = dict(DEV, slice_size=3, stream=True, continuous="throughput", use_decoder=False, max_new_tokens_per_utterance=LIMITS)
    cases["throughput-input-order"] = dict(DEV, slice_size=3, continuous="throughput", throughput_order="input", max_new_tokens_per_utterance=LIMITS)
    for share in (True, False):
        cases[f"candidates-share-{share}"] = dict(DEV, slice_size=8, num_candidates=3, share_prompt=share, return_details=True, params_per_utterance=_entries(), _ids_sink=True)
    cases["candidates-plain-wavs"] = dict(skip_refine_text=True, slice_size=8, num_candidates=3)
    cases["candidates-table-lora"] = dict(DEV, slice_size=8, num_candidates=3, spk=TABLE, lora_paths=LORA, max_new_tokens_per_utterance=LIMITS)
    cases["candidates-table-lora-shared"] = dict(DEV, slice_size=8, num_candidates=3, spk=TABLE, lora_paths=LORA, share_prompt=True)
    cases["candidates-continuous"] = dict(DEV, slice_size=8, num_candidates=3, continuous=True, return_details=True, spk=TABLE, lora_paths=LORA, _ids_sink=True)
    cases["candidates-continuous-refine-draw"] = dict(slice_size=8, num_candidates=3, continuous=True, share_prompt=True)
    cases["details"] = dict(DEV, slice_size=3, return_details=True, _ids_sink=True)
    cases["details-auto-draw-refine"] = dict(slice_size=3, return_details=True, noise="auto")
    cases["details-auto-draw-wide-refine"] = dict(slice_size=5, return_details=True, noise="auto", spk=TABLE)
    cases["details-table-one-text"] = dict(DEV, slice_size=3, return_details=True, spk=TABLE[3:4], texts=TEXTS[:1])
    cases["details-continuous"] = dict(DEV, slice_size=3, return_details=True, continuous=True, spk=TABLE)
    cases["lora-closed-after-first-yield"] = dict(DEV, slice_size=3, lora_paths=LORA, close_after=1)
    cases["lora-stream-closed-after-first-yield"] = dict(DEV, slice_size=3, lora_paths=LORA, stream=True, close_after=1)
    cases["sharded"] = dict(sharded=True, slice_size=3, lora_paths=LORA, params_per_utterance=_entries()[:3] + [None] * 4)
    cases["sharded-continuous-draw"] = dict(sharded=True, slice_size=3, continuous=True, skip_refine_text=False, max_new_tokens_per_utterance=LIMITS)
    return cases


CASES = _cases()


def _run(name, monkeypatch):
    kw = dict(CASES[name])
    pipe, trace = _make_pipe(monkeypatch)
    texts = list(kw.pop("texts", TEXTS))
    params = dataclasses.replace(BASE, spk_emb=kw.pop("spk")) if "spk" in kw else BASE
    if "throughput_order" in kw:
        pipe.throughput_order = kw.pop("throughput_order")
    close_after = kw.pop("close_after", None)
    sink = [] if kw.pop("_ids_sink", False) else None
    torch.manual_seed(0)
    if kw.pop("sharded", False):
        ids_out = []
        mine, wavs, lens = pipe.infer_sharded(texts, speaker_index=[u % 2 for u in range(len(texts))], speaker_table=TABLE[:2], params_infer_code=params,
                                              params_refine_text=RefineTextParams(prompt="[oral_1]"), ids_out=ids_out, **kw)
        trace.append(["result", mine, _summary(wavs), lens, _summary(ids_out)])
    else:
        gen = pipe._infer(texts, kw.pop("stream", False), None, kw.pop("skip_refine_text", False), kw.pop("refine_text_only", False), kw.pop("use_decoder", True),
                          True, True, True, RefineTextParams(prompt="[oral_1]"), params, **({} if sink is None else {"_ids_sink": sink}), **kw)
        for n, y in enumerate(gen, 1):
            trace.append(["yield", _summary(y)])
            if n == close_after:
                gen.close()
        if sink is not None:
            trace.append(["ids_sink", [[int(u), int(i.shape[0]), int(i[0, 0])] for u, i in sink]])
    trace.append(["next_rand", float(torch.rand(1))])                 # how far the request moved torch's CPU generator
    return json.loads(json.dumps(trace))


@pytest.mark.parametrize("name", sorted(CASES))
def test_request_trace(name, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = _run(name, monkeypatch)
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: trace entry {i}"
    if "closed" in name:
        assert got[-2] == ["set_row_adapters", None]


def test_every_case_is_recorded():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(CASES)


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    lines = [f"{json.dumps(name)}: {json.dumps(_run(name, mp), sort_keys=True)}" for name in sorted(CASES)]      # one case per line
    mp.undo()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
