"""Host side of the per-token log-probs of generate() and of candidate ranking (no GPU): GenerationOutputs' defaulted fields, the candidate noise-key
scheme and its refusals, the selection rule (ties, empty candidates), infer(return_details / num_candidates) on a stub engine, the new ABI symbols."""
import os
import re

import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import GenerationOutputs
from chatttsplus_amd.pipeline import (CANDIDATE_SHIFT, CandidateDetails, InferCodeParams, InferDetails, candidate_utt_id, check_candidate_request,
                                      mean_logprob, select_candidate)
from tests.test_row_sampling_host import _FakeSynth, _pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generation_outputs_defaults():
    o = GenerationOutputs(ids=[torch.zeros(2, 4)], attentions=[], hiddens=[])
    assert o.logprobs is None and o.sampled_logprobs is None and o.final_logprobs is None
    o = GenerationOutputs([], [], [], logprobs=[torch.zeros(1, 4)], sampled_logprobs=[torch.zeros(1, 4)], final_logprobs=[None])
    assert o.final_logprobs == [None]


def test_candidate_id_scheme():
    assert CANDIDATE_SHIFT == 48
    assert candidate_utt_id(7, 0) == 7                       # candidate 0 is the plain generation
    assert candidate_utt_id(7, 3) == 7 | (3 << 48)
    assert candidate_utt_id((1 << 48) - 1, 1) == (1 << 49) - 1
    keys = {candidate_utt_id(u, k) for u in range(50) for k in range(8)}
    assert len(keys) == 400 and max(keys) < 1 << 64
    assert check_candidate_request(1, [1 << 60], True, "torch") == 1          # N = 1 is today's call: nothing is refused
    assert check_candidate_request(4, [0, 5, (1 << 48) - 1], False, "auto") == 4
    with pytest.raises(_lib.HipBackendError, match=r"not below 2\^48"):
        check_candidate_request(2, [3, 1 << 48], False, "device")
    with pytest.raises(_lib.HipBackendError, match="stream=False"):
        check_candidate_request(2, [0], True, "device")
    with pytest.raises(_lib.HipBackendError, match="device noise"):
        check_candidate_request(2, [0], False, "torch")
    with pytest.raises(_lib.HipBackendError, match="device noise"):
        check_candidate_request(2, [0], False, torch.ones(3, 4, 626))
    for bad in (0, -1, 1.5, None):
        with pytest.raises(_lib.HipBackendError, match="integer >= 1"):
            check_candidate_request(bad, [0], False, "device")


def test_selection_rule():
    assert select_candidate([-3.0, -1.0, -2.0]) == 1
    assert select_candidate([-1.0, -1.0, -2.0]) == 0                       # ties: the lowest index
    assert select_candidate([-2.0, -1.0, -1.0]) == 1
    ninf = float("-inf")
    assert select_candidate([ninf, -9.0, ninf]) == 1                       # a candidate with no tokens ranks last
    assert select_candidate([ninf, ninf]) == 0
    assert select_candidate([float("nan"), -5.0]) == 1
    assert mean_logprob(torch.zeros(0, 4)) == ninf
    lp = torch.tensor([[-1.0, -2.0, -3.0, -4.0], [-1.0, -1.0, -1.0, -1.0]])
    assert mean_logprob(lp) == pytest.approx(-1.75)


class _LpGPT:
    """hip_models.GPT stand-in: row r of a call gets 2 + (uid mod 3) tokens, ids filled with its candidate index, raw log-probs -(1 + SCORE[k])."""
    num_vq, model_dim, max_batch = 4, 8, 8
    SCORE = [0.5, 0.25, 0.0, 0.75]

    def __init__(self):
        self.emb_code = [type("E", (), dict(num_embeddings=626))() for _ in range(4)]
        self.calls = []

    def __call__(self, input_ids, text_mask, spk_emb=None, spk_emb_ids=None):
        return torch.zeros(input_ids.shape[0], input_ids.shape[1], self.model_dim)

    def _out(self, kw, B):
        assert kw.get("return_logprobs") is True
        uids = [int(u) for u in kw.get("utt_ids") or range(B)]
        self.calls.append(dict(uids=uids, noise=kw.get("noise"), seed=kw.get("seed")))
        ids, lps, slps = [], [], []
        for u in uids:
            k, n = u >> 48, 2 + (u & 0xFFFF) % 3
            ids.append(torch.full((n, 4), k, dtype=torch.long))
            lps.append(torch.full((n, 4), -(1.0 + self.SCORE[k])))
            slps.append(torch.full((n, 4), -0.5))
        return GenerationOutputs(ids=ids, attentions=[], hiddens=[torch.full((i.shape[0], 768), 1.0) for i in ids], logprobs=lps, sampled_logprobs=slps,
                                 final_logprobs=[None] * len(ids))

    def generate(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, **kw):
        yield self._out(kw, emb.shape[0])

    def generate_many_iter(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, **kw):
        out = self._out(kw, emb.shape[0])
        yield [(b, out.ids[b], out.hiddens[b], None) for b in range(len(out.ids))]
        return out


class _CountSynth(_FakeSynth):
    def __init__(self):
        self.decoded = 0

    def decode_batch(self, hiddens):
        self.decoded += len(hiddens)
        return super().decode_batch(hiddens)


TEXTS = ["a b c", "a b c d a b", "a", "b c d a", "c c c"]
BASE = InferCodeParams(prompt="", max_new_token=64, show_tqdm=False, spk_emb=torch.ones(8))


def _lp_pipe(tmpdir):
    pipe = _pipe(tmpdir)
    pipe.models_dict["gpt"] = _LpGPT()
    pipe.synth = _CountSynth()
    return pipe


@pytest.mark.parametrize("mode", ["slices", "continuous"])
def test_return_details_and_candidates_on_a_stub_engine(tmp_path, mode):
    pipe = _lp_pipe(str(tmp_path))
    kw = dict(slice_size=8, continuous=(mode == "continuous"))
    out = list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise_seed=5, num_candidates=4, return_details=True, **kw))
    g = pipe.models_dict["gpt"]
    assert all(isinstance(d, InferDetails) for d in out)
    assert len(out) == (1 if mode == "continuous" else 3)                    # 8 rows / 4 candidates = 2 utterances per slice
    served = [u for c in g.calls for u in c["uids"]]
    assert served == [candidate_utt_id(u, k) for u in range(5) for k in range(4)]
    assert all(c["seed"] == 5 for c in g.calls)
    assert pipe.synth.decoded == 5                                           # only winners are vocoded
    cand = [k for d in out for k in d.candidate]
    assert cand == [2] * 5                                                   # the highest mean log-prob
    u = 0
    for d in out:
        for j in range(len(d.wavs)):
            n = 2 + u % 3
            assert d.ids[j].shape == (n, 4) and int(d.ids[j][0, 0]) == 2
            assert d.logprobs[j].shape == (n, 4) and d.sampled_logprobs[j].shape == (n, 4)
            assert d.mean_logprob[j] == pytest.approx(-1.0)
            assert d.candidate_scores[j].tolist() == pytest.approx([-1.5, -1.25, -1.0, -1.75])
            assert int(d.candidate_scores[j].argmax()) == d.candidate[j]
            assert [int(c.ids[0, 0]) for c in d.candidates[j]] == [0, 1, 2, 3]
            assert d.wavs[j].shape[0] == 256 * (2 * n - 1)
            u += 1
    assert u == 5
    # select overrides the rule and receives the candidates' details
    seen = []

    def pick(cands):
        seen.append([type(c) for c in cands])
        return 3

    pipe = _lp_pipe(str(tmp_path))
    out = list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise_seed=5, num_candidates=4, return_details=True, select=pick, **kw))
    assert [k for d in out for k in d.candidate] == [3] * 5 and all(s == [CandidateDetails] * 4 for s in seen) and len(seen) == 5
    assert all(int(i[0, 0]) == 3 for d in out for i in d.ids)
    with pytest.raises(_lib.HipBackendError, match="not a candidate index"):
        list(_lp_pipe(str(tmp_path))._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, num_candidates=4, select=lambda c: 4, **kw))
    # without return_details the winners' waveforms come back as the plain list
    pipe = _lp_pipe(str(tmp_path))
    out = list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, num_candidates=4, **kw))
    assert all(isinstance(w, list) for w in out) and sum(len(w) for w in out) == 5 and pipe.synth.decoded == 5


def test_return_details_without_candidates(tmp_path):
    pipe = _lp_pipe(str(tmp_path))
    out = list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", noise_seed=9, return_details=True, slice_size=3))
    assert [len(d.wavs) for d in out] == [3, 2]
    assert all(d.candidate is None and d.candidate_scores is None and d.candidates is None for d in out)
    assert [c["uids"] for c in pipe.models_dict["gpt"].calls] == [[0, 1, 2], [3, 4]]          # the plain call's ids: candidate 0
    assert all(m == pytest.approx(-1.5) for d in out for m in d.mean_logprob)


def test_candidate_refusals(tmp_path):
    pipe = _lp_pipe(str(tmp_path))
    run = lambda **kw: list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, **kw))      # noqa: E731
    with pytest.raises(_lib.HipBackendError, match="stream=False"):
        run(num_candidates=2, stream=True)
    with pytest.raises(_lib.HipBackendError, match="stream=False"):
        run(return_details=True, stream=True)
    with pytest.raises(_lib.HipBackendError, match="device noise"):
        run(num_candidates=2, noise="torch")
    with pytest.raises(_lib.HipBackendError, match=r"not below 2\^48"):
        run(num_candidates=2, utt_ids=[0, 1, 2, 3, 1 << 48])
    with pytest.raises(_lib.HipBackendError, match="exceeds slice_size"):
        run(num_candidates=4, slice_size=3)
    with pytest.raises(_lib.HipBackendError, match="infer_sharded"):
        pipe.infer_sharded(list(TEXTS), params_infer_code=BASE, num_candidates=2)
    assert pipe.models_dict["gpt"].calls == []


def test_new_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    for name, nargs in (("ctts_gpt_set_logprob_out", 4), ("ctts_sampler_run_rows_lp", 13)):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs == len(bound[name]), name
        assert hasattr(_lib.load(), name)
    for word in ("lp_raw", "lp_sampled", "-inf", "end_idx", "restart", "batch_invariant"):
        assert word in hdr[hdr.index("Log-probs of the sampled ids"):hdr.index("ctts_gpt_set_logprob_out(")], word
    lib = _lib.load()
    assert lib.ctts_gpt_set_logprob_out(None, None, None, None) != 0 and b"no generate state" in lib.ctts_last_error()
