"""Host side of the refine-text log-probs (no GPU): the ranking of refine candidates (length-normalised mean raw log-prob with the [Ebreak] step, the tie rule,
the utterance-id keying) on a stub engine, each refusal by name, InferDetails' defaulted fields, score_text_inputs' layout, the shapes OutBuffers.take hands out
for text rows, the new ABI symbols."""
import os
import re

import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import GenerationOutputs, OutBuffers, SessionResult, refuse_out_of_scope, score_text_inputs
from chatttsplus_amd.pipeline import (InferCodeParams, InferDetails, RefinedTexts, RefineTextParams, candidate_utt_id, check_refine_candidates, rank_refinements)
from tests.test_gen_logprobs_host import _CountSynth, _LpGPT
from tests.test_row_sampling_host import _pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD, WORD_ID = "[uv_break]", 9       # a token of the toy vocabulary below [break_0] that the code prompt keeps: it survives the decoding of a refinement and tokenises back to one id
# candidate k of a text: every token -LP[k], the step that sampled [Ebreak] -FIN[k].  Without the [Ebreak] step candidate 0 would win; with it 1 and 2 tie for
# the best mean and the lower index is taken; candidate 3 ends by its limit (no [Ebreak] step) and is worst
LP, FIN = [1.0, 1.2, 1.2, 3.0], [4.0, 0.2, 0.2, None]


def _mean(k, n):
    return -(n * LP[k] + (FIN[k] if FIN[k] is not None else 0.0)) / (n + (FIN[k] is not None))


class _RefineGPT(_LpGPT):
    """_LpGPT whose infer_text calls refine: row (u, k) gets 2 + u % 3 + k tokens WORD (the candidate shows in the length), raw log-probs from LP / FIN"""

    def __init__(self):
        super().__init__()
        self.text_calls, self.embedded = [], []

    def __call__(self, input_ids, text_mask, spk_emb=None, spk_emb_ids=None):
        self.embedded.append((input_ids[..., 0] == WORD_ID).sum(1).tolist())
        return super().__call__(input_ids, text_mask, spk_emb, spk_emb_ids)

    def _refine(self, emb, kw, how):
        assert kw.get("infer_text") is True
        uids = [int(u) for u in kw.get("utt_ids") or range(emb.shape[0])]
        self.text_calls.append(dict(how=how, uids=uids, seed=kw.get("seed"), rows=kw.get("rows"), lp=kw.get("return_text_logprobs", False), noise=kw.get("noise")))
        ids = [torch.full((2 + (u & 0xFFFF) % 3 + (u >> 48),), WORD_ID, dtype=torch.long) for u in uids]
        if not kw.get("return_text_logprobs"):
            return GenerationOutputs(ids=ids, attentions=[], hiddens=[])
        ks = [u >> 48 for u in uids]
        return GenerationOutputs(ids=ids, attentions=[], hiddens=[], logprobs=[torch.full((i.shape[0],), -LP[k]) for i, k in zip(ids, ks)],
                                 sampled_logprobs=[torch.full((i.shape[0],), -0.5) for i in ids],
                                 final_logprobs=[None if FIN[k] is None else torch.tensor([-FIN[k], -0.1]) for k in ks])

    def generate(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, **kw):
        if kw.get("infer_text"):
            yield self._refine(emb, kw, "generate")
        else:
            yield from super().generate(emb, inputs_ids, temperature, eos_token, attention_mask, **kw)

    def generate_many(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, **kw):
        return self._refine(emb, kw, "generate_many")


TEXTS = ["a b c", "a b c d a b", "a", "b c d a", "c c c"]
BASE = InferCodeParams(prompt="", max_new_token=64, show_tqdm=False, spk_emb=torch.ones(8))
REFINE = RefineTextParams(prompt="", max_new_token=16, show_tqdm=False)


def _rpipe(tmpdir):
    pipe = _pipe(tmpdir)
    pipe.models_dict["gpt"] = _RefineGPT()
    pipe.synth = _CountSynth()
    return pipe


def test_rank_refinements_mean_with_the_eos_step_and_the_tie_rule():
    ids = [torch.full((2,), k) for k in range(4)] + [torch.full((3,), 10 + k) for k in range(4)]
    lps = [torch.full((i.shape[0],), -LP[k % 4]) for k, i in enumerate(ids)]
    fls = [None if FIN[k % 4] is None else torch.tensor([-FIN[k % 4], -0.1]) for k in range(8)]
    r = rank_refinements(ids, lps, fls, 4)
    assert isinstance(r, RefinedTexts) and r.candidate == [1, 1]                              # 1 and 2 tie: the lower index; 0 wins only without its [Ebreak] step
    assert [int(i[0]) for i in r.ids] == [1, 11]
    assert r.logprobs[0].tolist() == pytest.approx([-1.2, -1.2, -0.2]) and r.logprobs[1].shape == (4,)
    assert r.mean_logprob == pytest.approx([_mean(1, 2), _mean(1, 3)])
    assert r.candidate_scores[0].tolist() == pytest.approx([_mean(k, 2) for k in range(4)])
    assert _mean(0, 2) < _mean(1, 2) and -LP[0] > -LP[1]
    one = rank_refinements(ids[:2], lps[:2], fls[:2], 1)                                   # N = 1: log-probs only, no candidate fields
    assert one.candidate is None and one.candidate_scores is None and [int(i[0]) for i in one.ids] == [0, 1]
    empty = rank_refinements([torch.zeros(0, dtype=torch.long), ids[1]], [torch.zeros(0), lps[1]], [None, fls[1]], 2)
    assert empty.candidate == [1]                                                          # a candidate without a step ranks last


@pytest.mark.parametrize("mode", ["slices", "continuous"])
def test_refine_candidates_on_a_stub_engine(tmp_path, mode):
    pipe = _rpipe(str(tmp_path))
    g = pipe.models_dict["gpt"]
    kw = dict(slice_size=4, continuous=(mode == "continuous"), params_refine_text=REFINE, params_infer_code=BASE, noise_seed=5)
    out = list(pipe._infer(list(TEXTS), refine_text_only=True, refine_candidates=4, utt_ids=[10, 11, 12, 13, 14], **kw))
    texts = [t for o in out for t in o]
    assert [t.count(WORD) for t in texts] == [2 + u % 3 + 1 for u in (10, 11, 12, 13, 14)]      # every text's winner is candidate 1: one token more than the plain refinement
    assert all(max(range(4), key=lambda k: (_mean(k, 2 + b + k), -k)) == 1 for b in range(3))
    served = [u for c in g.text_calls for u in c["uids"]]
    assert served == [candidate_utt_id(u, k) for u in (10, 11, 12, 13, 14) for k in range(4)]  # text-major, candidate 0 under the plain id
    assert all(c["seed"] == 5 and c["lp"] is True and c["how"] == "generate_many" and c["rows"] == 4 for c in g.text_calls)
    assert len(g.text_calls) == (1 if mode == "continuous" else 2) and g.calls == []
    # refine_candidates=1 is the plain call: no log-probs are asked for, the plain utterance ids
    pipe = _rpipe(str(tmp_path))
    plain = list(pipe._infer(list(TEXTS), refine_text_only=True, refine_candidates=1, **kw))
    tc = pipe.models_dict["gpt"].text_calls
    own = (lambda u: u) if mode == "continuous" else (lambda u: u % 4)                         # (the plain sliced refine pass numbers every slice's texts from 0)
    assert all(c["lp"] is False for c in tc) and [t.count(WORD) for o in plain for t in o] == [2 + own(u) % 3 for u in range(5)]
    assert list(_rpipe(str(tmp_path))._infer(list(TEXTS), refine_text_only=True, **kw)) == plain


def test_the_winner_feeds_the_code_pass_and_details_carry_the_refine_log_probs(tmp_path):
    pipe = _rpipe(str(tmp_path))
    g = pipe.models_dict["gpt"]
    out = list(pipe._infer(list(TEXTS), params_refine_text=REFINE, params_infer_code=BASE, noise="device", noise_seed=9, return_details=True, refine_candidates=3,
                           slice_size=3))
    assert all(isinstance(d, InferDetails) for d in out) and [len(d.wavs) for d in out] == [3, 2]
    u = 0
    for d in out:
        for j in range(len(d.wavs)):
            n = 2 + u % 3 + 1
            assert d.refined_logprobs[j].tolist() == pytest.approx([-LP[1]] * n + [-FIN[1]]) and d.refined_mean_logprob[j] == pytest.approx(_mean(1, n))
            u += 1
    code_prompts = [n for e in g.embedded[-2:] for n in e]                                     # the code pass's prompts hold the winners' words: candidate 1's count
    assert code_prompts == [2 + u % 3 + 1 for u in range(5)]
    assert [c["uids"] for c in g.calls] == [[0, 1, 2], [3, 4]]                                  # the code pass is the plain one
    # without refine candidates the details still carry the plain refinement's log-probs; with the pass skipped both fields stay None
    pipe = _rpipe(str(tmp_path))
    out = list(pipe._infer(list(TEXTS), params_refine_text=REFINE, params_infer_code=BASE, noise="device", noise_seed=9, return_details=True, slice_size=8))
    assert out[0].refined_mean_logprob == pytest.approx([_mean(0, 2 + u % 3) for u in range(5)]) and out[0].refined_logprobs[2].shape == (4 + 1,)
    assert pipe.models_dict["gpt"].text_calls[0]["lp"] is True
    out = list(_rpipe(str(tmp_path))._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", noise_seed=9, return_details=True, slice_size=8))
    assert out[0].refined_logprobs is None and out[0].refined_mean_logprob is None


def test_infer_details_defaults():
    d = InferDetails(wavs=[], ids=[], logprobs=[], sampled_logprobs=[], mean_logprob=[])
    assert d.refined_logprobs is None and d.refined_mean_logprob is None and d.candidate is None
    r = SessionResult(ticket=0, utt_id=0, ids=torch.zeros(3, dtype=torch.long), mode="text")
    assert r.logprobs is None and r.sampled_logprobs is None and r.final_logprobs is None


def test_refusals_by_name(tmp_path):
    pipe = _rpipe(str(tmp_path))
    run = lambda **kw: list(pipe._infer(list(TEXTS), params_refine_text=REFINE, params_infer_code=BASE, refine_text_only=True, **kw))      # noqa: E731
    with pytest.raises(_lib.HipBackendError, match="refine_candidates > 1 needs stream=False"):
        run(refine_candidates=2, stream=True)
    with pytest.raises(_lib.HipBackendError, match="refine_candidates > 1 needs device noise"):
        run(refine_candidates=2, noise="torch")
    with pytest.raises(_lib.HipBackendError, match="refine_candidates > 1 needs device noise"):
        run(refine_candidates=2, noise=torch.ones(3, 5, 17))
    with pytest.raises(_lib.HipBackendError, match="refine_candidates=4 exceeds slice_size=3"):
        run(refine_candidates=4, slice_size=3)
    with pytest.raises(_lib.HipBackendError, match=r"not below 2\^48"):
        run(refine_candidates=2, utt_ids=[0, 1, 2, 3, 1 << 48])
    for bad in (0, -1, 1.5, None):
        with pytest.raises(_lib.HipBackendError, match="refine_candidates must be an integer >= 1"):
            run(refine_candidates=bad)
    with pytest.raises(_lib.HipBackendError, match=r"infer_sharded\(refine_candidates"):
        pipe.infer_sharded(list(TEXTS), params_infer_code=BASE, refine_candidates=2)
    with pytest.raises(_lib.HipBackendError, match=r"ranked refine candidates \(refine_candidates=\) is not offered inside a session"):
        pipe.open_session(BASE, refine_candidates=2)
    with pytest.raises(_lib.HipBackendError, match="ranked refine candidates"):
        refuse_out_of_scope(dict(refine_candidates=3), "use infer() for it")
    refuse_out_of_scope(dict(refine_candidates=1), "use infer() for it")                   # the value that means "off"
    assert check_refine_candidates(1, [1 << 60], True, "torch", 1) == 1                     # N = 1 is today's call: nothing is refused
    assert check_refine_candidates(4, [0, 5], False, "auto", 4) == 4
    g = pipe.models_dict["gpt"]
    assert g.text_calls == [] and g.calls == []


def test_score_text_inputs_layout():
    ids = torch.zeros(2, 5, 4, dtype=torch.long)
    mask = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1]])
    ids[0, :, :] = torch.arange(100, 105)[:, None]
    ids[1, 2:, :] = torch.arange(200, 203)[:, None]
    si = score_text_inputs(ids, mask, [torch.tensor([7, 8]), [9, 10, 11, 12]], eos_token=99)
    assert si["ids"].shape == (2, 7, 4) and si["mask"].tolist() == [[1] * 7, [1] * 7]          # 5 + 2 and 3 + 4 rows: prompt, then every refined id as an input row
    assert si["ids"][0, :, 0].tolist() == [100, 101, 102, 103, 104, 7, 8] and si["ids"][1, :, 0].tolist() == [200, 201, 202, 9, 10, 11, 12]
    assert bool((si["ids"] == si["ids"][:, :, :1]).all()) and bool(si["text_mask"].all())       # the id on every column; every row a text row
    assert si["n_targets"].tolist() == [3, 5] and si["targets"].shape == (2, 5) and si["targets"].dtype == torch.int32
    assert si["targets"][0, :3].tolist() == [7, 8, 99] and si["targets"][1].tolist() == [9, 10, 11, 12, 99]
    # target j of sequence b is predicted by row T' - n_b + j: the row before the first refined id predicts it
    assert si["ids"][0, 7 - 3, 0] == 104 and si["ids"][1, 7 - 5, 0] == 202
    no = score_text_inputs(ids, mask, [torch.tensor([7, 8, 6]), [9, 10, 11, 12]], eos_token=99, append_eos=False)      # the last id is a target only: 5 + 2 and 3 + 3 rows
    assert no["n_targets"].tolist() == [3, 4] and no["ids"].shape == (2, 7, 4) and no["mask"].tolist() == [[1] * 7, [0] + [1] * 6]
    assert no["ids"][1, :, 0].tolist() == [0, 200, 201, 202, 9, 10, 11] and not bool(no["text_mask"][1, 0]) and no["targets"][0, :3].tolist() == [7, 8, 6]
    empty = score_text_inputs(ids, mask, [[], [5]], eos_token=99)                            # an empty refinement scores its [Ebreak] alone: n_b = 1
    assert empty["n_targets"].tolist() == [1, 2] and empty["targets"][0, 0] == 99
    with pytest.raises(ValueError, match="nothing to score"):
        score_text_inputs(ids, mask, [[], [5]], eos_token=99, append_eos=False)
    with pytest.raises(ValueError, match="2 prompts"):
        score_text_inputs(ids, mask, [[1]], eos_token=99)
    with pytest.raises(ValueError, match="LEFT"):
        score_text_inputs(ids, mask.flip(1), [[1], [2]], eos_token=99)


def test_out_buffers_take_shapes_for_text_rows():
    g = type("G", (), dict(device=torch.device("cpu"), num_vq=4, model_dim=8))()
    # a code state with text rows: text log-probs [2, n, text max_new] beside the text ids, one value per step
    out = OutBuffers(3, 6, g, False, True, text_new=4, text_logprobs=True)
    assert out.tlps.shape == (2, 3, 4) and out.lps.shape == (2, 3, 6, 4) and out.tids.shape == (3, 4, 4)
    out.tids[:] = 5; out.tlps[0] = -1.0; out.tlps[1] = -2.0; out.ids[:] = 1; out.lps[:] = -3.0
    ids, hid, lp, slp, flp = out.take(1, 2, True, text_row=True)
    assert ids.shape == (2,) and ids.dtype == torch.long and hid is None and lp.shape == (2,) and slp.shape == (2,) and flp.tolist() == [-1.0, -2.0]
    assert out.take(1, 4, True, text_row=True)[4] is None                                   # ended by its limit: no step at index n
    assert out.take(1, 2, False, text_row=True)[4] is None
    ids, hid, lp, slp, flp = out.take(0, 3, True)                                           # a code row of the same state: its own [n, 4] arrays
    assert ids.shape == (3, 4) and lp.shape == (3, 4) and flp.shape == (2, 4) and float(lp[0, 0]) == -3.0
    # return_logprobs alone stays code-only: a text row then carries none
    assert OutBuffers(3, 6, g, False, True, text_new=4).take(1, 2, True, text_row=True)[2:] == (None, None, None)
    # an infer_text state: [2, n, max_new]; ids [n], log-probs [n], final [2]
    t = OutBuffers(2, 5, g, False, False, text_logprobs=True, infer_text=True)
    assert t.tlps.shape == (2, 2, 5) and t.lps is None
    t.ids[:] = 3; t.tlps[:] = -0.5
    ids, hid, lp, slp, flp = t.take(0, 3, True, first_column=True)
    assert ids.shape == (3,) and lp.shape == (3,) and slp.shape == (3,) and flp.shape == (2,)
    assert OutBuffers(2, 5, g, False, False, infer_text=True).tlps is None                  # not asked for
    assert OutBuffers(2, 5, g, False, False, text_logprobs=True).tlps is None               # a code state without text rows has none


def test_new_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    for name, nargs in (("ctts_gpt_set_text_logprob_out", 4), ("ctts_gpt_score_text", 11), ("ctts_sampler_run_text_lp", 20)):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs == len(bound[name]), name
        assert hasattr(_lib.load(), name)
    for word in ("lp_raw", "lp_sampled", "-inf", "end_idx", "restart", "batch_invariant", "guided", "ONE value per step"):
        assert word in hdr[hdr.index("Log-probs of the refine-text pass"):hdr.index("ctts_gpt_set_text_logprob_out(ctts_gpt")], word
    assert "log-probs of text rows;" not in hdr and "returns no log-probs" not in hdr.split("ctts_gpt_set_text_logprob_out(ctts_gpt")[1][:10]
    lib = _lib.load()
    assert lib.ctts_gpt_set_text_logprob_out(None, None, None, None) != 0 and b"set_text_logprob_out: no generate state" in lib.ctts_last_error()
    assert lib.ctts_gpt_score_text(None, 1, 1, None, None, None, None, 1, None, None, None) != 0 and b"score_text: handle not ready" in lib.ctts_last_error()
