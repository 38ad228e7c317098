"""Shared prompt passes, host side (no GPU): the index bookkeeping of GPT.generate(prompt_of=...) / generate_many (hip_models.gpt.prompt_groups) with its
refusals, how infer(share_prompt=...) resolves (pipeline.resolve_share_prompt), what the pipeline hands a stub engine when the candidates of an utterance
share its prompt, and the new ABI symbol."""
import os
import re

import pytest
import torch

from chatttsplus_amd import _lib
from chatttsplus_amd.hip_models.gpt import prompt_groups
from chatttsplus_amd.pipeline import candidate_utt_id, resolve_share_prompt
from tests.test_gen_logprobs_host import BASE, TEXTS, _LpGPT, _lp_pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- prompt_groups -------------------------------------------------------------------------------------------------------------------------------
def test_leader_is_the_first_occurrence():
    prompts, local, leaders = prompt_groups([0, 0, 0, 1, 1, 1], 2)
    assert prompts == [0, 1] and local == [0, 0, 0, 1, 1, 1] and leaders == [0, 3]
    # one sequence per prompt: every sequence leads itself
    assert prompt_groups([0, 1, 2], 3) == ([0, 1, 2], [0, 1, 2], [0, 1, 2])
    assert prompt_groups([0], 1) == ([0], [0], [0])


def test_non_adjacent_and_unsorted_groups():
    prompts, local, leaders = prompt_groups([1, 0, 1, 2, 0, 1], 3)
    assert prompts == [1, 0, 2]                      # in order of first use: the rows of emb / mask the call passes
    assert local == [0, 1, 0, 2, 1, 0]               # re-indexed into `prompts`
    assert leaders == [0, 1, 3]                      # sequences 0, 1 and 3 run the prompt pass; 2, 4 and 5 receive a copy
    for j, i in enumerate(leaders):
        assert local[i] == j and j not in local[:i]


def test_subset_reindexing():
    pof = [1, 0, 1, 2, 0, 1]
    # an admission that seats sequences 5, 2 and 4: two prompts, sequence 5 leads prompt 1
    assert prompt_groups(pof, 3, subset=[5, 2, 4]) == ([1, 0], [0, 0, 1], [0, 2])
    # a subset with one sequence per prompt shares nothing
    assert prompt_groups(pof, 3, subset=[3, 4]) == ([2, 0], [0, 1], [0, 1])
    assert prompt_groups(pof, 3, subset=[4]) == ([0], [0], [0])
    # the whole list as a subset is the default
    assert prompt_groups(pof, 3, subset=range(6)) == prompt_groups(pof, 3)


def test_adapter_slots_inside_a_group():
    pof = [0, 0, 1, 1]
    assert prompt_groups(pof, 2, slots=[2, 2, -1, None]) == ([0, 1], [0, 0, 1, 1], [0, 2])          # one slot or none per group (-1 and None both mean none)
    with pytest.raises(_lib.HipBackendError, match=r"sequences 0 and 1 share prompt 0 but carry different adapter slots \(2, 3\).*one slot or none"):
        prompt_groups(pof, 2, slots=[2, 3, -1, -1])
    with pytest.raises(_lib.HipBackendError, match=r"sequences 2 and 3 share prompt 1 .*\(-1, 0\)"):
        prompt_groups(pof, 2, slots=[2, 2, None, 0])
    # only the sequences seated together are compared
    assert prompt_groups(pof, 2, slots=[2, 3, -1, -1], subset=[1, 2, 3]) == ([0, 1], [0, 1, 1], [0, 1])
    with pytest.raises(_lib.HipBackendError, match="4 sequences"):
        prompt_groups(pof, 2, slots=[0, 0])


def test_refusals_name_their_cause():
    with pytest.raises(_lib.HipBackendError, match=r"prompt_of: 3 entries for 4 sequences"):
        prompt_groups([0, 1, 1], 2, n=4)
    with pytest.raises(_lib.HipBackendError, match=r"prompt_of\[2\]=2 is out of range: the call has 2 prompts"):
        prompt_groups([0, 1, 2], 2)
    with pytest.raises(_lib.HipBackendError, match=r"prompt_of\[0\]=-1 is out of range"):
        prompt_groups([-1, 0], 1)
    with pytest.raises(_lib.HipBackendError, match=r"prompt 1 is named by no sequence"):
        prompt_groups([0, 2, 2], 3)
    with pytest.raises(_lib.HipBackendError, match=r"code mode only.*infer_text"):
        prompt_groups([0, 0], 1, infer_text=True)


# ---- share_prompt ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invariant", [0, 1])
def test_share_prompt_resolution(invariant):
    assert resolve_share_prompt(None, 4, invariant) is bool(invariant)        # None: exactly on invariant engines
    assert resolve_share_prompt(True, 4, invariant) is True
    assert resolve_share_prompt(False, 4, invariant) is False
    for n in (None, 1):                                                       # nothing to share: a no-op whatever is asked
        for sp in (None, True, False):
            assert resolve_share_prompt(sp, n, invariant) is False
    with pytest.raises(_lib.HipBackendError, match="share_prompt must be None, True or False"):
        resolve_share_prompt("yes", 4, invariant)
    with pytest.raises(_lib.HipBackendError, match="share_prompt must be None, True or False"):
        resolve_share_prompt(2, 4, invariant)


class _ShareGPT(_LpGPT):
    """_LpGPT that records how many prompts it embedded and which prompt each row named"""

    def __init__(self, invariant):
        super().__init__()
        self.invariant, self.seen = invariant, []

    def get_option(self, name):
        assert name == "batch_invariant"
        return self.invariant

    def _out(self, kw, B):
        pof = kw.pop("prompt_of", None)
        self.seen.append((B, pof))
        return super()._out(kw, len(pof) if pof is not None else B)


@pytest.mark.parametrize("mode", ["slices", "continuous"])
@pytest.mark.parametrize("invariant,share_prompt,shared", [(1, None, True), (0, None, False), (0, True, True), (1, False, False)])
def test_pipeline_hands_prompts_once_and_rows_per_candidate(tmp_path, mode, invariant, share_prompt, shared):
    pipe = _lp_pipe(str(tmp_path))
    g = pipe.models_dict["gpt"] = _ShareGPT(invariant)
    kw = dict(slice_size=8, continuous=(mode == "continuous"), share_prompt=share_prompt)
    out = list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise_seed=5, num_candidates=4, return_details=True, **kw))
    # the rows served and the winners are those of the unshared call (tests/test_gen_logprobs_host.py)
    assert [u for c in g.calls for u in c["uids"]] == [candidate_utt_id(u, k) for u in range(5) for k in range(4)]
    assert [k for d in out for k in d.candidate] == [2] * 5
    groups = [5] if mode == "continuous" else [2, 2, 1]                      # utterances per call
    assert len(g.seen) == len(groups)
    for (n_emb, pof), n_utt in zip(g.seen, groups):
        if shared:
            assert n_emb == n_utt and pof == [j for j in range(n_utt) for _ in range(4)]      # every utterance tokenised and embedded once
        else:
            assert n_emb == 4 * n_utt and pof is None
    # one candidate per utterance: share_prompt is a no-op
    g.seen.clear()
    list(pipe._infer(list(TEXTS), skip_refine_text=True, params_infer_code=BASE, noise="device", noise_seed=5, return_details=True, slice_size=8, share_prompt=True))
    assert g.seen == [(5, None)]


def test_per_prompt_and_per_row_arguments(tmp_path):
    """speaker rows and prompt prefixes go per PROMPT, limits and sampling per ROW"""
    pipe = _lp_pipe(str(tmp_path))
    seen = {}

    class G(_ShareGPT):
        def __call__(self, input_ids, text_mask, spk_emb=None, spk_emb_ids=None):
            seen["spk_rows"] = None if spk_emb is None or torch.as_tensor(spk_emb).dim() < 2 else int(torch.as_tensor(spk_emb).shape[0])
            return super().__call__(input_ids, text_mask, spk_emb, spk_emb_ids)

        def _out(self, kw, B):
            seen.update(limits=kw.get("max_new_tokens_per_row"), sampling=kw.get("sampling_per_row"))
            return super()._out(kw, B)

    pipe.models_dict["gpt"] = G(1)
    texts = TEXTS[:2]
    spk = torch.stack([torch.ones(8), 2 * torch.ones(8)])
    import dataclasses
    params = dataclasses.replace(BASE, spk_emb=spk)
    per = [dict(temperature=0.5), dict(max_new_token=40)]
    list(pipe._infer(list(texts), skip_refine_text=True, params_infer_code=params, noise_seed=5, num_candidates=3, slice_size=8, params_per_utterance=per))
    assert seen["spk_rows"] == 2
    assert seen["limits"] == [64, 64, 64, 40, 40, 40]
    assert seen["sampling"] == [dict(temperature=0.5)] * 3 + [None] * 3


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "ctts_hip.h")).read()
    assert re.search(r"int ctts_gpt_share_prompts\(ctts_gpt\* h, int n, const int32_t\* prompt_of_host, int n_prompts\);", header)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "ctts_gpt_share_prompts" in bound and len(bound["ctts_gpt_share_prompts"][1]) == 4
    assert "`ctts_gpt_share_prompts`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "kv_share.hip" in __import__("chatttsplus_amd.build", fromlist=["SOURCES"]).SOURCES
