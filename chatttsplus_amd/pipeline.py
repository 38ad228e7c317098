"""ChatTTSPlusPipeline with `infer_type: "hip"` -- the drop-in surface of the reference's
chattts_plus/pipelines/chattts_plus_pipeline.py for the hot path:

    pipe = ChatTTSPlusPipeline(cfg, device=torch.device("cuda"))
    for wavs in pipe.infer(text, params_infer_code=InferCodeParams(...), skip_refine_text=True, ...): ...

What is kept: constructor kwargs, YAML layout (MODELS.<key>.{name,infer_type,kwargs}), `infer()` /
`_infer()` / `_infer_code()` / `_decode_to_wavs()` / speaker helpers, the generator-of-wav-lists result,
InferCodeParams / RefineTextParams, and the CPU text front-end in front of the path (text_frontend.py: sentence splitting,
number spelling, short-sentence merging, the Normalizer -- replaceable callables, defaults as in the reference).  The Chinese
number reader (zh_normalization) and nemo_text_processing are optional plug-ins.  There is no CPU fallback for the models.
"""
from __future__ import annotations

import dataclasses
import json
import math
import logging
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from . import _lib, codec, hip_models, text_frontend


@dataclass(repr=False, eq=False)
class RefineTextParams:                      # reference commons/utils.py:12-22
    prompt: str = ""
    top_P: float = 0.7
    top_K: int = 20
    temperature: float = 0.7
    repetition_penalty: float = 1.0
    max_new_token: int = 384
    min_new_token: int = 0
    show_tqdm: bool = True
    ensure_non_empty: bool = True


@dataclass(repr=False, eq=False)
class InferCodeParams(RefineTextParams):     # reference commons/utils.py:25-36
    prompt: str = "[speed_5]"
    spk_emb: Optional[str] = None
    spk_smp: Optional[str] = None
    txt_smp: Optional[str] = None
    temperature: float = 0.3
    repetition_penalty: float = 1.05
    max_new_token: int = 2048
    stream_batch: int = 24
    stream_speed: int = 12000
    pass_first_n_batches: int = 2


class TorchSeedContext:                        # reference commons/utils.py:48-58: seed torch's CPU generator for one request, restore it afterwards
    def __init__(self, seed):
        self.seed, self.state = seed, None

    def __enter__(self):
        self.state = torch.random.get_rng_state()
        torch.manual_seed(self.seed)

    def __exit__(self, exc_type, exc, tb):
        torch.random.set_rng_state(self.state)


# gen_logits and its scalar carriers live beside the sampler configuration they feed (hip_models/gpt.py): one conversion for a call's knobs and for an
# utterance's (sampling_per_row)
from .hip_models.gpt import LORA_TARGETS, TextGuide, _RepPenalty, _TopK, _TopP, check_lora_shapes, gen_logits, refuse_out_of_scope  # noqa: E402,F401
from .hip_models.vocoder import prefix_samples, prefix_tokens  # noqa: E402


# params_per_utterance (ChatTTSPlusPipeline.infer / infer_sharded): the InferCodeParams fields one utterance may set for itself.  The sampling knobs
# reach the engine's per-row table (GPT sampling_per_row, ctts_gpt_set_row_sampling); max_new_token becomes the utterance's token limit, prompt its
# [speed_N] / [oral_N] prefix, spk_emb its speaker row, spk_smp / txt_smp its cloned voice (the zero-shot audio prompt behind its text and the transcript of
# that clip in front of it: ClonedVoice.overrides()).  Every other field is per call.
NATIVE_RATE = 24000         # what the vocoder produces; infer(sample_rate=) / submit(sample_rate=) resample it on the device (hip_models.Resampler)
PER_UTTERANCE_SAMPLING = ("temperature", "top_P", "top_K", "repetition_penalty", "min_new_token")
PER_UTTERANCE_FIELDS = PER_UTTERANCE_SAMPLING + ("max_new_token", "prompt", "spk_emb", "spk_smp", "txt_smp")


@dataclass(eq=False)
class ClonedVoice:
    """One cloned voice (ChatTTSPlusPipeline.clone_voices): `spk_smp`, the base16384 audio-prompt string of the clip's codes, and `txt_smp`, the transcript of the
    clip.  `overrides()` is the params_per_utterance / SynthSession.submit(params=) entry that speaks an utterance in this voice."""
    spk_smp: str
    txt_smp: str = ""
    _codes: Optional[torch.Tensor] = dataclasses.field(default=None, repr=False)

    @property
    def codes(self) -> torch.Tensor:
        """the clip's codes [num_vq, T] (decoded once)"""
        if self._codes is None:
            self._codes = codec.decode_prompt(self.spk_smp)
        return self._codes

    def overrides(self) -> dict:
        """spk_emb None: no speaker vector of the entry's own -- a row that sets spk_smp gets the [empty_spk] tag, whatever the call's speaker"""
        return {"spk_smp": self.spk_smp, "txt_smp": self.txt_smp, "spk_emb": None}


def encode_clips(enc, wavs, what: str = "clip") -> List[torch.Tensor]:
    """The one door from the clip encoder to the host: DVAEEncoder.encode_batch(wavs) -> one code tensor int32 [num_vq, T_i] per clip, on the CPU.  The encoder marks a
    code frame whose features are not finite (a NaN or infinite sample in the clip: a bad decode, an overflowed resampler) with id -1; such a clip would otherwise
    be written into a prompt string as plausible codes (codec.encode_prompt casts to uint16).  It is refused here, by index."""
    codes = [c.cpu() for c in enc.encode_batch(wavs)]
    for i, c in enumerate(codes):
        bad = int((c < 0).any(0).sum())
        if bad:
            raise _lib.HipBackendError(f"{what} {i}: {bad} of {c.shape[1]} code frames are not finite -- the waveform holds NaN or infinite samples")
    return codes


def utterance_voices(base, diffs) -> Optional[list]:
    """params_per_utterance entries (per_utterance_overrides) -> one (speaker tag, txt_smp, spk_smp) per utterance, None when no entry touches spk_smp / txt_smp.
    An utterance that sets its own spk_smp speaks without a speaker vector ([empty_spk]; setting both is refused by per_utterance_overrides); every other utterance
    keeps the call's voice: its speaker row where the call has a speaker, the call's spk_smp / txt_smp where it has those."""
    if not any(("spk_smp" in d or "txt_smp" in d) for d in diffs):
        return None
    out = []
    for d in diffs:
        has_vec = "spk_emb" in d or (base.spk_emb is not None and d.get("spk_smp") is None)
        txt = d.get("txt_smp", base.txt_smp)
        out.append(("[spk_emb]" if has_vec else "[empty_spk]", "" if txt is None else txt, d.get("spk_smp", base.spk_smp)))
    return out


def _same_value(a, b) -> bool:
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and bool(torch.equal(a.cpu(), b.cpu()))
    try:
        return bool(a == b)
    except Exception:       # noqa: BLE001 (values that do not compare are different)
        return False


def per_utterance_overrides(base, entries) -> List[dict]:
    """`entries` (one InferCodeParams, dict of overrides or None per utterance) -> the fields in which each differs from `base`.  An entry's
    spk_emb of None means the call's speaker.  A field outside PER_UTTERANCE_FIELDS that differs raises HipBackendError naming it."""
    names = [f.name for f in dataclasses.fields(InferCodeParams)]
    out = []
    for i, e in enumerate(entries):
        if e is None:
            vals = {}
        elif isinstance(e, InferCodeParams):
            vals = {n: getattr(e, n) for n in names}
        elif isinstance(e, dict):
            unknown = sorted(set(e) - set(names))
            if unknown:
                raise _lib.HipBackendError(f"params_per_utterance: entry {i}: unknown field(s) {unknown}")
            vals = dict(e)
        else:
            raise _lib.HipBackendError(f"params_per_utterance: entry {i} is a {type(e).__name__} (InferCodeParams, dict or None)")
        if vals.get("spk_emb", 0) is None:
            vals.pop("spk_emb")
        diff = {k: v for k, v in vals.items() if not _same_value(v, getattr(base, k))}
        bad = [k for k in diff if k not in PER_UTTERANCE_FIELDS]
        if bad:
            raise _lib.HipBackendError(f"params_per_utterance: entry {i}: field {bad[0]!r} differs from params_infer_code but is per call "
                                       f"(per utterance: {', '.join(PER_UTTERANCE_FIELDS)})")
        if diff.get("spk_smp") is not None and "spk_emb" in diff:
            raise _lib.HipBackendError(f"params_per_utterance: entry {i} sets both spk_smp (a cloned voice) and spk_emb (a speaker vector): an utterance speaks in one "
                                       f"of them; leave spk_emb None beside spk_smp")
        out.append(diff)
    return out


def _with_uv_break(text: str) -> str:
    """pipeline:414-416: a text that goes to the code pass ends with [uv_break]."""
    return text if text.strip().endswith("[uv_break]") else text + " [uv_break]"


def _decode_refined(tok, ids_list) -> List[str]:
    """pipeline:406-411: the refine-text pass's ids without the control tokens from [break_0] up, as text."""
    return tok.decode([i[i.less(tok.break_0_ids)] for i in ids_list])


# -- guided refine-text (refine_guided=; GPT TextGuide): the refined text is provably the submitted tokens, with only prosody tokens inserted ----------------------
REFINE_FREE_TOKENS = ("[uv_break]", "[v_break]", "[lbreak]", "[llbreak]", "[laugh]")


def _token_id(tok, name: str) -> Optional[int]:
    """the id of a token the tokenizer knows, None for a name that maps to the unknown id"""
    bt = tok._tokenizer
    i = bt.convert_tokens_to_ids(name)
    return None if i is None or i == getattr(bt, "unk_token_id", None) else int(i)


def default_text_guide(tok, max_run: int = 2) -> TextGuide:
    """refine_guided=True: the free set is the ids of REFINE_FREE_TOKENS the tokenizer knows (names that map to the unknown id are skipped; none left is an error)"""
    ids = [i for i in (_token_id(tok, n) for n in REFINE_FREE_TOKENS) if i is not None]
    if not ids:
        raise _lib.HipBackendError(f"refine_guided=True: the tokenizer knows none of {list(REFINE_FREE_TOKENS)}; pass a TextGuide(free_ids, max_run)")
    return TextGuide(list(dict.fromkeys(ids)), max_run)


def resolve_refine_guided(value, tok) -> Optional[TextGuide]:
    """refine_guided = False / None | True | TextGuide -> the guide of the refine pass, or None"""
    if value is None or value is False:
        return None
    if value is True:
        return default_text_guide(tok)
    if isinstance(value, TextGuide):
        return value
    raise _lib.HipBackendError(f"refine_guided={value!r} (False, True or a TextGuide)")


def refine_sources(tok, input_ids, attention_mask) -> List[List[int]]:
    """The source of every row of a refine prompt, read off the prompt's own ids: the ids strictly between [Sbreak] and [Pbreak] of the row's attended tokens --
    the very tokenisation the model sees.  input_ids [B, T] or [B, T, num_vq] (left padded), attention_mask [B, T]."""
    sb, pb = _token_id(tok, "[Sbreak]"), _token_id(tok, "[Pbreak]")
    if sb is None or pb is None:
        raise _lib.HipBackendError("refine_guided: the tokenizer does not know [Sbreak] / [Pbreak]")
    ids = torch.as_tensor(input_ids).cpu()
    ids = ids[..., 0] if ids.dim() == 3 else ids
    att = torch.as_tensor(attention_mask).cpu()
    out = []
    for r in range(ids.shape[0]):
        row = ids[r][att[r] != 0].tolist()
        if sb not in row or pb not in row[row.index(sb) + 1:]:
            raise _lib.HipBackendError(f"refine_guided: row {r} of the refine prompt has no [Sbreak] ... [Pbreak] span")
        a = row.index(sb)
        out.append([int(i) for i in row[a + 1: row.index(pb, a + 1)]])
    return out


def check_refine_sources(srcs, max_new_token: int, what: str = "refine_guided") -> None:
    """by utterance: an empty sentence, or a max_new_token below the sentence's n + 1 (its tokens and [Ebreak])"""
    for u, s in enumerate(srcs):
        if len(s) < 1:
            raise _lib.HipBackendError(f"{what}: utterance {u} has no token between [Sbreak] and [Pbreak]")
        if int(max_new_token) < len(s) + 1:
            raise _lib.HipBackendError(f"{what}: utterance {u} has {len(s)} tokens and needs max_new_token >= {len(s) + 1} (its tokens and [Ebreak]); "
                                       f"params_refine_text.max_new_token is {int(max_new_token)}")


def _draw_request_seed() -> int:
    """A request's device-noise seed where the caller names none: ONE draw from torch's CPU generator (torch.manual_seed / TorchSeedContext reproduce the request)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _code_sampler_args(params: InferCodeParams, gpt):
    """What the code pass's sampler takes from an InferCodeParams: (temperature per codebook, num_code = the EOS id, logits warpers, logits processors)."""
    num_code = int(gpt.emb_code[0].num_embeddings - 1)
    warpers, processors = gen_logits(num_code=num_code, top_P=params.top_P, top_K=params.top_K, repetition_penalty=params.repetition_penalty)
    temperature = params.temperature if isinstance(params.temperature, list) else [params.temperature] * gpt.num_vq
    return temperature, num_code, warpers, processors


def _is_speaker_table(spk, n: int) -> bool:
    """Is `spk` one speaker row per utterance ([n, 768]: infer_sharded's rows, params_per_utterance's _speaker_rows) and not one speaker for the call?"""
    return torch.is_tensor(spk) and spk.dim() == 2 and spk.shape[0] == n


def _check_entries(name: str, entries, n: int, where: str = "") -> None:
    """A per-utterance list (None: not given) has one entry per utterance."""
    if entries is not None and len(entries) != n:
        raise _lib.HipBackendError(f"{name}: {len(entries)} entries for {n} utterances{where}")


@dataclass(repr=False, eq=False)
class _Request:
    """One _infer() call, resolved once (ChatTTSPlusPipeline._resolve_request): the normalised texts, the engine, and every per-call and per-utterance value
    the three paths (_infer_sliced, _infer_continuous, _infer_details) read.  The per-utterance lists are None where the caller set none."""
    texts: List[str]; gpt: object; slice_size: int
    params_refine_text: RefineTextParams; params_infer_code: InferCodeParams      # the latter after the max_new_token / spk_emb replacements of params_per_utterance
    utt_ids: list; utt_limits: Optional[list]; utt_sampling: Optional[list]; utt_prompts: Optional[list]; lora_paths: Optional[list]
    utt_voices: Optional[list]                          # per utterance (speaker tag, txt_smp, spk_smp): params_per_utterance entries with spk_smp / txt_smp (utterance_voices)
    noise_mode: object; noise_seed: Optional[int]      # "auto" | "device" | what else GPT.generate takes as `noise`; seed None: drawn by the path that runs, when it needs one
    stream: bool; use_decoder: bool; skip_refine_text: bool; refine_text_only: bool; continuous: object      # continuous: False | True | "throughput"
    n_cand: int; return_details: bool; select: Optional[Callable]; share_prompt: Optional[bool]; ids_sink: Optional[list]
    overlap_vocoder: bool; vocoder_chunk: object
    sample_rate: Optional[int] = None                   # infer(sample_rate=): the rate the waveforms leave at; None = the vocoder's own 24 kHz
    refine_guide: Optional[TextGuide] = None            # infer(refine_guided=): the refine pass's guide (resolve_refine_guided); None = free sampling, as ever
    refine_cand: int = 1                                # infer(refine_candidates=N): every text is refined N times, the best mean raw log-prob feeds the code pass
    guide_kw = property(lambda self: {} if self.refine_guide is None else dict(guide=self.refine_guide))      # _refine_text's extra keyword: none without a guide (the call as it was)
    cand_kw = property(lambda self: {} if self.refine_cand <= 1 else dict(n_cand=self.refine_cand))          # ... and none without refine candidates
    device_noise = property(lambda self: self.n_cand > 1 or self.noise_mode == "device")      # (details path) device noise whatever the slice's size

    def rows(self, idx, adapters: bool = False, params: bool = True) -> dict:
        """The generation keywords of utterances `idx` (a range or a list of indices into `texts`, in the order the rows are laid out): `utt_ids`; where the request
        has them `max_new_tokens_per_row` / `sampling_per_row` / `prompts` / `voices` / (`adapters`) `lora_paths`; `params`: the InferCodeParams, the rows of a per-utterance
        speaker table gathered.  An identity `idx` (a slice that is the whole request, the [1, 768] table of one utterance) hands the table on untouched; a range takes a view."""
        kw = dict(utt_ids=[self.utt_ids[i] for i in idx])
        for key, per_utt in (("max_new_tokens_per_row", self.utt_limits), ("sampling_per_row", self.utt_sampling), ("prompts", self.utt_prompts), ("voices", self.utt_voices),
                             ("lora_paths", self.lora_paths if adapters else None)):
            if per_utt is not None:
                kw[key] = [per_utt[i] for i in idx]
        if params:
            kw["params"], spk = self.params_infer_code, self.params_infer_code.spk_emb
            if _is_speaker_table(spk, len(self.texts)) and list(idx) != list(range(len(self.texts))):
                rows = spk[idx.start:idx.stop] if isinstance(idx, range) else spk[torch.as_tensor(list(idx), device=spk.device)]
                kw["params"] = dataclasses.replace(self.params_infer_code, spk_emb=rows)
        return kw


# -- log-probs of a generation and N-candidate ranking (infer(return_details=..., num_candidates=...); no counterpart in the reference) -----------------
CANDIDATE_SHIFT = 48        # candidate k of utterance id u draws the device noise of key u | (k << 48): candidate 0 is the plain generation


@dataclass(repr=False, eq=False)
class CandidateDetails:
    """One generated candidate of one utterance: `ids` [n, 4], `logprobs` / `sampled_logprobs` [n, 4] (GenerationOutputs), `final_logprobs` [2, 4] or None,
    `hiddens` [n, 768] or None, `mean_logprob` = the mean of `logprobs` over tokens and codebooks (-inf for a candidate with no tokens)."""
    ids: torch.Tensor
    logprobs: torch.Tensor
    sampled_logprobs: torch.Tensor
    mean_logprob: float
    final_logprobs: Optional[torch.Tensor] = None
    hiddens: Optional[torch.Tensor] = None


@dataclass(repr=False, eq=False)
class InferDetails:
    """What infer(return_details=True) yields instead of the bare list of waveforms.  Per utterance (lists in input order): `wavs`, `ids`, `logprobs`,
    `sampled_logprobs`, `mean_logprob` (the length-normalised raw score: the negative of ScoreOutputs.nll for the same tokens).  With num_candidates:
    `candidate` (the chosen index), `candidate_scores` ([N] mean log-probs) and `candidates` (the N CandidateDetails, hiddens dropped).  Where the refine-text
    pass ran: `refined_logprobs` (per utterance the raw log-probs [m] of its refined ids under the text head, the step that sampled [Ebreak] included) and
    `refined_mean_logprob` (their mean: the score refine_candidates ranks by); None when the pass was skipped."""
    wavs: list
    ids: List[torch.Tensor]
    logprobs: List[torch.Tensor]
    sampled_logprobs: List[torch.Tensor]
    mean_logprob: List[float]
    candidate: Optional[List[int]] = None
    candidate_scores: Optional[List[torch.Tensor]] = None
    candidates: Optional[List[List[CandidateDetails]]] = None
    refined_logprobs: Optional[List[torch.Tensor]] = None
    refined_mean_logprob: Optional[List[float]] = None


@dataclass(repr=False, eq=False)
class RefinedTexts:
    """What the refine pass hands on (_refine_text with log-probs or candidates): per text the winner's `ids` [n], its raw `logprobs` [m] (m = n + 1 where it
    ended by [Ebreak]: the stopping step counts) and their mean; with refine_candidates the chosen index and the [N] scores per text."""
    ids: List[torch.Tensor]
    logprobs: List[torch.Tensor]
    mean_logprob: List[float]
    candidate: Optional[List[int]] = None
    candidate_scores: Optional[List[torch.Tensor]] = None


def check_refine_candidates(refine_candidates, utt_ids, stream: bool, noise_mode, slice_size: int) -> int:
    """Validates infer(refine_candidates=N); returns N.  Each refusal is a HipBackendError that says what is refused."""
    try:
        n = int(refine_candidates)
    except (TypeError, ValueError):
        n = 0
    if n < 1 or n != refine_candidates:
        raise _lib.HipBackendError(f"refine_candidates must be an integer >= 1 (got {refine_candidates!r})")
    if n > 1:
        if stream:
            raise _lib.HipBackendError("refine_candidates > 1 needs stream=False: the refinements are ranked once all of them are complete")
        if not (isinstance(noise_mode, str) and noise_mode in ("auto", "device")):
            raise _lib.HipBackendError('refine_candidates > 1 needs device noise (noise="device" or "auto"): host noise is indexed by batch row, not keyed by utterance id')
        if n > int(slice_size):
            raise _lib.HipBackendError(f"refine_candidates={n} exceeds slice_size={slice_size}: the refinements of a text share one decode batch")
        if n >= (1 << (64 - CANDIDATE_SHIFT)):
            raise _lib.HipBackendError(f"refine_candidates must be below {1 << (64 - CANDIDATE_SHIFT)}")
        big = [int(u) for u in utt_ids if int(u) >= (1 << CANDIDATE_SHIFT) or int(u) < 0]
        if big:
            raise _lib.HipBackendError(f"refine_candidates > 1: utterance id {big[0]} is not below 2^{CANDIDATE_SHIFT} (the candidate index takes the bits above)")
    return n


def rank_refinements(ids, logprobs, final_logprobs, n_cand: int) -> RefinedTexts:
    """Rows laid out text-major ([text 0 candidate 0, text 0 candidate 1, ...]): per text the candidate with the highest length-normalised mean raw log-prob,
    the [Ebreak] step included (select_candidate's tie rule: the lowest index; a candidate without a step ranks last)."""
    raw = [torch.cat([lp.cpu().flatten(), fl[0:1].cpu().flatten()]) if fl is not None else lp.cpu().flatten() for lp, fl in zip(logprobs, final_logprobs)]
    means = [mean_logprob(r) for r in raw]
    out = RefinedTexts(ids=[], logprobs=[], mean_logprob=[], candidate=[], candidate_scores=[])
    for j in range(len(ids) // n_cand):
        sc = means[j * n_cand:(j + 1) * n_cand]
        k = select_candidate(sc)
        out.ids.append(ids[j * n_cand + k]); out.logprobs.append(raw[j * n_cand + k]); out.mean_logprob.append(sc[k])
        out.candidate.append(k); out.candidate_scores.append(torch.tensor(sc, dtype=torch.float64))
    if n_cand == 1:
        out.candidate = out.candidate_scores = None
    return out


def candidate_utt_id(utt_id: int, k: int) -> int:
    """Noise key of candidate k of utterance id `utt_id`."""
    return int(utt_id) | (int(k) << CANDIDATE_SHIFT)


def check_candidate_request(num_candidates, utt_ids, stream: bool, noise_mode) -> int:
    """Validates infer(num_candidates=N); returns N.  Each refusal is a HipBackendError that says what is refused."""
    try:
        n = int(num_candidates)
    except (TypeError, ValueError):
        n = 0
    if n < 1 or n != num_candidates:
        raise _lib.HipBackendError(f"num_candidates must be an integer >= 1 (got {num_candidates!r})")
    if n > 1:
        if stream:
            raise _lib.HipBackendError("num_candidates > 1 needs stream=False: the candidates are ranked once all of them are complete")
        if not (isinstance(noise_mode, str) and noise_mode in ("auto", "device")):
            raise _lib.HipBackendError('num_candidates > 1 needs device noise (noise="device" or "auto"): host noise is indexed by batch row, not keyed by utterance id')
        if n >= (1 << (64 - CANDIDATE_SHIFT)):
            raise _lib.HipBackendError(f"num_candidates must be below {1 << (64 - CANDIDATE_SHIFT)}")
        big = [int(u) for u in utt_ids if int(u) >= (1 << CANDIDATE_SHIFT) or int(u) < 0]
        if big:
            raise _lib.HipBackendError(f"num_candidates > 1: utterance id {big[0]} is not below 2^{CANDIDATE_SHIFT} (the candidate index takes the bits above)")
    return n


def resolve_share_prompt(share_prompt, num_candidates, batch_invariant) -> bool:
    """infer(num_candidates=N, share_prompt=...): do the N candidates of an utterance share one prompt pass (GPT.generate(prompt_of=...))?  None: exactly when the
    engine's batch_invariant option reads 1 -- there a copied KV lane is bit for bit what the candidate's own prompt pass writes, so the result is the unshared
    call's; True: in any mode (default-mode engines: same distribution, tokens may differ from the unshared schedule's); False: never.  One candidate per
    utterance has nothing to share."""
    if num_candidates is None or int(num_candidates) <= 1:
        return False
    if share_prompt is None:
        return bool(batch_invariant)
    if not isinstance(share_prompt, bool):
        raise _lib.HipBackendError(f"share_prompt must be None, True or False (got {share_prompt!r})")
    return bool(share_prompt)


def mean_logprob(logprobs: torch.Tensor) -> float:
    """Mean of [n, 4] log-probs over tokens and codebooks; -inf when there is no token."""
    return float(logprobs.double().mean()) if logprobs.numel() else float("-inf")


def select_candidate(scores) -> int:
    """The default rule: the highest mean log-prob; ties go to the lowest index; a candidate with no tokens (-inf) or a NaN score ranks last."""
    best, best_s = 0, None
    for k, v in enumerate(scores):
        v = float(v)
        v = float("-inf") if v != v else v
        if best_s is None or v > best_s:
            best, best_s = k, v
    return best


@dataclass(repr=False, eq=False)
class SessionDetails:
    """What SynthSession.poll returns per utterance instead of the bare waveform under open_session(return_details=True): one utterance's entry of InferDetails."""
    wav: torch.Tensor
    ids: torch.Tensor
    logprobs: torch.Tensor
    sampled_logprobs: torch.Tensor
    mean_logprob: float
    finished_by_eos: bool = False
    refined_text: Optional[str] = None         # sessions opened with refine=: the text the refine stage produced (what the code stage spoke); None otherwise


@dataclass(repr=False, eq=False)
class SessionChunk:
    """What SynthSession.poll returns for a streaming ticket (submit(stream=...)), zero or more times, the last one with final=True: samples
    [start, start + len(wav)) of the utterance's waveform -- float32, or int16 PCM under pcm16=True.  The chunks of a ticket are consecutive.  `details`: only on
    the final chunk of a return_details session (its `wav` is this final chunk's, not the whole utterance's)."""
    wav: torch.Tensor
    start: int
    final: bool = False
    details: Optional[SessionDetails] = None
    n_tokens: int = 0             # tokens the utterance had when the chunk was cut ("eager": the chunk is a slice of THAT prefix's waveform)
    sample_rate: int = 24000      # submit(sample_rate=): `start` and len(wav) count samples at THIS rate


class SynthSession:
    """A serving session of the pipeline (ChatTTSPlusPipeline.open_session): texts are submitted and cancelled while others are being spoken.  A
    GPT.DecodeSession (elastic decode batch, ctts_gpt_grow / ctts_gpt_cancel) under the prompt building of infer() and the batched vocoder.  Opened with
    `refine` (a RefineTextParams) a text is refined first, INSIDE the session: its refine prompt is seated as a text row beside the code rows of the one decode
    batch (DecodeSession.submit(mode="text")); when the row delivers, its ids are filtered and decoded as infer() does and the code utterance is submitted --
    both stages under the ticket submit() returned and under one utterance id (noise stream 4 for the text row, 0-3 for the code row).
    submit(stream="exact" | "eager") streams an utterance's audio while it decodes: poll() vocodes the sample windows the step made due (SessionBook) in one
    ctts_synth_windows call and returns them as SessionChunks.  "exact" emits only samples no later token can change (vocoder.settled_samples: it holds back the
    last 53 tokens' worth until the utterance ends), so the chunks concatenate to the waveform a non-streaming poll returns, bit for bit; "eager" keeps
    infer(stream=True)'s and the reference's semantics -- each chunk is a slice of the PREFIX waveform, whose last 1.1 s is computed against zero padding, so the
    concatenation is not the offline waveform and chunk boundaries carry seams.
    submit(sample_rate=) (default: open_session(sample_rate=)) delivers an utterance at another rate, resampled on the device (hip_models.Resampler): a
    non-streaming ticket's waveform after the vocoder, one ctts_resample_windows call per distinct rate of the poll; an "exact" ticket's chunks so that they
    concatenate, bit for bit, to the resampling of the offline waveform -- each settled window is vocoded as float32 from Resampler.lookback samples before
    its start (SessionWindow.v0), the outputs it settles (Resampler.out_settled) are cut from it, and PCM conversion happens after resampling.  "eager" chunks
    are slices of different prefix waveforms: no single waveform to resample, refused."""

    def __init__(self, pipe, gpt, params: InferCodeParams, use_decoder: bool, rows, seed, return_details: bool, refine: Optional[RefineTextParams] = None,
                 sample_rate: Optional[int] = None, refine_guided=False):
        self.pipe, self.gpt, self.params, self.use_decoder, self.return_details = pipe, gpt, params, bool(use_decoder), bool(return_details)
        self.refine = refine
        self.refine_guide = resolve_refine_guided(refine_guided, pipe.models_dict["tokenizer"])      # the refine stage's guide; None = free sampling
        if self.refine_guide is not None and refine is None:
            raise _lib.HipBackendError("open_session: refine_guided needs refine=RefineTextParams(...)")
        self.sample_rate = None if sample_rate is None else pipe.output_rate(sample_rate, "open_session")      # None: the vocoder's own 24 kHz
        self._rates = {}                           # code-stage ticket -> its output rate (tickets at 24 kHz are not in it)
        self._emitted = {}                         # code-stage ticket of a resampled "exact" utterance -> J, the output samples emitted so far
        temperature, num_code, warpers, processors = _code_sampler_args(params, gpt)
        text_rows = None
        if refine is not None:
            if refine.repetition_penalty is not None and float(refine.repetition_penalty) != 1.0:
                raise _lib.HipBackendError("open_session: refine.repetition_penalty must be 1 (the refine-text pass supports no repetition penalty)")
            text_rows = dict(temperature=refine.temperature, top_P=refine.top_P, top_K=refine.top_K, eos_token=pipe.models_dict["tokenizer"].eos_token,
                             max_new_token=refine.max_new_token, min_new_token=refine.min_new_token)
            if self.refine_guide is not None:
                text_rows["guide"] = self.refine_guide
        self.session = gpt.open_session(torch.tensor(temperature), num_code, params.max_new_token, min_new_token=params.min_new_token, logits_warpers=warpers,
                                        logits_processors=processors, return_hidden=self.use_decoder, return_logprobs=self.return_details, seed=seed, rows=rows,
                                        ensure_non_empty=params.ensure_non_empty, text_rows=text_rows)
        self.session.book.stream_batch, self.session.book.stream_speed = max(1, int(params.stream_batch)), max(1, int(params.stream_speed))
        self._streams = {}                         # code-stage ticket of a streaming utterance -> pcm16
        self._paths = []                           # adapters utterances of this session named: all stay resident (at most _lib.MAX_ADAPTERS)
        self._auto_id = 0
        self._refining = {}                        # public ticket (= the refine stage's) -> what the code stage needs: dict(diff, slot, utt_id)
        self._public = {}                          # code-stage ticket of a refined utterance -> its public ticket
        self._code_tk = {}                         # ... and back
        self._refined = {}                         # public ticket -> refined text
        self.failed = {}                           # public ticket -> why its code stage could not be submitted (delivered empty, cancelled=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def batch_trace(self):
        return self.session.batch_trace

    def submit(self, text: str, params=None, lora_path: Optional[str] = None, utt_id: Optional[int] = None, max_new_token: Optional[int] = None,
               refine: Optional[bool] = None, stream: Optional[str] = None, stream_batch: Optional[int] = None, pcm16: bool = False,
               sample_rate: Optional[int] = None, refine_guided: Optional[bool] = None) -> int:
        """`refine_guided` (None = as the session was opened): guide this utterance's refine stage by its own tokens (True needs a session opened with
        refine_guided=); False = it samples freely.
        `sample_rate`: this utterance's output rate in Hz (default: the session's; 24000 = the vocoder's own, today's path): with stream=None or "exact".
        `stream` "exact" or "eager": poll() returns this ticket's audio as SessionChunks while it decodes (class docstring; "exact" is the one to use unless the
        reference's windows are wanted); `stream_batch`: tokens between chunks (default: the session's params.stream_batch); `pcm16`: its chunks are int16 PCM.
        Queues one text.  `params`: this utterance's overrides (an InferCodeParams or a dict, checked by per_utterance_overrides: sampling knobs,
        max_new_token, prompt, spk_emb, or a cloned voice: spk_smp / txt_smp, e.g. ClonedVoice.overrides() -- the refine stage does not see the voice); `lora_path`: its own adapter; `utt_id`: its noise key (default: a counter).  `refine`: refine the text first (default:
        iff the session was opened with refine=); False = the text is already refined.  Returns its ticket."""
        if not isinstance(text, str):
            raise _lib.HipBackendError("SynthSession.submit takes one text (a str) per call")
        if stream not in (None, "exact", "eager"):
            raise _lib.HipBackendError(f"submit: stream={stream!r} (None, \"exact\" or \"eager\")")
        if stream is None and (stream_batch is not None or pcm16):
            raise _lib.HipBackendError("submit: stream_batch= and pcm16= belong to a streaming utterance (stream=\"exact\" | \"eager\")")
        if stream_batch is not None and int(stream_batch) < 1:
            raise _lib.HipBackendError(f"submit: stream_batch={stream_batch} (at least 1)")
        rate = self.sample_rate if sample_rate is None else self.pipe.output_rate(sample_rate, "submit")
        if rate is not None and stream == "eager":
            raise _lib.HipBackendError(f"submit: stream=\"eager\" with sample_rate={rate} is not offered: eager chunks are slices of different prefix waveforms, so "
                                       "there is no single waveform to resample (use stream=\"exact\", or resample the 24 kHz chunks yourself)")
        streaming = None if stream is None else (stream, None if stream_batch is None else int(stream_batch), bool(pcm16))
        refine = (self.refine is not None) if refine is None else bool(refine)
        if refine and self.refine is None:
            raise _lib.HipBackendError("submit: refine=True needs a session opened with refine=RefineTextParams(...)")
        pipe, gpt, base = self.pipe, self.gpt, self.params
        diff = per_utterance_overrides(base, [params])[0] if params is not None else {}
        if max_new_token is not None:
            if "max_new_token" in diff:
                raise _lib.HipBackendError("submit: max_new_token and a per-utterance params.max_new_token are exclusive")
            diff["max_new_token"] = int(max_new_token)
        if int(diff.get("max_new_token", base.max_new_token)) > base.max_new_token:
            raise _lib.HipBackendError(f"submit: max_new_token={diff['max_new_token']} exceeds the session's {base.max_new_token}")
        slot = None
        if lora_path:
            paths = list(dict.fromkeys(self._paths + [lora_path]))
            if len(paths) > _lib.MAX_ADAPTERS:
                raise _lib.HipBackendError(f"submit: {len(paths)} distinct adapters in this session; the engine holds {_lib.MAX_ADAPTERS}")
            slot = pipe._adapter_slots(gpt, paths)[paths.index(lora_path)]
            self._paths = paths
        t = pipe.normalizer(text, True, True, None)                      # infer()'s defaults
        if utt_id is None:
            utt_id, self._auto_id = self._auto_id, self._auto_id + 1
        if refine:
            # stage 1: the refine prompt as a text row (pipeline:237-277).  No per-utterance adapter: infer() refines on the base weights (_refine_text); a session
            # opened with lora_path runs on the merged engine in both stages
            input_ids, attention_mask, text_mask = pipe._refine_prompt([t], self.refine)
            guided = (self.refine_guide is not None) if refine_guided is None else bool(refine_guided)
            if guided and self.refine_guide is None:
                raise _lib.HipBackendError("submit: refine_guided=True needs a session opened with refine_guided=True | TextGuide(...)")
            src = None
            if guided:
                src = refine_sources(pipe.models_dict["tokenizer"], input_ids, attention_mask)[0]
                check_refine_sources([src], self.refine.max_new_token, "submit: refine_guided")
            emb = gpt(input_ids, text_mask)
            tk = self.session.submit(emb[0], attention_mask[0], int(utt_id), mode="text", **({} if src is None else dict(guide_src=src)))
            self._refining[tk] = dict(diff=diff, slot=slot, utt_id=int(utt_id), streaming=streaming, rate=rate)      # (the refine stage streams nothing)
            return tk
        return self._submit_code(t, diff, slot, int(utt_id), streaming, rate)

    def _submit_code(self, t: str, diff: dict, slot, utt_id: int, streaming=None, rate: Optional[int] = None) -> int:
        """the code utterance of one (refined) text: infer()'s prompt building, then DecodeSession.submit"""
        pipe, gpt, base = self.pipe, self.gpt, self.params
        t = _with_uv_break(t)
        pic = dataclasses.replace(base, spk_emb=diff["spk_emb"]) if "spk_emb" in diff else base
        voices = utterance_voices(base, [diff])            # its own cloned voice (spk_smp / txt_smp): its own tag, transcript and codes
        input_ids, attention_mask, text_mask = pipe._code_prompt([t], pic, gpt, [diff["prompt"] or ""] if "prompt" in diff else None, voices)
        if voices is not None and int(attention_mask.shape[1]) + self.session.book.max_new > self.session.book.max_seq:
            codes = 0 if voices[0][2] is None else int(codec.decode_prompt(voices[0][2]).shape[1])
            raise _lib.HipBackendError(f"submit: utterance {utt_id}: prompt of {int(attention_mask.shape[1])} tokens ({codes} of them audio-prompt codes) + "
                                       f"max_new_token={self.session.book.max_new} exceed max_seq_len={self.session.book.max_seq}")
        emb = gpt(input_ids, text_mask, spk_emb=pic.spk_emb, spk_emb_ids=pipe.models_dict["tokenizer"].spk_emb_ids)
        sampling = {k: diff[k] for k in PER_UTTERANCE_SAMPLING if k in diff} or None
        if streaming is None:
            tk = self.session.submit(emb[0], attention_mask[0], utt_id, limit=diff.get("max_new_token"), sampling=sampling, adapter_slot=slot)
            if rate is not None:
                self._rates[tk] = rate
            return tk
        tk = self.session.submit(emb[0], attention_mask[0], utt_id, limit=diff.get("max_new_token"), sampling=sampling, adapter_slot=slot, stream=streaming[0],
                                 stream_batch=streaming[1], stream_hidden=self.use_decoder,
                                 **({} if rate is None else dict(stream_lookback=self.pipe.resampler(rate).lookback)))
        self._streams[tk] = streaming[2]
        if rate is not None:
            self._rates[tk], self._emitted[tk] = rate, 0
        return tk

    def cancel(self, ticket: int) -> bool:
        """Works in either stage of a refined utterance: during the refine stage the text row is cancelled and the utterance is delivered with an empty waveform
        and cancelled=True (no code stage follows); during the code stage as for any utterance.  A refine-stage cancel answers True for every first call, also
        when the text row had already finished on the device and only its report was still on the way: the utterance is delivered empty with cancelled=True then
        too (the host decides it; no code stage is started)."""
        if ticket in self._refining:
            if self._refining[ticket].get("cancelled"):
                return False
            self._refining[ticket]["cancelled"] = True
            self.session.cancel(ticket)
            return True
        return self.session.cancel(self._code_tk.get(ticket, ticket))

    def _empty(self, cancelled: bool, refined_text=None):
        w = torch.zeros(0, device=self.pipe.device)
        if not self.return_details:
            return w
        e = torch.empty(0, self.gpt.num_vq)
        return SessionDetails(wav=w, ids=torch.empty(0, self.gpt.num_vq, dtype=torch.long, device=self.pipe.device), logprobs=e, sampled_logprobs=e.clone(),
                              mean_logprob=mean_logprob(e), finished_by_eos=False, refined_text=refined_text)

    def _vocode_windows(self, wins):
        """Every due window of the step through ctts_synth_windows: one call (one per sample format when float and int16 tickets are mixed); window ->
        (wav, start), or None for a window that yields no chunk.  A resampled ticket's window is vocoded as float32 from its v0 and goes, with the others of its
        rate (and sample format), through one ctts_resample_windows call: outputs [J, J1), J the ticket's outputs so far, J1 = out_settled(s1, final, total).
        A non-final window that settles no new output frame (J1 == J) yields nothing and is not vocoded."""
        syn = self.pipe.synth if self.use_decoder else self.pipe._codes_synth()
        hop, out, cut = syn.cfg.hop, {}, {}
        for w in wins:
            rate = self._rates.get(w.ticket)
            if rate is None:
                continue
            rs, J = self.pipe.resampler(rate), self._emitted[w.ticket]
            J1 = rs.out_settled(w.s1, w.final, prefix_samples(w.n_tokens))
            cut[id(w)] = (rs, J, max(J1, J))
            if w.final:
                self._emitted.pop(w.ticket)
            else:
                self._emitted[w.ticket] = max(J1, J)
            if J1 <= J:
                pcm = self._streams.get(w.ticket, False)
                out[id(w)] = (torch.zeros(0, dtype=torch.int16 if pcm else torch.float32, device=self.pipe.device), J) if w.final else None
        for pcm in (False, True):
            sel = [w for w in wins if id(w) not in out and (id(w) in cut and not pcm or id(w) not in cut and self._streams.get(w.ticket, False) == pcm)]
            if not sel:
                continue
            wavs = syn.synth_windows([(w.hiddens if self.use_decoder else w.ids) for w in sel], [w.v0 - 2 * w.tok0 * hop for w in sel], [w.s1 - w.v0 for w in sel], pcm)
            for w, v in zip(sel, wavs):
                if id(w) in cut:
                    cut[id(w)] += (v,)
                else:
                    out[id(w)] = (v, w.s0)
        todo = [w for w in wins if id(w) in cut and id(w) not in out]
        for rs, pcm in dict.fromkeys((cut[id(w)][0], self._streams.get(w.ticket, False)) for w in todo):
            sel = [w for w in todo if cut[id(w)][0] is rs and self._streams.get(w.ticket, False) == pcm]
            res = rs.resample_windows([cut[id(w)][3] for w in sel], [w.v0 for w in sel], [prefix_samples(w.n_tokens) if w.final else None for w in sel],
                                      [cut[id(w)][1] for w in sel], [cut[id(w)][2] - cut[id(w)][1] for w in sel], pcm)
            out.update({id(w): (v, cut[id(w)][1]) for w, v in zip(sel, res)})
        return out

    def _deliver(self, results, wins=()):
        tok = self.pipe.models_dict["tokenizer"]
        out, code = [], []
        wav_of_win = self._vocode_windows(wins) if wins else {}
        final_of = {}
        for w in wins:
            if w.final:
                final_of[w.ticket] = w
            elif wav_of_win[id(w)] is not None:
                wav, start = wav_of_win[id(w)]
                out.append((self._public.get(w.ticket, w.ticket),
                            SessionChunk(wav=wav, start=start, final=False, n_tokens=w.n_tokens, sample_rate=self._rates.get(w.ticket, NATIVE_RATE)), False))
        for r in results:
            if getattr(r, "mode", "code") != "text":
                code.append(r)
                continue
            # a refine stage ended: cancelled -> the utterance ends here; else filter and decode its ids exactly as infer() does and start the code stage
            info = self._refining.pop(r.ticket)
            if r.cancelled or info.get("cancelled"):
                e = self._empty(True)
                out.append((r.ticket, self._end_chunk(e, info.get("streaming"), info.get("rate")), True))
                continue
            text = _decode_refined(tok, [r.ids])[0]
            try:
                tk2 = self._submit_code(text, info["diff"], info["slot"], info["utt_id"], info.get("streaming"), info.get("rate"))
            except _lib.HipBackendError as e:
                # the code stage was refused (a refined text whose prompt no longer fits max_seq_len, ...): this utterance ends here, delivered like a cancelled
                # one with the reason on record; the other results of the step are not lost
                self.failed[r.ticket] = str(e)
                out.append((r.ticket, self._end_chunk(self._empty(True, refined_text=text), info.get("streaming"), info.get("rate")), True))
                continue
            self._public[tk2], self._code_tk[r.ticket], self._refined[r.ticket] = r.ticket, tk2, text
        spoken = [r for r in code if r.ids.shape[0] > 0 and r.ticket not in self._streams]      # (a streaming ticket's audio left as windows)
        wavs = self.pipe._decode_to_wavs([(r.hiddens if self.use_decoder else r.ids) for r in spoken], self.use_decoder) if spoken else []
        wav_of = {r.ticket: w for r, w in zip(spoken, wavs)}
        for rate in dict.fromkeys(self._rates[r.ticket] for r in spoken if r.ticket in self._rates):      # one resample call per distinct rate of the poll
            tks = [r.ticket for r in spoken if self._rates.get(r.ticket) == rate]
            wav_of.update(zip(tks, self.pipe.resampler(rate).resample([wav_of[tk] for tk in tks])))
        for r in code:
            pub = self._public.pop(r.ticket, r.ticket)
            self._code_tk.pop(pub, None)
            refined = self._refined.pop(pub, None)
            w = wav_of.get(r.ticket)
            fw = final_of.get(r.ticket)
            rate = self._rates.pop(r.ticket, NATIVE_RATE)
            if fw is not None:
                w, start = wav_of_win[id(fw)]
            if w is None:
                w = torch.zeros(0, device=self.pipe.device)
            if self.return_details:
                w = SessionDetails(wav=w, ids=r.ids, logprobs=r.logprobs.cpu(), sampled_logprobs=r.sampled_logprobs.cpu(), mean_logprob=mean_logprob(r.logprobs.cpu()),
                                   finished_by_eos=r.finished_by_eos, refined_text=refined)
            if fw is not None:
                self._streams.pop(r.ticket, None)
                w = SessionChunk(wav=w.wav if self.return_details else w, start=start, final=True, details=w if self.return_details else None, n_tokens=fw.n_tokens,
                                 sample_rate=rate)
            out.append((pub, w, r.cancelled))
        return out

    def _end_chunk(self, empty, streaming, rate=None):
        """how an utterance that ends in its refine stage is delivered: a streaming ticket gets its (empty) final chunk"""
        if streaming is None:
            return empty
        wav = torch.zeros(0, dtype=torch.int16 if streaming[2] else torch.float32, device=self.pipe.device)
        return SessionChunk(wav=wav, start=0, final=True, details=empty if self.return_details else None, sample_rate=rate or NATIVE_RATE)

    @torch.no_grad()
    def poll(self):
        """One DecodeSession.step(); what finished is vocoded in one batch.  Returns [(ticket, wav or SessionDetails, cancelled)]: a cancelled utterance with at
        least one token is vocoded, one with none yields an empty waveform.  A refine stage that ended is not returned: its code stage is submitted instead.
        A streaming ticket (submit(stream=...)) appears as (ticket, SessionChunk, cancelled) zero or more times, the last one with final=True; every window
        the step made due is vocoded in one ctts_synth_windows call, right behind the step's decode launches on the same stream."""
        results = self.session.step()
        return self._deliver(results, self.session.take_windows() if self._streams else ())      # (no streaming ticket in flight: nothing can be due)

    def drain(self):
        out = []
        while not self.session.book.idle():
            out += self.poll()
        return out

    def close(self) -> None:
        self.session.close()


def _get(cfg, key, default=None):
    try:
        return cfg[key]
    except Exception:
        return getattr(cfg, key, default)


def load_config(path: str) -> dict:
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def load_lora_adapter(path: str, hidden_size: int = 768, intermediate_size: int = 3072):
    """peft adapter directory -> [(layer, target, A[r,in], B[out,r], scale)] (pipeline:420-432; train config
    configs/train/train_voice_clone_lora.yaml:72-83: r=8, alpha=16 on q/k/v/o, with gate / up / down as the commented-out candidates).  Reads
    adapter_config.json + adapter_model.safetensors directly; peft is not needed.  The seven targets of the decoder layers are served (`self_attn.{q,k,v,o}_proj`,
    `mlp.{gate,up,down}_proj`); any other tensor in the file (`lora_embedding_A` / `_B`, `modules_to_save` copies, heads) is an error that names the key and the file, and so is an A / B pair
    whose shapes do not fit its target.  Config: `r` and `lora_alpha` default to 8 as in peft's LoraConfig; `use_rslora` gives scale = alpha / sqrt(r);
    `use_dora` is refused (its merge rule is not W + scale * B A).  The file layout itself is not pinned against peft (not available offline): pinned algebraically only."""
    from safetensors.numpy import load_file
    cfg_path = os.path.join(path, "adapter_config.json")
    with open(cfg_path) as f:
        ac = json.load(f)
    if ac.get("use_dora", False):
        raise ValueError(f"{cfg_path}: use_dora adapters are not supported (DoRA's merge is not W + scale * B A; merging it as LoRA would be silently wrong)")
    r = int(ac.get("r", 8))
    alpha = float(ac.get("lora_alpha", 8))
    scale = alpha / math.sqrt(r) if ac.get("use_rslora", False) else alpha / float(r)
    st_path = os.path.join(path, "adapter_model.safetensors")
    sd = load_file(st_path)
    out = []

    def parse(k):
        """(layer, target, 'lora_A' | 'lora_B') of `...layers.N.{self_attn,mlp}.TARGET.lora_{A,B}[.adapter_name].weight`, else None."""
        parts = k.split(".")
        if "layers" not in parts:
            return None
        li = parts.index("layers")
        if len(parts) < li + 6 or not parts[li + 1].isdigit() or LORA_TARGETS.get(parts[li + 3]) != parts[li + 2]:
            return None
        if parts[li + 4] not in ("lora_A", "lora_B") or parts[-1] != "weight" or len(parts) > li + 7:
            return None
        return int(parts[li + 1]), parts[li + 3], parts[li + 4]
    for k in sd:        # every tensor of the file must be one this backend applies: anything else (lora_embedding_A / _B, modules_to_save copies, heads, DoRA magnitudes) would be dropped silently
        if parse(k) is None:
            raise ValueError(f"{st_path}: key '{k}' is not a lora_A / lora_B matrix of a decoder layer's {' '.join(LORA_TARGETS)} (embeddings, heads and modules_to_save are not served)")
    for k, A in sd.items():
        layer, target, which = parse(k)
        if which != "lora_A":
            if k.replace("lora_B", "lora_A") not in sd:
                raise ValueError(f"{st_path}: key '{k}' has no '{k.replace('lora_B', 'lora_A')}'")
            continue
        Bk = k.replace("lora_A", "lora_B")
        if Bk not in sd:
            raise ValueError(f"{st_path}: key '{k}' has no '{Bk}'")
        A = np.asarray(A, dtype=np.float32); Bm = np.asarray(sd[Bk], dtype=np.float32)
        check_lora_shapes(layer, target, A, Bm, hidden_size, intermediate_size, where=f" {st_path} (key '{k}')")
        if A.shape[0] != r and "r" in ac:
            raise ValueError(f"{st_path}: key '{k}' has rank {A.shape[0]}, adapter_config.json says r = {r} (rank_pattern is not supported)")
        out.append((layer, target, A, Bm, scale))
    return out


def merge_short_sentences(pieces: List[str], min_len: int = 30) -> List[str]:
    """The merge step of the reference's text optimisation (pipeline:353-377), after whatever splitter produced `pieces`: sentences
    shorter than `min_len` characters are chained with " [uv_break] " until the chain exceeds `min_len`; a long sentence absorbs the
    chain in front of it; a left-over chain becomes its own utterance if long enough (or if nothing else exists), else it is
    appended to the last utterance.  CPU text work in front of the hot path -- kept because it decides the batch the path sees."""
    out: List[str] = []
    chain = ""
    for piece in pieces:
        if len(piece) < min_len:
            chain += f"{piece} [uv_break] "
            if len(chain) > min_len:
                out.append(chain)
                chain = ""
        else:
            out.append(chain + piece)
            chain = ""
    if len(chain) > min_len or not out:
        out.append(chain)
    elif chain:
        out[-1] += f" [uv_break] {chain}"
    return out


class ChatTTSPlusPipeline:
    def __init__(self, cfg, **kwargs):
        self.logger = logging.getLogger(self.__class__.__name__)
        self.cfg = cfg
        self.device = torch.device(kwargs.get("device", "cuda"))
        self.dtype = torch.float32                 # activations / outputs are fp32; weights per `weight_dtype`
        # CPU text front-end in front of the path (pipeline:147-155,353-388): `normalizer(text, do_text_normalization,
        # do_homophone_replacement, lang)` and `text_splitter(lines) -> sentences`; both replaceable, `text_splitter=None` keeps the
        # input lines as they are.  Defaults: text_frontend.Normalizer over <checkpoint_dir>/homophones_map.json and text_frontend.split_text
        self.normalizer: Optional[Callable] = kwargs.get("normalizer")
        self.text_splitter: Optional[Callable] = kwargs.get("text_splitter", text_frontend.split_text)
        self.load_lora = False
        self._lora_models = OrderedDict()          # lora_path -> merged sibling engine, LRU-bounded (`lora_cache`, default 1)
        self._lora_cache = max(1, int(kwargs.get("lora_cache", 1)))
        self.load_models(**kwargs)

    @classmethod
    def from_components(cls, gpt, synth, tokenizer, device, normalizer=None, text_splitter=None):
        """A pipeline around engines that are already loaded (bench.py's sharded-request leg, services that build their engines themselves):
        the same infer() / infer_sharded() surface without the checkpoint-directory pass of load_models.  No zero-shot encoder, no use_decoder=False."""
        self = object.__new__(cls)
        self.logger = logging.getLogger(cls.__name__)
        self.cfg = None
        self.device = torch.device(device)
        self.dtype = torch.float32
        self.normalizer = normalizer if normalizer is not None else text_frontend.Normalizer(None)
        self.text_splitter = text_splitter
        self.load_lora = False
        self._lora_models = OrderedDict()
        self._lora_cache = 1
        self.models_dict = dict(gpt=gpt, tokenizer=tokenizer)
        self.synth = synth
        self.std = self.mean = None
        self.infer_type = "hip"
        return self

    # -- loading (pipeline:53-155) -----------------------------------------------------------------
    def load_models(self, **kwargs):
        self.models_dict = {}
        models = _get(self.cfg, "MODELS")
        coef = kwargs.get("coef", None)
        if coef is None:
            coef = codec.coef_to_string(torch.rand(100).numpy())            # pipeline:56-59
        self.dave_coef = coef
        ckpt_dir = kwargs.get("checkpoint_dir") or os.environ.get("CHATTTS_PLUS_CHECKPOINT_DIR", "checkpoints")
        self.infer_type = None
        synth = None
        for model_name in models:
            m = models[model_name]
            kw = dict(_get(m, "kwargs") or {})
            mp = kw.get("model_path")
            if mp and not os.path.isabs(mp):
                kw["model_path"] = os.path.join(ckpt_dir, mp.replace("checkpoints/", ""))   # pipeline:70-71
            itype = _get(m, "infer_type")
            if model_name == "tokenizer":
                tok = kwargs.get("tokenizer")
                if tok is None:
                    from .tokenizer import Tokenizer
                    tok = Tokenizer(**kw)
                self.models_dict[model_name] = tok
                continue
            if model_name == "dvae_encode":                 # zero-shot speaker prompt (pipeline:279-284): optional checkpoint
                if itype == "hip" and kw.get("model_path") and os.path.exists(kw["model_path"]):
                    # the same checkpoint's decoder + quantiser serve use_decoder=False (pipeline:292): built on first use (_codes_synth)
                    self._full_ckpt = dict(path=kw["model_path"], decoder_config=dict(kw.get("decoder_config") or {}), vq_config=dict(kw.get("vq_config") or {}))
                    path = kw.pop("model_path")
                    enc = hip_models.DVAEEncoder(device=str(self.device), **kw)
                    sd = dict(torch.load(path, weights_only=True, mmap=True))
                    if "coef" not in sd:
                        sd["coef"] = torch.from_numpy(codec.coef_from_string(coef)).view(1, -1, 1)
                    self.models_dict[model_name] = enc.load_state_dict(sd)
                continue
            if itype != "hip":
                raise _lib.HipBackendError(f"model {model_name}: infer_type={itype!r}; this pipeline serves infer_type 'hip' only")
            self.infer_type = self.infer_type or itype
            if model_name in ("dvae_decode", "vocos") and synth is None:
                dk = dict(_get(models["dvae_decode"], "kwargs"))
                vk = dict(_get(models["vocos"], "kwargs"))
                dcfg = dict(dk["decoder_config"]); dcfg["n_mels"] = 100
                vcfg = dict(vk["backbone_config"]); vcfg.update(vk["head_config"])
                synth = hip_models.Synth(dcfg, vcfg, max_frames=int(kwargs.get("max_frames", 2 * 2048 + 64)), device=self.device,
                                         max_batch=int(kwargs.get("vocoder_batch", 32)))
                self.synth = synth
            if model_name == "vocos":                       # pipeline:93-111
                model_ = hip_models.Vocos(synth)
                model_.load_state_dict(torch.load(kw["model_path"], weights_only=True, mmap=True))
                self._vocos_ckpt = dict(path=kw["model_path"], cfg=vcfg)
            elif model_name == "dvae_decode":
                kw["coef"] = coef
                path = kw.pop("model_path")
                model_ = hip_models.DVAE(synth=synth, **kw)
                sd = dict(torch.load(path, weights_only=True, mmap=True))
                if "coef" not in sd:                        # the buffer is persistent: a checkpoint value wins (dvae.py:222,241-247)
                    sd["coef"] = torch.from_numpy(codec.coef_from_string(coef)).view(1, -1, 1)
                model_.load_state_dict(sd)
            else:
                kw.setdefault("device", str(self.device))
                model_ = getattr(hip_models, _get(m, "name"))(**kw)          # pipeline:113-129 dispatch
            self.models_dict[model_name] = model_.eval().to(self.device)
        spk_stat_path = os.path.join(ckpt_dir, "asset/spk_stat.pt")
        if os.path.exists(spk_stat_path):                   # pipeline:131-145
            spk_stat = torch.load(spk_stat_path, weights_only=True, mmap=True).to(self.device, dtype=self.dtype)
            self.std, self.mean = spk_stat.chunk(2)
        else:
            self.std = self.mean = None
        if self.normalizer is None:                         # pipeline:147-155 (the reference downloads the map when it is missing)
            map_path = os.path.join(ckpt_dir, "homophones_map.json")
            if not os.path.exists(map_path):
                self.logger.warning("%s not found: homophone replacement is off", map_path)
                map_path = None
            self.normalizer = text_frontend.Normalizer(map_path)

    # -- speakers (pipeline:306-331) ---------------------------------------------------------------
    @torch.inference_mode()
    def sample_audio_speaker(self, wav) -> str:
        """pipeline:279-284: 24 kHz mono waveform -> base16384 audio-prompt string (`spk_smp`)."""
        enc = self.models_dict.get("dvae_encode")
        if enc is None:
            raise _lib.HipBackendError("zero-shot speaker needs the dvae_encode checkpoint (DVAE_full.pt) configured with infer_type 'hip'")
        wav = torch.as_tensor(wav, dtype=torch.float32)
        codes = encode_clips(enc, [wav.view(-1)])[0]            # the entry clone_voices batches over, with B = 1
        return codec.encode_prompt(codes)

    @staticmethod
    def _load_clip(path, wav=None, sample_rate=None) -> torch.Tensor:
        """A reference clip as infer(speaker_audio_path=) prepares it (pipeline:486-496): read (or taken as [n] / [channels, n] samples at `sample_rate`),
        resampled to 24 kHz, channels averaged -> [n] fp32."""
        from . import audio
        if wav is None:
            wav, sample_rate = audio.load_audio(path)
        wav = torch.as_tensor(wav, dtype=torch.float32)
        wav = wav.view(1, -1) if wav.dim() == 1 else wav
        return torch.mean(audio.resample(wav, int(sample_rate or 24000), 24000), 0)

    @torch.inference_mode()
    def clone_voices(self, clips, texts, sample_rates=None) -> List[ClonedVoice]:
        """One ClonedVoice per reference clip, all clips through ONE encoder call (DVAEEncoder.encode_batch; the reference can clone one voice per infer call,
        pipeline:486-499).  `clips`: paths, or waveforms ([n] or [channels, n]; `sample_rates`: one rate for all or one per clip, default 24000 -- ignored for
        paths, whose files name their own); each is resampled and mono-mixed exactly as infer(speaker_audio_path=) does.  `texts`: the transcript of each clip
        (txt_smp).  Voice i equals ClonedVoice(sample_audio_speaker(clip i), texts[i]), string for string."""
        enc = self.models_dict.get("dvae_encode")
        if enc is None:
            raise _lib.HipBackendError("zero-shot speaker needs the dvae_encode checkpoint (DVAE_full.pt) configured with infer_type 'hip'")
        clips, texts = list(clips), list(texts)
        if len(clips) != len(texts):
            raise _lib.HipBackendError(f"clone_voices: {len(texts)} transcripts for {len(clips)} clips")
        rates = list(sample_rates) if isinstance(sample_rates, (list, tuple)) else [sample_rates] * len(clips)
        _check_entries("sample_rates", rates, len(clips))
        wavs = []
        for c, r in zip(clips, rates):
            if isinstance(c, (str, os.PathLike)):
                if not os.path.exists(c):
                    raise _lib.HipBackendError(f"clone_voices: clip {os.fspath(c)!r} does not exist")
                wavs.append(self._load_clip(os.fspath(c)))
            else:
                wavs.append(self._load_clip(None, c, r))
        if not wavs:
            return []
        codes = encode_clips(enc, wavs)
        return [ClonedVoice(spk_smp=codec.encode_prompt(c), txt_smp=t or "", _codes=c.to(torch.int64)) for c, t in zip(codes, texts)]

    def sample_random_speaker(self) -> str:
        return self._encode_spk_emb(self._sample_random_speaker())

    @staticmethod
    def _encode_spk_emb(spk_emb: torch.Tensor) -> str:
        return codec.encode_spk_emb(spk_emb)

    def _sample_random_speaker(self) -> torch.Tensor:
        if self.std is None:
            raise _lib.HipBackendError("spk_stat.pt not loaded: pass a speaker embedding explicitly")
        dim = self.std.shape[-1]
        return torch.randn(dim, device=self.std.device, dtype=self.std.dtype).mul_(self.std).add_(self.mean)

    # -- hot path callers --------------------------------------------------------------------------
    def _code_prompt(self, text, params: InferCodeParams, gpt, prompts=None, voices=None):
        """The code-generation prompt of pipeline:157-235 (shared by _infer_code and score): "[Stts]{spk tag}{txt_smp}{prompt}{text}[Ptts]", tokenised
        with the zero-shot audio prompt (spk_smp) after the text.  Returns input_ids [B, T, 4], attention_mask, text_mask (left padded).
        `voices`: one (spk tag, txt_smp, spk_smp) per text instead of the params' (utterance_voices): every row its own tag, transcript and codes."""
        tok = self.models_dict["tokenizer"]
        if not isinstance(text, list):
            text = [text]
        assert len(text), "text should not be empty"
        text = [t.replace("[Stts]", "").replace("[spk_emb]", "").replace("[empty_spk]", "").strip() for t in text]
        if prompts is not None:
            text = [p + i for p, i in zip(prompts, text)]
        elif params.prompt:
            text = [params.prompt + i for i in text]
        if voices is not None:
            text = [f"[Stts]{tag}{txt_smp}{i}[Ptts]" for (tag, txt_smp, _), i in zip(voices, text)]
            return tok.encode(text, gpt.num_vq, prompt_str=[smp for _, _, smp in voices], device=self.device)
        txt_smp = "" if params.txt_smp is None else params.txt_smp
        tag = "[spk_emb]" if params.spk_emb is not None else "[empty_spk]"
        text = [f"[Stts]{tag}{txt_smp}{i}[Ptts]" for i in text]
        return tok.encode(text, gpt.num_vq, prompt_str=params.spk_smp, device=self.device)

    @torch.no_grad()
    def score(self, text, codes=None, wavs=None, params_infer_code: Optional[InferCodeParams] = None, append_eos: bool = True,
              lora_path: Optional[str] = None, lora_paths: Optional[List[Optional[str]]] = None):
        """Teacher-forced scoring of audio codes under the code GPT (no counterpart in the reference's pipeline; the evaluation of train_lora.py:430-469):
        the prompt is built exactly as _infer_code builds it, utterance i's codes [n_i, 4] follow it, and GPT.score returns each code's log-probability
        and argmax under the raw heads (hip_models.gpt.ScoreOutputs: per utterance logprob / argmax / nll / seq_accuracy, token-weighted loss / accuracy).
          codes   one [n_i, 4] code array per text (e.g. GenerationOutputs.ids of a generate() call: re-scoring costs one prompt pass), or
          wavs    one 24 kHz mono waveform per text, encoded by the dvae_encode model along the path of sample_audio_speaker -- with (text, audio) pairs
                  this gives train_lora's validation metrics
          append_eos  the targets end with EOS on all 4 codebooks (train_lora.py:401-404); False scores the codes only
          lora_path   one merged adapter for the call (the engine infer() uses for it); lora_paths: one adapter directory (or None) per utterance,
                  through the engine's resident slots (_adapter_slots)
        train_lora's prompts carry no "[speed_5]" prefix (datasets/base_dataset.py:113-115): InferCodeParams(prompt="") reproduces them."""
        params = params_infer_code if params_infer_code is not None else InferCodeParams()
        texts = text if isinstance(text, list) else [text]
        if (codes is None) == (wavs is None):
            raise ValueError("score: pass exactly one of codes= and wavs=")
        if codes is None:
            enc = self.models_dict.get("dvae_encode")
            if enc is None:
                raise _lib.HipBackendError("score(wavs=...) needs the dvae_encode checkpoint (DVAE_full.pt) configured with infer_type 'hip'")
            clips = [torch.as_tensor(w, dtype=torch.float32).view(-1) for w in (wavs if isinstance(wavs, list) else [wavs])]
            codes = [c.t() for c in encode_clips(enc, clips, "score: waveform")] if clips else []      # one encoder call; [4, n] (sample_audio_speaker) -> [n, 4]
        elif not isinstance(codes, list):
            codes = [codes]
        if len(codes) != len(texts):
            raise ValueError(f"score: {len(codes)} code sequences / waveforms for {len(texts)} texts")
        if lora_path and lora_paths:
            raise ValueError("score: pass lora_path (one merged adapter) or lora_paths (one per utterance), not both")
        gpt = self._gpt_for_lora(lora_path)
        tok = self.models_dict["tokenizer"]
        input_ids, attention_mask, text_mask = self._code_prompt(texts, params, gpt)
        eos = int(gpt.emb_code[0].num_embeddings - 1)
        si = hip_models.gpt.score_inputs(input_ids, attention_mask, text_mask, codes, eos, append_eos=append_eos)
        emb = gpt(si["ids"], si["text_mask"], spk_emb=params.spk_emb, spk_emb_ids=tok.spk_emb_ids)
        if lora_paths is not None:
            if len(lora_paths) != len(texts):
                raise ValueError(f"score: {len(lora_paths)} lora_paths for {len(texts)} texts")
            gpt.set_row_adapters(self._adapter_slots(gpt, lora_paths))
        try:
            return gpt.score(emb, si["mask"], si["targets"], si["n_targets"])
        finally:
            if lora_paths is not None:
                gpt.set_row_adapters(None)

    @torch.no_grad()
    def score_text(self, text, refined, params_refine_text: Optional[RefineTextParams] = None, lora_path: Optional[str] = None):
        """Teacher-forced scoring of refined texts under the refine-text head (the text twin of score(); no counterpart in the reference): the prompt of every
        text is built exactly as the refine pass builds it ("[Sbreak]{text}[Pbreak]{prompt}"), `refined[i]` follows it -- a string (tokenised without special
        tokens, as the tokenizer decodes the pass's output) or a sequence of text ids -- then [Ebreak], and GPT.score_text returns each token's log-probability
        and argmax under the raw text head (ScoreOutputs: logprob[i] / argmax[i] are [n_i + 1]; -nll[i] is the score refine_candidates ranks by).  `text` is
        taken as given (infer() normalises its texts before it refines them).  `lora_path`: one merged adapter for the call."""
        params = params_refine_text if params_refine_text is not None else RefineTextParams()
        texts = text if isinstance(text, list) else [text]
        refined = refined if isinstance(refined, list) and (len(refined) == 0 or isinstance(refined[0], (str, list, tuple, torch.Tensor))) else [refined]
        if len(refined) != len(texts):
            raise ValueError(f"score_text: {len(refined)} refined sequences for {len(texts)} texts")
        gpt = self._gpt_for_lora(lora_path)
        tok = self.models_dict["tokenizer"]
        ids = [torch.as_tensor(tok._tokenizer(r, add_special_tokens=False)["input_ids"] if isinstance(r, str) else r, dtype=torch.long).flatten() for r in refined]
        input_ids, attention_mask, _ = self._refine_prompt(texts, params)
        si = hip_models.gpt.score_text_inputs(input_ids, attention_mask, ids, int(tok.eos_token))
        return gpt.score_text(gpt(si["ids"], si["text_mask"]), si["mask"], si["targets"], si["n_targets"])

    @torch.no_grad()
    def _infer_code(self, text, stream: bool, return_hidden: bool, params: InferCodeParams, gpt=None, prompts=None, voices=None, **gen_kwargs):
        """pipeline:157-235 -- same argument plumbing; the GPT object is the hip backend.  `gen_kwargs` (noise, seed, utt_ids, sampling_per_row) ride
        through to GPT.generate: the device noise stream of an utterance is keyed by the request seed and its global utterance id.  `prompts`: one
        prompt prefix per text instead of params.prompt (params_per_utterance); `voices`: one (spk tag, txt_smp, spk_smp) per text (_code_prompt)."""
        gpt = gpt or self.models_dict["gpt"]
        tok = self.models_dict["tokenizer"]
        input_ids, attention_mask, text_mask = self._code_prompt(text, params, gpt, prompts, voices)
        if voices is not None:
            # an audio prompt can be long: text + codes + the utterance's token limit must fit a KV lane -- refused here, before the engine begins, by utterance
            limits, prompt_of = gen_kwargs.get("max_new_tokens_per_row"), gen_kwargs.get("prompt_of")
            for r, n in enumerate(attention_mask.sum(1).tolist()):
                rows_r = [r] if prompt_of is None else [j for j, p in enumerate(prompt_of) if p == r]      # (shared prompt passes: the rows that decode from prompt r)
                lim = max(int(limits[j]) for j in rows_r) if limits is not None else int(params.max_new_token)
                if n + lim > gpt.max_seq:
                    codes = 0 if voices[r][2] is None else int(codec.decode_prompt(voices[r][2]).shape[1])
                    raise _lib.HipBackendError(f"utterance {r} of this batch: prompt of {int(n)} tokens ({codes} of them audio-prompt codes) + max_new_token={lim} "
                                               f"exceed max_seq_len={gpt.max_seq}")
        emb = gpt(input_ids, text_mask, spk_emb=params.spk_emb, spk_emb_ids=tok.spk_emb_ids)     # get_emb + apply_spk_emb, one launch
        temperature, num_code, warpers, processors = _code_sampler_args(params, gpt)
        gen_kwargs.update(temperature=torch.tensor(temperature), eos_token=num_code, attention_mask=attention_mask, max_new_token=params.max_new_token,
                          min_new_token=params.min_new_token, logits_warpers=warpers, logits_processors=processors, return_hidden=return_hidden,
                          ensure_non_empty=params.ensure_non_empty)
        if gen_kwargs.pop("continuous", False):
            # more utterances than decode rows: queued utterances take over rows as they free up (GPT.generate_many_iter: a generator of
            # completion events whose return value is the GenerationOutputs of all utterances)
            gen_kwargs.pop("noise", None)
            return gpt.generate_many_iter(emb, input_ids, **gen_kwargs)
        return gpt.generate(emb, input_ids, infer_text=False, stream=stream, show_tqdm=params.show_tqdm, stream_batch=params.stream_batch, **gen_kwargs)

    def _refine_prompt(self, text, params: RefineTextParams):
        """The refine-text prompt of pipeline:237-277 (shared by _refine_text and SynthSession): "[Sbreak]{text}[Pbreak]{prompt}", tokenised.  Returns input_ids
        [B, T, 4], attention_mask, text_mask (left padded)."""
        gpt, tok = self.models_dict["gpt"], self.models_dict["tokenizer"]
        return tok.encode([f"[Sbreak]{i}[Pbreak]{params.prompt}" for i in text], gpt.num_vq, device=self.device)

    @torch.no_grad()
    def _refine_text(self, text, params: RefineTextParams, continuous_rows: int = 0, seed=None, utt_ids=None, guide: Optional[TextGuide] = None, n_cand: int = 1,
                     want_logprobs: bool = False, gpt=None):
        """pipeline:237-277: "[Sbreak]{text}[Pbreak]{prompt}" -> GPT.generate(infer_text=True) on the 21178-way text head.
        `continuous_rows` > 0 (no counterpart in the reference, which refines slice by slice): all sentences of the request through that many decode
        rows with row re-use (GPT.generate_many, device noise keyed by utterance id: a sentence's refined text does not depend on its neighbours).
        `guide` (refine_guided=): every sentence is guided by its own tokens, read off the refine prompt (refine_sources).
        `want_logprobs` / `n_cand` > 1 (return_details, refine_candidates=N): the call returns a RefinedTexts instead of the GenerationOutputs -- the pass runs with
        return_text_logprobs; with N candidates every text is laid out N times as ordinary text rows under the utterance ids candidate_utt_id(u, k) (candidate 0
        is the plain refinement), device noise keyed by `seed`, through `continuous_rows` rows with row re-use, and rank_refinements picks the winners.  With a
        guide every candidate holds the source tokens: the ranking chooses among the insertions.  No prompt pass is shared (ctts_gpt_share_prompts refuses infer_text)."""
        gpt, tok = gpt or self.models_dict["gpt"], self.models_dict["tokenizer"]
        want_logprobs = want_logprobs or getattr(self, "_refine_details", False)      # (_infer_details with return_details)
        input_ids, attention_mask, text_mask = self._refine_prompt(text, params)
        if n_cand > 1:
            rep = torch.arange(len(text), device=input_ids.device).repeat_interleave(n_cand)
            input_ids, attention_mask, text_mask = input_ids[rep], attention_mask[rep], text_mask[rep]
            utt_ids = [candidate_utt_id(u, k) for u in (utt_ids if utt_ids is not None else range(len(text))) for k in range(n_cand)]
        gkw = {}
        if guide is not None:
            srcs = refine_sources(tok, input_ids, attention_mask)
            check_refine_sources(srcs, params.max_new_token)
            gkw = dict(text_guide=guide, guide_src=srcs)
        if want_logprobs or n_cand > 1:
            gkw["return_text_logprobs"] = True
        warpers, processors = gen_logits(num_code=tok.len, top_P=params.top_P, top_K=params.top_K, repetition_penalty=params.repetition_penalty)
        emb = gpt(input_ids, text_mask)
        kw = dict(temperature=torch.tensor([params.temperature]), eos_token=tok.eos_token, attention_mask=attention_mask, max_new_token=params.max_new_token,
                  min_new_token=params.min_new_token, logits_warpers=warpers, logits_processors=processors, ensure_non_empty=params.ensure_non_empty, infer_text=True)
        if continuous_rows > 0:
            res = gpt.generate_many(emb, input_ids, seed=seed, utt_ids=utt_ids, rows=continuous_rows, **kw, **gkw)
        else:
            res = next(gpt.generate(emb, input_ids, stream=False, show_tqdm=params.show_tqdm, **kw, **gkw))
        if not (want_logprobs or n_cand > 1):
            return res
        return rank_refinements(res.ids, res.logprobs, res.final_logprobs, n_cand)

    def _codes_synth(self):
        """The "decode codes" model of use_decoder=False (pipeline:292: decoder = models_dict["dvae_encode"], i.e. the DVAE_full checkpoint
        run in decode mode on the generated ids, dvae.py:272-291): its decoder stack + the quantiser's project_out + a second copy of the
        Vocos weights in one native handle, created on first use."""
        if getattr(self, "synth_codes", None) is not None:
            return self.synth_codes
        full, voc = getattr(self, "_full_ckpt", None), getattr(self, "_vocos_ckpt", None)
        if full is None or voc is None:
            raise _lib.HipBackendError("use_decoder=False needs the dvae_encode checkpoint (DVAE_full.pt, infer_type 'hip') and vocos configured")
        dcfg = dict(full["decoder_config"]); dcfg["n_mels"] = 100
        sc = hip_models.Synth(dcfg, voc["cfg"], max_frames=int(self.synth.cfg.max_frames), device=self.device, max_batch=int(self.synth.max_batch),
                              vq_cfg=full["vq_config"])
        sd = dict(torch.load(full["path"], weights_only=True, mmap=True))
        if "coef" not in sd:
            sd["coef"] = torch.from_numpy(codec.coef_from_string(self.dave_coef)).view(1, -1, 1)
        sc.load("dvae.", sd)
        sc.load("vocos.", torch.load(voc["path"], weights_only=True, mmap=True))
        self.synth_codes = sc
        return sc

    @torch.inference_mode()
    def _decode_to_wavs(self, result_list, use_decoder: bool = True):
        """pipeline:286-305: per utterance hidden[n,768] -> DVAE -> mel[1,100,2n] -> Vocos -> wav[256(2n-1)]; with use_decoder=False the
        inputs are the generated ids [n,4] and the decoder is the DVAE_full model (pipeline:292,435-439)."""
        if not use_decoder:
            return self._codes_synth().decode_batch(list(result_list))
        if len(result_list) >= 1 and getattr(self, "synth", None) is not None:
            return self.synth.decode_batch(list(result_list))           # one launch sequence for the batch (ctts_synth_batch)
        wavs = []
        decoder, vocos = self.models_dict["dvae_decode"], self.models_dict["vocos"]
        for h in result_list:
            if h.shape[0] == 0:
                wavs.append(torch.zeros(0, device=self.device))
                continue
            mel = decoder(h.permute(1, 0)[None])
            wavs.append(vocos.decode(mel)[0])
        return wavs

    def _request_wavs(self, req: _Request, result_list):
        """_decode_to_wavs for a request, at the rate it asked for: one ctts_resample_windows launch over the vocoded batch"""
        wavs = self._decode_to_wavs(result_list, req.use_decoder)
        return wavs if req.sample_rate is None else self.resampler(req.sample_rate).resample(wavs)

    def resampler(self, rate: int):
        """The hip_models.Resampler 24 kHz -> `rate`, one per rate, created on first use (an unsupported pair is refused there)."""
        cache = self.__dict__.setdefault("_resamplers", {})
        if int(rate) not in cache:
            cache[int(rate)] = hip_models.Resampler(NATIVE_RATE, int(rate), device=self.device)
        return cache[int(rate)]

    def output_rate(self, sample_rate, who: str) -> Optional[int]:
        """sample_rate= of infer / open_session / submit: None for None or 24000 (the vocoder's own rate: nothing is resampled, today's path launch for
        launch), else the rate as an int with its resampler created -- so a pair the device resampler does not serve is refused by the call that names it."""
        if sample_rate is None:
            return None
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or int(sample_rate) < 1:
            raise _lib.HipBackendError(f"{who}: sample_rate={sample_rate!r} (a positive integer number of Hz)")
        if int(sample_rate) == NATIVE_RATE:
            return None
        try:
            self.resampler(int(sample_rate))
        except _lib.HipBackendError as e:
            raise _lib.HipBackendError(f"{who}: sample_rate={int(sample_rate)}: {e}") from None
        return int(sample_rate)

    def _adapter_slots(self, gpt, paths) -> List[int]:
        """Slot per utterance for `paths` (adapter directory or None each); adapters are loaded into the engine's resident slots on first
        use and evicted least-recently-used first (at most _lib.MAX_ADAPTERS distinct adapters per slice)."""
        if not hasattr(self, "_slot_of_path"):
            self._slot_of_path = OrderedDict()
        need = [p for p in dict.fromkeys(paths) if p]
        if len(need) > _lib.MAX_ADAPTERS:
            raise _lib.HipBackendError(f"{len(need)} distinct adapters in one slice; the engine holds {_lib.MAX_ADAPTERS}: lower slice_size")
        for p in need:
            if p in self._slot_of_path:
                self._slot_of_path.move_to_end(p)
                continue
            if len(self._slot_of_path) >= _lib.MAX_ADAPTERS:
                victim = next(q for q in self._slot_of_path if q not in need)
                slot = self._slot_of_path.pop(victim)
            else:
                slot = next(i for i in range(_lib.MAX_ADAPTERS) if i not in self._slot_of_path.values())
            gpt.load_adapter(slot, load_lora_adapter(p))
            self._slot_of_path[p] = slot
        return [(-1 if not p else self._slot_of_path[p]) for p in paths]

    def _gpt_for_lora(self, lora_path: Optional[str]):
        """pipeline:420-434,465-470: the reference merges the adapter into a copy of the Llama for the call and restores
        `gpt_org` afterwards, i.e. it holds ONE merged model at a time.  Here a merged sibling engine (GPT.with_lora: its own
        packed weights, the base engine's KV cache shared) is cached per adapter path in a small LRU (`lora_cache`, default 1);
        evicted engines are destroyed, so a service cycling through adapters does not grow HBM."""
        if not lora_path:
            return self.models_dict["gpt"]
        if lora_path in self._lora_models:
            self._lora_models.move_to_end(lora_path)
            return self._lora_models[lora_path]
        while len(self._lora_models) >= self._lora_cache:
            victim = next(iter(self._lora_models))
            if self._lora_models[victim].busy:
                # a partially consumed infer(stream=True) generator still owns the KV cache its siblings share and, possibly, this
                # engine's native handle: destroying it now would be a use-after-free when that generator resumes
                raise _lib.HipBackendError(f"cannot load adapter {lora_path!r}: a generator of an earlier infer() call is still live "
                                           f"(adapter {victim!r} would have to be evicted); exhaust or close it first")
            _, old = self._lora_models.popitem(last=False)
            old.close()
        base = self.models_dict["gpt"]
        self._lora_models[lora_path] = base.with_lora(load_lora_adapter(lora_path))
        return self._lora_models[lora_path]

    def _speaker_rows(self, call_spk, diffs) -> torch.Tensor:
        """[N, 768] speaker rows for params_per_utterance: an utterance's own spk_emb where it sets one, else the call's (a speaker string / vector,
        or row u of a per-utterance table, infer_sharded)."""
        dim = self.models_dict["gpt"].model_dim

        def vec(v):
            return codec.speaker_to_vector(v).view(dim) if isinstance(v, str) else torch.as_tensor(v, dtype=torch.float32).cpu().reshape(dim)
        table = _is_speaker_table(call_spk, len(diffs))
        rows = []
        for u, d in enumerate(diffs):
            if "spk_emb" in d:
                rows.append(vec(d["spk_emb"]))
            elif d.get("spk_smp") is not None:
                rows.append(torch.zeros(dim))               # a cloned voice: its prompt has no [spk_emb] token, the row is never applied
            elif call_spk is None:
                raise _lib.HipBackendError("params_per_utterance: an utterance sets spk_emb and the call has no speaker for the others")
            else:
                rows.append(call_spk[u].float().cpu() if table else vec(call_spk))
        return torch.stack(rows)

    def _infer(self, text_in, stream=False, lang=None, skip_refine_text=False, refine_text_only=False, use_decoder=True,
               do_text_normalization=True, do_text_optimization=True, do_homophone_replacement=True,
               params_refine_text=RefineTextParams(), params_infer_code=InferCodeParams(), **kwargs):
        """pipeline:333-470: the text front-end, the request resolved once, the generator of its mode.  A generator itself: no refusal is raised before the first next()."""
        if not isinstance(text_in, list):
            text_in = [text_in]
        if do_text_optimization and self.text_splitter is not None:
            # pipeline:353-377: split on newlines, hand the lines to the (pluggable) sentence splitter, merge short sentences
            lines = [t.strip() for text_ in text_in for t in text_.split("\n") if t.strip()]
            text_in = merge_short_sentences(self.text_splitter(lines))
        text_in = [self.normalizer(t, do_text_normalization, do_homophone_replacement, lang) for t in text_in]
        req = self._resolve_request(text_in, stream, skip_refine_text, refine_text_only, use_decoder, params_refine_text, params_infer_code, kwargs)
        if (req.n_cand > 1 or req.return_details) and not req.refine_text_only:
            yield from self._infer_details(req)
        elif req.continuous and len(req.texts) > req.slice_size:
            yield from self._infer_continuous(req)
        else:
            yield from self._infer_sliced(req)

    def _resolve_request(self, texts, stream, skip_refine_text, refine_text_only, use_decoder, params_refine_text, params_infer_code, kwargs) -> _Request:
        """_infer()'s arguments and keywords -> the _Request its paths read, with every refusal that does not depend on the path.  Unknown keywords are ignored."""
        n, after = len(texts), " (after text splitting)"
        slice_size = int(kwargs.get("slice_size", self.models_dict["gpt"].max_batch))     # reference: 4 (pipeline:391)
        gpt = self._gpt_for_lora(kwargs.get("lora_path"))
        # `lora_paths` (the reference merges ONE adapter for a whole call): one adapter directory (or None) per text; up to 8 stay resident, each row selects its own
        lora_paths = kwargs.get("lora_paths")
        if lora_paths is not None and kwargs.get("lora_path"):
            raise _lib.HipBackendError("lora_path (one merged adapter) and lora_paths (one adapter per utterance) are exclusive")
        _check_entries("lora_paths", lora_paths, n, after)
        # Device noise is keyed by (request seed, global utterance id): one seed per request and each utterance its own id, so the result does not depend on slice_size or
        # on which rank serves the utterance (infer_sharded).  `noise="auto"` keeps the reference-compatible torch-generator noise for slices of <= 4 utterances.
        noise_mode = kwargs.get("noise", "auto")
        utt_ids = kwargs.get("utt_ids") if kwargs.get("utt_ids") is not None else list(range(n))
        _check_entries("utt_ids", utt_ids, n, after)
        # optional per-utterance token limits (<= params_infer_code.max_new_token): ctts_gen_io.row_limits
        utt_limits = kwargs.get("max_new_tokens_per_utterance")
        _check_entries("max_new_tokens_per_utterance", utt_limits, n, after)
        # optional per-utterance parameters (no counterpart in the reference, whose InferCodeParams apply to a whole call): one InferCodeParams or dict of
        # overrides per utterance; the sampling knobs go to the engine's per-row table (GPT sampling_per_row), max_new_token to the per-row limits
        utt_sampling = utt_prompts = utt_voices = None
        diffs = kwargs.get("_utt_overrides")       # infer / infer_sharded: the entries already resolved against the params their CALLER passed
        if diffs is None and kwargs.get("params_per_utterance") is not None:
            diffs = per_utterance_overrides(params_infer_code, kwargs["params_per_utterance"])
        if diffs is not None:
            _check_entries("params_per_utterance", diffs, n, after)
            if any(set(d) & set(PER_UTTERANCE_SAMPLING) for d in diffs):
                utt_sampling = [({k: d[k] for k in PER_UTTERANCE_SAMPLING if k in d} or None) for d in diffs]
            if any("max_new_token" in d for d in diffs):
                if utt_limits is not None:
                    raise _lib.HipBackendError("params_per_utterance with a per-utterance max_new_token and max_new_tokens_per_utterance are exclusive")
                utt_limits = [int(d.get("max_new_token", params_infer_code.max_new_token)) for d in diffs]
                params_infer_code = dataclasses.replace(params_infer_code, max_new_token=max(utt_limits))
            if any("prompt" in d for d in diffs):
                utt_prompts = [d.get("prompt", params_infer_code.prompt) or "" for d in diffs]
            utt_voices = utterance_voices(params_infer_code, diffs)            # (against the call's speaker, before the table below replaces it)
            if any("spk_emb" in d for d in diffs):
                params_infer_code = dataclasses.replace(params_infer_code, spk_emb=self._speaker_rows(params_infer_code.spk_emb, diffs))
        # return_details / num_candidates (no counterpart in the reference): log-probs written by the sampler, N candidates per utterance ranked by them
        n_cand = check_candidate_request(kwargs.get("num_candidates", 1), utt_ids, stream, noise_mode)
        # refine_candidates (the text twin): every text refined N times as ordinary text rows, ranked by the text sampler's raw log-probs; the winner feeds the code pass
        refine_cand = check_refine_candidates(kwargs.get("refine_candidates", 1), utt_ids, stream, noise_mode, slice_size)
        # sample_rate (no counterpart in the reference, which delivers 24 kHz): the finished waveforms resampled on the device; the pair is refused here, before any decoding
        rate = self.output_rate(kwargs.get("sample_rate"), "infer")
        if rate is not None and stream:
            raise _lib.HipBackendError(f"infer(stream=True, sample_rate={rate}) is not offered: its windows are slices of different prefix waveforms, so there is no "
                                       "single waveform to resample (stream from a session: open_session + submit(stream=\"exact\", sample_rate=...))")
        if (n_cand > 1 or kwargs.get("return_details")) and not refine_text_only and stream:
            raise _lib.HipBackendError("return_details=True needs stream=False")
        return _Request(texts=texts, gpt=gpt, slice_size=slice_size, params_refine_text=params_refine_text, params_infer_code=params_infer_code, utt_ids=utt_ids,
                        utt_limits=utt_limits, utt_sampling=utt_sampling, utt_prompts=utt_prompts, utt_voices=utt_voices, lora_paths=lora_paths, noise_mode=noise_mode, stream=stream,
                        noise_seed=kwargs.get("noise_seed"), use_decoder=use_decoder, skip_refine_text=skip_refine_text, refine_text_only=refine_text_only,
                        continuous=kwargs.get("continuous"), n_cand=n_cand, return_details=bool(kwargs.get("return_details")), select=kwargs.get("select"),
                        share_prompt=kwargs.get("share_prompt"), ids_sink=kwargs.get("_ids_sink"), overlap_vocoder=bool(kwargs.get("overlap_vocoder", False)),
                        vocoder_chunk=kwargs.get("vocoder_chunk", 32), sample_rate=rate, refine_cand=1 if skip_refine_text else refine_cand,
                        refine_guide=None if skip_refine_text else resolve_refine_guided(kwargs.get("refine_guided"), self.models_dict["tokenizer"]))

    def _infer_sliced(self, req: _Request):
        """pipeline:391-470: slices of slice_size utterances, each waiting for its slowest row; one list of waveforms per slice (stream=True: [B, samples]
        windows of the slice's padded prefix waveforms).  The request seed is drawn lazily: inside the first slice that uses device noise, after that slice's
        refine pass -- slices of <= 4 under noise="auto" keep the reference-compatible torch noise and draw nothing."""
        gpt, seed = req.gpt, req.noise_seed
        for ii in range(0, len(req.texts), req.slice_size):
            idx = range(ii, min(ii + req.slice_size, len(req.texts)))
            text = [req.texts[i] for i in idx]
            if not req.skip_refine_text:                                                   # pipeline:399-411
                ckw = {}
                if req.refine_cand > 1:            # N refinements per text through slice_size rows, device noise keyed by candidate_utt_id
                    seed = seed if seed is not None else _draw_request_seed()
                    ckw = dict(continuous_rows=req.slice_size, seed=seed, utt_ids=[req.utt_ids[i] for i in idx], **req.cand_kw)
                text = _decode_refined(self.models_dict["tokenizer"], self._refine_text(text, req.params_refine_text, **req.guide_kw, **ckw).ids)
                if req.refine_text_only:
                    yield text
            if req.refine_text_only:
                continue
            text = [_with_uv_break(t) for t in text]
            kw = req.rows(idx, adapters=True)
            pic, utt_ids, paths = kw.pop("params"), kw.pop("utt_ids"), kw.pop("lora_paths", None)
            if paths is not None:
                gpt.set_row_adapters(self._adapter_slots(gpt, paths))
            if req.noise_mode != "auto" or len(text) > 4:      # device (or caller-chosen) noise; slices of <= 4 keep the reference-compatible default
                if seed is None and (req.noise_mode in ("auto", "device")):
                    seed = _draw_request_seed()
                kw.update(noise=("device" if req.noise_mode == "auto" else req.noise_mode), seed=seed, utt_ids=utt_ids)
            results = self._infer_code(text, req.stream, req.use_decoder, pic, gpt=gpt, **kw)
            length, passed, last, total = 0, 0, None, 0
            try:
                for result in results:
                    if not req.stream:
                        if req.ids_sink is not None:
                            req.ids_sink.extend(zip(utt_ids, result.ids))
                        yield self._request_wavs(req, result.hiddens if req.use_decoder else result.ids)      # pipeline:435-439
                        continue
                    # The reference's stream branch vocodes the whole prefix for every chunk and indexes a python list with .shape.  Here every yield is the
                    # [length, b) sample window of that prefix waveform, vocoded from the tokens in its receptive field only (Synth.decode_window), zero padded like pad_sequence pads
                    last, passed = (result.hiddens if req.use_decoder else result.ids), passed + 1
                    total = max(prefix_samples(h.shape[0]) for h in last)
                    b = min(length + pic.stream_speed, total)
                    if passed > pic.pass_first_n_batches and b > length:
                        yield self._window(last, length, b, req.use_decoder)
                        length = b
            finally:
                if paths is not None:               # the generator stays lazy (streaming works with per-utterance adapters); the row table is
                    gpt.set_row_adapters(None)      # reset when the slice is exhausted, closed or fails
            if total > length:                      # streaming: what is left once the slice has ended
                yield self._window(last, length, total, req.use_decoder)

    def _infer_continuous(self, req: _Request):
        """`continuous=True` (no counterpart in the reference): the request's utterances are NOT cut into slices that each wait for their slowest row
        (pipeline:391-397); slice_size decode rows are kept busy -- queued utterances take over the rows of finished ones (GPT.generate_many_iter,
        ctts_gpt_admit).  Device noise keyed by utterance id: every utterance gets the waveform the sliced path gives it, whatever the admission order.  Not
        for caller-supplied noise.  The completion events go to _stream_continuous, to _overlap_vocoder or to the ordered-prefix loop below."""
        if req.noise_mode not in ("auto", "device"):
            raise _lib.HipBackendError("continuous=True works with device noise")
        adapter_slots = None
        if req.lora_paths is not None:      # an admitted utterance brings its own adapter (ctts_gpt_admit_adapters): all adapters of the request are resident at once
            distinct = len({p for p in req.lora_paths if p})
            if distinct > _lib.MAX_ADAPTERS:
                raise _lib.HipBackendError(f"continuous=True: {distinct} distinct adapters in the request; the engine holds {_lib.MAX_ADAPTERS} (use slices: continuous=False)")
            adapter_slots = self._adapter_slots(req.gpt, req.lora_paths)
        seed = req.noise_seed if req.noise_seed is not None else _draw_request_seed()
        texts = list(req.texts)
        if not req.skip_refine_text:
            # pipeline:399-411 for the whole request at once, `slice_size` rows kept busy (noise keyed by utterance id on stream 4: a sentence's refined text does not depend on the batch)
            refined = self._refine_text(texts, req.params_refine_text, continuous_rows=req.slice_size, seed=seed, utt_ids=req.utt_ids, **req.guide_kw, **req.cand_kw)
            texts = _decode_refined(self.models_dict["tokenizer"], refined.ids)
            if req.refine_text_only:
                yield texts
                return
        texts = [_with_uv_break(t) for t in texts]
        # admission order: input order, or under "throughput" the longest first (the last rows to finish are short utterances) -- by the utterance's own token limit where the
        # caller gave one (bench.py's 256-utterance request: 2625 decode steps instead of 2905 for 2518 ideal ones); `throughput_order = "input"` keeps arrival order
        order = list(range(len(texts)))
        if req.continuous == "throughput" and getattr(self, "throughput_order", "longest_first") == "longest_first":
            limits = req.utt_limits if req.utt_limits is not None else [0] * len(texts)
            order.sort(key=lambda i: (-int(limits[i]), -len(texts[i]), i))
        kw = req.rows(order)
        if adapter_slots is not None:
            kw["adapter_slots"] = [adapter_slots[i] for i in order]
        events = self._infer_code([texts[i] for i in order], False, req.use_decoder, kw.pop("params"), gpt=req.gpt, continuous=True, seed=seed, rows=req.slice_size,
                                  progress=bool(req.stream), **kw)
        ordered, n_all = req.continuous != "throughput", len(texts)
        if req.stream:
            return (yield from self._stream_continuous(req, events, order))
        if not ordered and self.device.type == "cuda" and req.overlap_vocoder:
            return (yield from self._overlap_vocoder(req, events, order))
        # continuous=True: the waveforms IN ORDER as soon as a prefix of the request is complete (the first list as early as possible, later ones in groups of >= 8 so
        # that the vocoder runs batched) while the rest keeps decoding.  continuous="throughput": one list at the end, in input order.
        ready, next_i, first = {}, 0, True
        for done in self._completions(req, events, order):
            ready.update(done)
            run = 0
            while ordered and next_i + run in ready:
                run += 1
            if run and (first or run >= 8 or next_i + run == n_all):
                yield self._request_wavs(req, [ready.pop(next_i + j) for j in range(run)])
                next_i, first = next_i + run, False
        rest = [i for i in range(next_i, n_all) if i in ready]      # (everything, in throughput mode; nothing unless the run was interrupted, otherwise)
        if rest:
            yield self._request_wavs(req, [ready[i] for i in rest])

    def _stream_continuous(self, req: _Request, events, order):
        """stream=True with row re-use (no counterpart in the reference, whose stream branch serves one slice, pipeline:440-463): every yield is a list of
        (utterance index, sample window) -- the next [emitted, b) samples of that utterance's prefix waveform, vocoded from the tokens inside the window's
        receptive field only (Synth.decode_window) -- as soon as `stream_batch` new tokens of it exist; an utterance's last window comes with its completion."""
        syn = self.synth if req.use_decoder else self._codes_synth()
        p, emitted, last_n = req.params_infer_code, {}, {}
        for ev in events:
            final = not (isinstance(ev, tuple) and ev[0] == "progress")      # a completion list; else ("progress", [(k, tokens so far, ids, hiddens)])
            got = []
            for k, n, ids_k, hid_k in ([(k, int(ids_k.shape[0]), ids_k, hid_k) for k, ids_k, hid_k in ev] if final else ev[1]):
                u = order[k]
                total, s0 = prefix_samples(n), emitted.get(u, 0)
                if total > s0 and (final or n - last_n.get(u, 0) >= p.stream_batch):
                    b = total if final else min(s0 + p.stream_speed, total)
                    got.append((u, syn.decode_window([hid_k if req.use_decoder else ids_k], [s0], [b])[0]))
                    emitted[u], last_n[u] = b, int(n)
            if got:
                yield got

    def _completions(self, req: _Request, events, order):
        """generate_many_iter's completion events as lists of (utterance index, what the vocoder takes of it); the ids go to the request's ids_sink"""
        for ev in events:
            done = []
            for k, ids_k, hid_k in ev:
                if req.ids_sink is not None:
                    req.ids_sink.append((req.utt_ids[order[k]], ids_k))
                done.append((order[k], hid_k if req.use_decoder else ids_k))
            yield done

    def _overlap_vocoder(self, req: _Request, events, order):
        """continuous="throughput" + overlap_vocoder=True (OPT-IN): finished utterances are vocoded in batches of `vocoder_chunk` on a SIDE stream while the decode
        rows keep stepping on the caller's stream; one list at the end, in input order.  Measured: no gain (256 ragged utterances 2682 vs 2665-2687 ms: the
        vocoder's GEMMs fill the chip, the decode chain's small kernels queue behind them, and a <= 5-row tail's persistent launch shares the chip with them), so
        the default stays off; tests/test_gpu_pipeline.py::test_vocoder_overlap_soak drives exactly this overlap."""
        voc_chunk = max(1, int(req.vocoder_chunk))
        side = torch.cuda.Stream(device=self.device)
        t_req, t_first = torch.cuda.Event(enable_timing=True), None
        t_req.record(torch.cuda.current_stream(self.device))
        done_wavs, pending = {}, []

        def vocode(batch):              # [(utterance index, what the vocoder takes of it)]
            nonlocal t_first
            items = [it for _, it in batch]
            go = torch.cuda.Event()
            go.record(torch.cuda.current_stream(self.device))      # every token of these utterances was written before this point of the caller's stream
            side.wait_event(go)
            with torch.cuda.stream(side):
                for it in items:
                    it.record_stream(side)                           # (views of the generate call's buffers: keep the allocator off them until the side stream is done)
                wavs = self._request_wavs(req, items)
                if t_first is None:
                    t_first = torch.cuda.Event(enable_timing=True)
                    t_first.record(side)
            done_wavs.update((u, w) for (u, _), w in zip(batch, wavs))

        for done in self._completions(req, events, order):
            pending += done
            while len(pending) >= voc_chunk:
                vocode(pending[:voc_chunk])
                pending = pending[voc_chunk:]
        if pending:
            vocode(pending)
        torch.cuda.current_stream(self.device).wait_stream(side)      # the caller's stream sees the finished waveforms
        side.synchronize()
        self.last_first_audio_ms = t_req.elapsed_time(t_first) if t_first is not None else None
        if done_wavs:
            yield [done_wavs[i] for i in sorted(done_wavs)]

    def _infer_details(self, req: _Request):
        """infer(return_details=True) / infer(num_candidates=N): the code pass with return_logprobs, every utterance served N times as ordinary decode rows
        (candidate k under noise key candidate_utt_id(u, k), so candidate 0 is the plain generation), the winner picked by `select` or select_candidate,
        only winners vocoded.  Sliced: max(1, slice_size // N) utterances per slice, one yield per slice; continuous (more rows than slice_size): the
        whole request through GPT.generate_many, one yield.  The refine-text pass runs once per utterance, before the candidates are laid out.
        `share_prompt` (resolve_share_prompt): the candidates of an utterance share its prompt pass -- each utterance is tokenised and embedded once and the
        rows name their prompt (GPT prompt_of); speaker rows, prompts and adapters go per prompt, limits / sampling / noise keys per row."""
        tok, gpt = self.models_dict["tokenizer"], req.gpt
        n_utt, n_cand, slice_size = len(req.texts), req.n_cand, req.slice_size
        if n_cand > slice_size:
            raise _lib.HipBackendError(f"num_candidates={n_cand} exceeds slice_size={slice_size}: the candidates of an utterance share one decode batch")
        cont = bool(req.continuous) and n_utt * n_cand > slice_size
        if cont and req.noise_mode not in ("auto", "device"):
            raise _lib.HipBackendError("continuous=True works with device noise")
        per_slice = max(1, slice_size // n_cand)
        seed = req.noise_seed
        if seed is None and req.noise_mode in ("auto", "device") and (req.device_noise or cont or min(per_slice, n_utt) * n_cand > 4):
            seed = _draw_request_seed()
        texts = list(req.texts)
        refined = None
        if not req.skip_refine_text:                 # once per utterance (refine_candidates: N times), in the batches the plain call refines in
            # return_details: the pass also returns its log-probs (RefinedTexts).  Asked through the instance, not through a keyword: the calls below are the
            # plain request's, argument for argument
            self._refine_details = bool(req.return_details)
            try:
                if cont:
                    parts = [self._refine_text(texts, req.params_refine_text, continuous_rows=slice_size, seed=seed, utt_ids=req.utt_ids, **req.guide_kw, **req.cand_kw)]
                else:
                    parts = []
                    for ii in range(0, n_utt, slice_size):
                        ckw = {}
                        if req.refine_cand > 1:
                            seed = seed if seed is not None else _draw_request_seed()
                            ckw = dict(continuous_rows=slice_size, seed=seed, utt_ids=req.utt_ids[ii:ii + slice_size], **req.cand_kw)
                        parts.append(self._refine_text(texts[ii:ii + slice_size], req.params_refine_text, **req.guide_kw, **ckw))
            finally:
                self._refine_details = False
            texts = [t for p in parts for t in _decode_refined(tok, p.ids)]
            if req.return_details and all(isinstance(p, RefinedTexts) for p in parts):
                refined = ([lp for p in parts for lp in p.logprobs], [m for p in parts for m in p.mean_logprob])
        texts = [_with_uv_break(t) for t in texts]
        read_option = getattr(gpt, "get_option", None)           # (an engine object without options shares only when asked to)
        share = resolve_share_prompt(req.share_prompt, n_cand, n_cand > 1 and read_option is not None and read_option("batch_invariant"))
        for us in ([range(n_utt)] if cont else [range(ii, min(ii + per_slice, n_utt)) for ii in range(0, n_utt, per_slice)]):
            cands = self._run_candidates(req, texts, list(us), seed, cont, share)
            if cands is not None:
                yield self._pick_candidates(req, list(us), cands, refined)

    def _run_candidates(self, req: _Request, texts, us, seed, cont: bool, share: bool):
        """utterances `us` x n_cand candidates as one list of rows (utterance-major) -> one CandidateDetails per row; None: ensure_non_empty gave up (gpt.py:525)"""
        gpt, n_cand, use_decoder = req.gpt, req.n_cand, req.use_decoder
        rows = [(u, k) for u in us for k in range(n_cand)]
        src = [(u, 0) for u in us] if share else rows          # what is tokenised and embedded: every utterance once, or every row
        row_kw = req.rows([u for u, _ in rows], adapters=True, params=not share)
        src_kw = req.rows([u for u, _ in src]) if share else row_kw           # speaker rows and prompts go per prompt, the rest per row
        pic, paths = src_kw["params"], row_kw.get("lora_paths")
        gen_kw = dict(return_logprobs=True)
        for key, of in (("max_new_tokens_per_row", row_kw), ("sampling_per_row", row_kw), ("prompts", src_kw), ("voices", src_kw)):
            if key in of:
                gen_kw[key] = of[key]
        if share:
            gen_kw["prompt_of"] = [j for j in range(len(us)) for _ in range(n_cand)]
        if req.device_noise or cont or len(rows) > 4:      # (the plain call's rule: slices of <= 4 keep the reference-compatible torch noise under "auto")
            gen_kw.update(seed=seed, utt_ids=[candidate_utt_id(i, k) for i, (_, k) in zip(row_kw["utt_ids"], rows)])
            if not cont:
                gen_kw["noise"] = "device" if req.noise_mode == "auto" else req.noise_mode
        elif req.noise_mode != "auto":
            gen_kw["noise"] = req.noise_mode
        slots = self._adapter_slots(gpt, paths) if paths is not None else None
        if cont:            # the whole request at once, more rows than slice_size: row re-use (GPT.generate_many_iter), an admitted row brings its adapter
            gen_kw.update(continuous=True, rows=req.slice_size, adapter_slots=slots)
        res = None
        try:
            if slots is not None and not cont:
                gpt.set_row_adapters(slots)
            results = self._infer_code([texts[u] for u, _ in src], False, use_decoder, pic, gpt=gpt, **gen_kw)
            try:
                while True:
                    res = next(results)            # GPT.generate: the last result counts
            except StopIteration as stop:
                res = stop.value if cont else res      # GPT.generate_many_iter: the GenerationOutputs of all rows is the generator's return value
        finally:
            if slots is not None and not cont:
                gpt.set_row_adapters(None)
        return None if res is None else [CandidateDetails(ids=res.ids[r], logprobs=res.logprobs[r].cpu(), sampled_logprobs=res.sampled_logprobs[r].cpu(),
                                                          mean_logprob=mean_logprob(res.logprobs[r]), final_logprobs=res.final_logprobs[r],
                                                          hiddens=res.hiddens[r] if use_decoder else None) for r in range(len(rows))]

    def _pick_candidates(self, req: _Request, us, cands, refined=None):
        """the winner of every utterance of `us` among its n_cand CandidateDetails (`select` or select_candidate), vocoded: a list of waveforms or InferDetails"""
        n_cand, use_decoder = req.n_cand, req.use_decoder
        chosen, scores = [], []
        for j in range(len(us)):
            group = cands[j * n_cand:(j + 1) * n_cand]
            sc = torch.tensor([c.mean_logprob for c in group], dtype=torch.float64)
            k = int(req.select(list(group))) if req.select is not None else select_candidate(sc.tolist())
            if not 0 <= k < n_cand:
                raise _lib.HipBackendError(f"select returned {k}: not a candidate index (0..{n_cand - 1})")
            chosen.append(k)
            scores.append(sc)
        win = [cands[j * n_cand + k] for j, k in enumerate(chosen)]
        if req.ids_sink is not None:
            req.ids_sink.extend((req.utt_ids[u], w.ids) for u, w in zip(us, win))
        wavs = self._request_wavs(req, [w.hiddens if use_decoder else w.ids for w in win])      # pipeline:435-439; winners only
        if not req.return_details:
            return wavs
        det = InferDetails(wavs=wavs, ids=[w.ids for w in win], logprobs=[w.logprobs for w in win], sampled_logprobs=[w.sampled_logprobs for w in win],
                           mean_logprob=[w.mean_logprob for w in win])
        if refined is not None:                      # the refine pass ran: the raw log-probs of each utterance's refined ids ([Ebreak] step included) and their mean
            det.refined_logprobs, det.refined_mean_logprob = [refined[0][u] for u in us], [refined[1][u] for u in us]
        if n_cand > 1:
            det.candidate, det.candidate_scores = chosen, scores
            det.candidates = [[dataclasses.replace(c, hiddens=None) for c in cands[j * n_cand:(j + 1) * n_cand]] for j in range(len(us))]
        return det

    def _window(self, hiddens, s0: int, s1: int, use_decoder: bool = True) -> torch.Tensor:
        """[B, s1-s0] samples s0..s1 of the padded batch of prefix waveforms."""
        syn = self.synth if use_decoder else self._codes_synth()
        parts = syn.decode_window(list(hiddens), [s0] * len(hiddens), [s1] * len(hiddens))
        out = torch.zeros(len(parts), s1 - s0, device=self.device)
        for u, w in enumerate(parts):
            out[u, :w.shape[0]] = w
        return out

    @torch.no_grad()
    def infer(self, text, stream=False, lang=None, skip_refine_text=False, refine_text_only=False, use_decoder=True,
              do_text_normalization=True, do_text_optimization=True, do_homophone_replacement=True,
              params_refine_text=RefineTextParams(), params_infer_code=InferCodeParams(), **kwargs):
        """pipeline:472-579.  Speaker resolution: `speaker_emb_path` (.pt holding a base16384 str or a tensor),
        else params_infer_code.spk_emb as given (the reference overwrites it with a random speaker whenever no path is passed,
        pipeline:547-556), else a random speaker from spk_stat.  The params object is copied first: the default argument is one shared
        instance, and the reference's in-place writes make a zero-shot prompt or a sampled speaker stick to every later default call.
        `params_per_utterance`: one InferCodeParams or dict per utterance (after text splitting); an entry overrides the fields in which it differs
        from the params_infer_code passed HERE -- not from the speaker / zero-shot prompt filled in below.  An entry may name a cloned voice
        (spk_smp / txt_smp: ClonedVoice.overrides(), clone_voices) on every path -- sliced, continuous, stream, num_candidates (the candidates of an
        utterance share its voice, hence its prompt pass); such a row is tagged [empty_spk], rows with a speaker vector and cloned rows mix freely.
        No random speaker is sampled for a call that names a cloned voice (params_infer_code.spk_smp) or whose every utterance brings its own voice."""
        own_voices = False
        if kwargs.get("params_per_utterance") is not None:
            kwargs["_utt_overrides"] = per_utterance_overrides(params_infer_code, kwargs.pop("params_per_utterance"))
            own_voices = bool(kwargs["_utt_overrides"]) and all(("spk_emb" in d or d.get("spk_smp") is not None) for d in kwargs["_utt_overrides"])
        params_infer_code = dataclasses.replace(params_infer_code)
        if kwargs.get("speaker_audio_path"):                                      # zero shot (pipeline:486-499)
            p = kwargs["speaker_audio_path"]
            assert os.path.exists(p), f"speaker_audio_path {p} not exists!"
            params_infer_code.spk_smp = self.sample_audio_speaker(self._load_clip(p))
            params_infer_code.txt_smp = kwargs.get("speaker_audio_text", "")
            params_infer_code.spk_emb = None
        elif kwargs.get("speaker_emb_path"):
            p = kwargs["speaker_emb_path"]
            assert os.path.exists(p), f"speaker_emb_path {p} not exists!"
            obj = torch.load(p, weights_only=True, map_location="cpu")
            if isinstance(obj, dict):
                obj = next(iter(obj.values()))
            params_infer_code.spk_emb = obj if isinstance(obj, str) else codec.speaker_to_vector(obj)
        elif params_infer_code.spk_emb is None and params_infer_code.spk_smp is None and not own_voices:
            # (a call that names a cloned voice itself -- spk_smp, as open_session reads it -- or whose every utterance brings its own voice needs no sampled speaker)
            params_infer_code.spk_emb = self.sample_random_speaker()
        return self._infer(text, stream, lang, skip_refine_text, refine_text_only, use_decoder, do_text_normalization,
                           do_text_optimization, do_homophone_replacement, params_refine_text, params_infer_code, **kwargs)

    # -- serving session (no counterpart in the reference) ------------------------------------------------------------------------
    def open_session(self, params_infer_code: Optional[InferCodeParams] = None, use_decoder: bool = True, lora_path: Optional[str] = None, rows: Optional[int] = None,
                     seed: Optional[int] = None, return_details: bool = False, refine: Optional[RefineTextParams] = None, sample_rate: Optional[int] = None, refine_guided=False,
                     **out_of_scope) -> SynthSession:
        """A SynthSession: submit(text) / cancel(ticket) / poll() / drain() / close() while the engine keeps decoding -- the decode batch grows when texts arrive
        and shrinks when they end.  `params_infer_code` are the session's values (speaker included; a random one is sampled if it names none), `lora_path` one
        merged adapter for the whole session (an utterance may name its own at submit), `rows` bounds the decode batch, `seed` keys the device noise.
        `refine` (a RefineTextParams; max_new_token <= the code parameters', repetition_penalty 1): submit() refines every text first, inside the session -- as
        a text row beside the code rows (SynthSession); SessionDetails.refined_text carries the result.  `sample_rate`: the session's output rate in Hz (None or
        24000: the vocoder's own); a submit may name its own.
        Not offered inside a session (refused): num_candidates / shared prompt passes, caller-supplied noise, session-wide streaming windows
        (stream=True here: streaming is asked per utterance, submit(stream="exact" | "eager")), infer_sharded, and infer()'s call-level names of the refine-text
        pass (refine_text_only, params_refine_text: use refine=)."""
        refuse_out_of_scope(out_of_scope, "use infer() for it (the refine-text pass is served inside a session through open_session(refine=RefineTextParams(...)))")
        if refine is not None and not isinstance(refine, RefineTextParams):
            raise _lib.HipBackendError("open_session: refine must be a RefineTextParams")
        params = dataclasses.replace(params_infer_code if params_infer_code is not None else InferCodeParams())
        if params.spk_emb is None and params.spk_smp is None:
            params.spk_emb = self.sample_random_speaker()
        return SynthSession(self, self._gpt_for_lora(lora_path), params, use_decoder, rows, seed, return_details, refine=refine, sample_rate=sample_rate, refine_guided=refine_guided)

    # -- multi-GPU: utterance sharding (BASELINE configs[3]: batch 256 over 8 GPUs) --------------------------------
    @torch.no_grad()
    def infer_sharded(self, texts: List[str], speaker_index: Optional[List[int]] = None, speaker_table: Optional[torch.Tensor] = None,
                      skip_refine_text: bool = True, params_refine_text=RefineTextParams(), params_infer_code=InferCodeParams(), **kwargs):
        """One request over all ranks of the initialised torch.distributed group (one process per GPU; world 1 works too).
        Every rank calls this with the same `texts`; utterances are independent (the reference runs them as sequential slices
        of 4 with no cross-slice state, pipeline:391-397), so they are split by `dist.partition` (length-balanced snake) and
        each rank runs its own utterances through the ordinary `_infer` (slices of `max_batch`) + `_decode_to_wavs`.  The only
        exchange: ONE broadcast of the speaker table [n_spk, 768] from rank 0 (RCCL over xGMI) and one all-reduce of the
        generated lengths (disjoint supports).  `speaker_index[i]` selects utterance i's row; without a table every utterance
        uses params_infer_code.spk_emb.
        `params_per_utterance` (one entry per GLOBAL utterance) is accepted with every per-utterance field, cloned voices (spk_smp / txt_smp) included: the
        list is an argument every rank holds, like `prompt`, so nothing more is exchanged -- a cloned row ignores its speaker_index row.
        Returns (indices of this rank's utterances, their waveforms in that order, generated token counts of ALL utterances).
        Note SURVEY F8: the reference's repetition penalty skips rows >= 625 of the flattened [B*4] batch; a rank never holds
        more than max_batch <= 128 sequences (512 rows) per call, so the quirk cannot trigger on any rank."""
        from . import dist as cdist
        if kwargs.get("num_candidates", 1) != 1 or kwargs.get("return_details"):
            raise _lib.HipBackendError("infer_sharded serves one generation per utterance and returns waveforms: num_candidates > 1 and return_details are "
                                       "refused (rank the candidates with infer() on one rank)")
        kwargs.pop("num_candidates", None); kwargs.pop("return_details", None)
        if kwargs.get("refine_candidates", 1) != 1:
            raise _lib.HipBackendError("infer_sharded(refine_candidates=...) is not offered: text log-probs are not exchanged between ranks (rank the "
                                       "refinements with infer() on one rank)")
        kwargs.pop("refine_candidates", None)
        if kwargs.get("refine_guided") not in (None, False):
            raise _lib.HipBackendError("infer_sharded(refine_guided=...) is not offered: guided refinement is served by infer() and by sessions "
                                       "(open_session(refine=..., refine_guided=...))")
        kwargs.pop("refine_guided", None)
        if kwargs.get("sample_rate") is not None and int(kwargs["sample_rate"]) != NATIVE_RATE:
            raise _lib.HipBackendError(f"infer_sharded(sample_rate={kwargs['sample_rate']}) is not offered: the generated lengths every rank exchanges are read off "
                                       "its 24 kHz waveforms; resample a rank's waveforms with pipe.resampler(rate).resample(wavs)")
        kwargs.pop("sample_rate", None)
        if not isinstance(texts, list):
            texts = [texts]
        params = dataclasses.replace(params_infer_code)
        n_spk, dim = 1, self.models_dict["gpt"].model_dim
        if speaker_table is not None or speaker_index is not None:
            if speaker_index is None or len(speaker_index) != len(texts):
                raise _lib.HipBackendError("infer_sharded: speaker_index needs one entry per utterance")
            if speaker_table is None and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
                raise _lib.HipBackendError("infer_sharded: speaker_index given without speaker_table (rank 0 holds the table that is broadcast)")
            n_spk = int(max(speaker_index)) + 1
            if speaker_table is not None:
                speaker_table = torch.as_tensor(speaker_table, dtype=torch.float32).reshape(-1, dim)
                assert speaker_table.shape[0] >= n_spk
                speaker_table = speaker_table[:n_spk]
        else:
            speaker_index = [0] * len(texts)
            if params.spk_emb is None:
                speaker_table = self._sample_random_speaker().view(1, dim) if (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0) else None
            else:
                speaker_table = codec.speaker_to_vector(params.spk_emb).view(1, dim) if isinstance(params.spk_emb, str) else torch.as_tensor(params.spk_emb, dtype=torch.float32).view(1, dim)
        slice_size = int(kwargs.pop("slice_size", self.models_dict["gpt"].max_batch))
        # the request's noise seed: the same on every rank; each utterance's device noise stream is keyed by (seed, its global index), so N ranks
        # produce what one rank would.  Without `noise_seed` rank 0 draws it from torch's CPU generator -- like infer() does, so torch.manual_seed /
        # TorchSeedContext reproduce a request and two requests differ -- and broadcasts it with the speaker table's process group.
        noise_seed = kwargs.pop("noise_seed", None)
        if noise_seed is None:
            noise_seed = cdist.broadcast_seed(_draw_request_seed(), self.device)
        noise_seed = int(noise_seed)
        kwargs.pop("noise", None); kwargs.pop("utt_ids", None)
        wavs_local: List[torch.Tensor] = []
        limits_all = kwargs.pop("max_new_tokens_per_utterance", None)          # per GLOBAL utterance; each slice gets its own entries
        lora_all = kwargs.pop("lora_paths", None)                              # one adapter directory (or None) per GLOBAL utterance; each slice gets its own entries
        ppu_all = kwargs.pop("params_per_utterance", None)                     # one InferCodeParams / dict of overrides per GLOBAL utterance; each slice gets its own
        for name, entries in (("max_new_tokens_per_utterance", limits_all), ("lora_paths", lora_all), ("params_per_utterance", ppu_all)):
            _check_entries(name, entries, len(texts))
        # resolved against the caller's params_infer_code: run_local below swaps spk_emb for the rank's speaker rows, which an entry must not be compared with
        over_all = per_utterance_overrides(params_infer_code, ppu_all) if ppu_all is not None else None
        ids_out = kwargs.pop("ids_out", None)                                  # optional list: receives this rank's generated ids, in `mine` order
        sink = [] if ids_out is not None else None
        continuous = bool(kwargs.pop("continuous", False))      # each rank keeps slice_size decode rows busy over ALL its utterances (infer(continuous=True))

        def run_local(indices, rows):
            lens = []
            step = len(indices) if continuous else slice_size
            for ii in range(0, len(indices), max(step, 1)):
                sl = indices[ii:ii + step]
                p = dataclasses.replace(params, spk_emb=rows[ii:ii + len(sl)])
                kw_sl = dict(kwargs, _ids_sink=sink)
                for key, per_utt in (("max_new_tokens_per_utterance", limits_all), ("lora_paths", lora_all), ("_utt_overrides", over_all)):
                    if per_utt is not None:
                        kw_sl[key] = [per_utt[i] for i in sl]
                for wavs in self._infer([texts[i] for i in sl], False, None, skip_refine_text, False, True, True, False, True,
                                        params_refine_text, p, slice_size=(slice_size if continuous else len(sl)), utt_ids=list(sl), noise="device",
                                        noise_seed=noise_seed, continuous=("throughput" if continuous else False), **kw_sl):
                    wavs_local.extend(wavs)
                    lens.extend([prefix_tokens(w.shape[0]) for w in wavs])
            return lens

        mine, all_lens = cdist.sharded_generate([len(t) for t in texts], speaker_index, speaker_table, n_spk, dim, self.device, run_local)
        if ids_out is not None:
            by_utt = dict(sink)
            ids_out.extend(by_utt[i] for i in mine)
        return mine, wavs_local, all_lens

