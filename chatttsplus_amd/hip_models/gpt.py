"""hip_models.GPT -- drop-in for chattts_plus.models.GPT (reference chattts_plus/models/gpt.py) whose
decoder, heads, sampler and generate-loop bookkeeping run in libctts_hip.so on an MI355X.

Same constructor kwargs, `__call__(input_ids, text_mask) -> emb`, `generate(...)` generator of
GenerationOutputs, `num_vq`, `emb_code[i].num_embeddings`, `.eval()`, `.to()`, `from_pretrained`.
torch is used for device memory, the current stream and the (negligible) embedding gather only.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib

RMS_EPS = 1e-6
ROPE_BASE = 10000.0


def rope_table(n_pos: int) -> np.ndarray:
    """[n_pos][64] = cos[32] | sin[32] with the reference's fp32 arithmetic (llama.py:100,106-119)."""
    inv_freq = 1.0 / (ROPE_BASE ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64))
    freqs = torch.arange(n_pos, dtype=torch.int64)[:, None].float() * inv_freq[None, :]
    return torch.cat((freqs.cos(), freqs.sin()), dim=-1).contiguous().numpy()


class _EmbShim:
    def __init__(self, n):
        self.num_embeddings = n


@dataclass(repr=False, eq=False)
class GenerationOutputs:          # gpt.py:280-284
    ids: List[torch.Tensor]
    attentions: list
    hiddens: List[torch.Tensor]
    # return_logprobs=True (no counterpart in the reference): per sequence b, [n_b, 4] aligned with ids[b] --
    #   logprobs          log_softmax(raw code logits)[id]: what GPT.score gives for the same token
    #   sampled_logprobs  log p(id) under the distribution the sampler drew from (after temperature, repetition penalty, top-P, top-K, min_new_token)
    #   final_logprobs    [2, 4] (raw, sampled) of the step that sampled EOS -- its ids are not part of ids[b] -- or None for a sequence that ended by its limit
    # return_text_logprobs=True with infer_text=True: the same three fields with ONE value per step -- [n_b], [n_b], [2] -- under the text head
    #   (ctts_gpt_set_text_logprob_out): logprobs is what GPT.score_text gives for the same token
    logprobs: Optional[List[torch.Tensor]] = None
    sampled_logprobs: Optional[List[torch.Tensor]] = None
    final_logprobs: Optional[List[Optional[torch.Tensor]]] = None


@dataclass(repr=False, eq=False)
class ScoreOutputs:
    """GPT.score: per sequence b, `logprob[b]` / `argmax[b]` [n_b, 4] (log_softmax of the raw code logits at the target, first argmax), `nll[b]` (the mean of
    -logprob) and `accuracy[b]` (argmax == target); over the whole batch the token-weighted `loss` and `accuracy` (train_lora.py:455-469)."""
    logprob: List[torch.Tensor]
    argmax: List[torch.Tensor]
    nll: torch.Tensor
    seq_accuracy: torch.Tensor
    loss: float
    accuracy: float


def score_reduce(logprob: List[torch.Tensor], argmax: List[torch.Tensor], targets: List[torch.Tensor]):
    """(nll [B], accuracy [B], loss, accuracy) from per-sequence [n_b, 4] log-probs, argmaxes and targets.  The batch values weight every (target, codebook)
    entry alike, as cross_entropy(..., ignore_index) and the masked accuracy mean of train_lora.py:455-469 do."""
    nll = torch.stack([(-lp.double()).mean() for lp in logprob]).float()
    acc = torch.stack([(am == t.to(am.dtype)).double().mean() for am, t in zip(argmax, targets)]).float()
    n = sum(int(lp.numel()) for lp in logprob)
    loss = float(sum(float(-lp.double().sum()) for lp in logprob) / n)
    accuracy = float(sum(int((am == t.to(am.dtype)).sum()) for am, t in zip(argmax, targets)) / n)
    return nll, acc, loss, accuracy


LORA_TARGETS = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


def check_lora_shapes(layer, target, A, B, hidden_size: int = 768, intermediate_size: int = 3072, where: str = "") -> None:
    """A must be [r, in] and B [out, r] for the (out, in) of the nn.Linear `target` names (llama.py:214,737-739: gate / up intermediate x hidden, down hidden x
    intermediate, q/k/v/o hidden x hidden): the engine reads both by these sizes.  ValueError naming layer, target and the shapes."""
    if target not in LORA_TARGETS:
        raise ValueError(f"LoRA{where}: layer {layer}: unknown target '{target}' (one of {' '.join(LORA_TARGETS)})")
    out, inn = {"gate_proj": (intermediate_size, hidden_size), "up_proj": (intermediate_size, hidden_size),
                "down_proj": (hidden_size, intermediate_size)}.get(target, (hidden_size, hidden_size))
    a, b = tuple(np.shape(A)), tuple(np.shape(B))
    r = a[0] if len(a) == 2 else -1
    if len(a) != 2 or len(b) != 2 or r < 1 or a != (r, inn) or b != (out, r):
        raise ValueError(f"LoRA{where}: layer {layer} {target}: A {a} / B {b}, expected (r, {inn}) / ({out}, r)")


def score_inputs(input_ids: torch.Tensor, attention_mask: torch.Tensor, text_mask: torch.Tensor, codes, eos_token: int, append_eos: bool = True):
    """Host helper of GPT.score (CPU): utterance i's codes [n_i, 4] follow its left-padded prompt (input_ids [B, T, 4], attention_mask / text_mask [B, T], as
    Tokenizer.encode gives them); the joined sequences are left padded again.  Returns dict(ids [B, T', 4], mask [B, T'] int32, text_mask [B, T'] bool,
    targets [B, max_targets, 4] int32, n_targets [B] int32).
      append_eos=True:  every code is an input row and the targets are the codes followed by EOS on all 4 codebooks (the extended labels of
                        train_lora.py:401-404), n_b = n_i + 1; the last code row predicts EOS, no EOS input row is needed.
      append_eos=False: the targets are the codes, n_b = n_i; the last code is not fed as input.
    Target j of sequence b is predicted by row T' - n_b + j (ctts_gpt_score)."""
    ids = torch.as_tensor(input_ids).cpu()
    mask = torch.as_tensor(attention_mask).cpu().to(torch.int64)
    tm = torch.as_tensor(text_mask).cpu().bool()
    if ids.dim() != 3 or mask.shape != ids.shape[:2] or tm.shape != ids.shape[:2]:
        raise ValueError(f"score_inputs: input_ids [B, T, num_vq] with attention_mask / text_mask [B, T] (got {tuple(ids.shape)}, {tuple(mask.shape)}, {tuple(tm.shape)})")
    B, nvq = int(ids.shape[0]), int(ids.shape[2])
    if len(codes) != B:
        raise ValueError(f"score_inputs: {len(codes)} code sequences for {B} prompts")
    _check_left_padded(mask)
    conts = []
    for b in range(B):
        c = torch.as_tensor(codes[b]).cpu().to(ids.dtype)
        if c.dim() != 2 or c.shape[1] != nvq:
            raise ValueError(f"score_inputs: codes[{b}] must be [n, {nvq}] (got {tuple(c.shape)})")
        if not append_eos and c.shape[0] < 1:
            raise ValueError(f"score_inputs: codes[{b}] is empty and append_eos is off: nothing to score")
        conts.append(c)
    return _join_scored(ids, mask, tm, conts, eos_token, append_eos)


def _join_scored(ids, mask, tm, conts, eos_token, append_eos):
    """The strip / append / re-pad work of score_inputs and score_text_inputs: prompt b without its left pad, then conts[b] [n_b, num_vq] (all of it under
    append_eos, where the targets end in a row of EOS; else without its last row), left padded again to the longest -> score_inputs' dict."""
    B, nvq = int(ids.shape[0]), int(ids.shape[2])
    seqs, tms, tgts = [], [], []
    for b, c in enumerate(conts):
        pad = int((mask[b] == 0).sum())
        inp = c if append_eos else c[:-1]
        seqs.append(torch.cat([ids[b, pad:], inp], 0))
        tms.append(torch.cat([tm[b, pad:], torch.zeros(inp.shape[0], dtype=torch.bool)], 0))
        tgts.append(torch.cat([c, torch.full((1, nvq), int(eos_token), dtype=c.dtype)], 0) if append_eos else c)
    T = max(int(s.shape[0]) for s in seqs)
    nt = torch.tensor([int(t.shape[0]) for t in tgts], dtype=torch.int32)
    out_ids = torch.zeros(B, T, nvq, dtype=ids.dtype)
    out_mask = torch.zeros(B, T, dtype=torch.int32)
    out_tm = torch.zeros(B, T, dtype=torch.bool)
    targets = torch.zeros(B, int(nt.max()), nvq, dtype=torch.int32)
    for b in range(B):
        n = int(seqs[b].shape[0])
        out_ids[b, T - n:] = seqs[b]
        out_mask[b, T - n:] = 1
        out_tm[b, T - n:] = tms[b]
        targets[b, :int(nt[b])] = tgts[b].to(torch.int32)
    return dict(ids=out_ids, mask=out_mask, text_mask=out_tm, targets=targets, n_targets=nt)


def score_text_inputs(input_ids: torch.Tensor, attention_mask: torch.Tensor, refined, eos_token: int, append_eos: bool = True):
    """The text twin of score_inputs, host helper of GPT.score_text (CPU): utterance i's refined text ids [n_i] follow its left-padded refine prompt (input_ids
    [B, T, num_vq], attention_mask [B, T], as Tokenizer.encode gives them for the refine pass: every row a text row); the joined sequences are left padded again.
    Returns dict(ids [B, T', num_vq], mask [B, T'] int32, text_mask [B, T'] bool (True on every real row), targets [B, max_targets] int32, n_targets [B] int32).
      append_eos=True:  every refined id is an input row (the id on every column, as the refine pass feeds it back: emb_text[id]) and the targets are the ids
                        followed by `eos_token` ([Ebreak]), n_b = n_i + 1: the log-probs generate(infer_text=True, return_text_logprobs=True) wrote, final one included.
      append_eos=False: the targets are the ids, n_b = n_i; the last id is not fed as input.
    Target j of sequence b is predicted by row T' - n_b + j (ctts_gpt_score_text)."""
    ids = torch.as_tensor(input_ids).cpu()
    mask = torch.as_tensor(attention_mask).cpu().to(torch.int64)
    if ids.dim() != 3 or mask.shape != ids.shape[:2]:
        raise ValueError(f"score_text_inputs: input_ids [B, T, num_vq] with attention_mask [B, T] (got {tuple(ids.shape)}, {tuple(mask.shape)})")
    B, nvq = int(ids.shape[0]), int(ids.shape[2])
    if len(refined) != B:
        raise ValueError(f"score_text_inputs: {len(refined)} refined sequences for {B} prompts")
    _check_left_padded(mask)
    conts = []
    for b in range(B):
        c = torch.as_tensor(refined[b]).cpu().to(ids.dtype).flatten()
        if not append_eos and c.numel() < 1:
            raise ValueError(f"score_text_inputs: refined[{b}] is empty and append_eos is off: nothing to score")
        conts.append(c[:, None].expand(-1, nvq))
    out = _join_scored(ids, mask, mask.bool(), conts, eos_token, append_eos)
    return dict(out, text_mask=out["mask"].bool(), targets=out["targets"][:, :, 0].contiguous())


def _check_left_padded(mask: torch.Tensor) -> None:
    """Every row of `mask` [B, T] is 0...0 1...1 with at least one 1: no holes, no right padding."""
    m = torch.as_tensor(mask).cpu().to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        raise ValueError("attention_mask: values must be 0 or 1")
    if bool((m.sum(1) == 0).any()):
        raise ValueError("attention_mask: a sequence has no token")
    if m.shape[1] > 1 and bool((m[:, 1:] < m[:, :-1]).any()):
        raise ValueError("attention_mask: scoring needs LEFT padding (0...0 1...1 per row); a row has a hole or right padding")


class Context:                    # gpt.py:87-95
    def __init__(self):
        self._interrupt = False

    def set(self, v: bool):
        self._interrupt = v

    def get(self) -> bool:
        return self._interrupt


# The conversions of the sampling scalars, shared by the per-call configuration (sampler_cfg_from_objects) and the per-utterance knobs
# (row_sampling_from_values), so that the two cannot drift apart.
def _temperatures(temperature, num_vq: int) -> List[float]:
    t = torch.as_tensor(temperature, dtype=torch.float32).flatten().tolist()
    return t * num_vq if len(t) == 1 else t


def _top_p_threshold(top_p) -> float:
    # torch compares the fp32 cumsum with the python double (1 - top_p) cast to fp32
    return float(np.float32(1 - float(top_p)))


def _penalty_table(penalty) -> torch.Tensor:
    return torch.pow(float(penalty), torch.arange(0, 17, dtype=torch.int64))     # processors.py:28


def sampler_cfg_from_objects(temperature, eos_token, max_new_token, min_new_token, logits_warpers, logits_processors,
                             num_vq=4, infer_text=False) -> _lib.SamplerCfg:
    """Reads the scalars off the HF warpers / reference processor objects that processors.gen_logits builds
    (models/processors.py:37-57).  Unknown object types are rejected (no silent host fallback)."""
    sc = _lib.SamplerCfg()
    t = _temperatures(temperature, num_vq)
    for i in range(num_vq):
        sc.temperature[i] = t[i]
    sc.top_p_threshold = -1.0
    sc.top_k = 0
    sc.min_tokens_to_keep = 1
    # the kernel applies top-p FIRST and top-k second -- the order processors.gen_logits builds (models/processors.py:43-48) and the
    # reference's loop applies them in (gpt.py:474-475); the two do not commute, so any other list is rejected rather than re-ordered
    seen = []
    for w in logits_warpers or []:
        if hasattr(w, "top_p"):
            if seen:
                raise _lib.HipBackendError("logits_warpers: the hip sampler applies [top-p, top-k] in that order (processors.gen_logits); "
                                           f"got a top-p warper after {seen}")
            sc.top_p_threshold = _top_p_threshold(w.top_p)
            sc.min_tokens_to_keep = int(w.min_tokens_to_keep)
            seen.append("top_p")
        elif hasattr(w, "top_k"):
            if "top_k" in seen:
                raise _lib.HipBackendError("logits_warpers: more than one top-k warper")
            sc.top_k = int(w.top_k)          # already max(top_k, min_tokens_to_keep)
            seen.append("top_k")
        else:
            raise _lib.HipBackendError(f"unsupported logits warper for the hip backend: {type(w).__name__}")
    sc.use_penalty = 0
    sc.past_window = 16
    sc.max_input_ids = 1 << 30
    tab = torch.ones(17)
    for p in logits_processors or []:
        if hasattr(p, "penalty") and hasattr(p, "past_window"):
            sc.use_penalty = 1
            sc.past_window = int(p.past_window)
            sc.max_input_ids = int(p.max_input_ids)
            tab = _penalty_table(p.penalty)
        else:
            raise _lib.HipBackendError(f"unsupported logits processor for the hip backend: {type(p).__name__}")
    for i in range(17):
        sc.penalty_table[i] = float(tab[i])
    sc.eos_token = int(eos_token)
    sc.min_new_token = int(min_new_token)
    sc.max_new_token = int(max_new_token)
    sc.infer_text = 1 if infer_text else 0
    if infer_text and sc.use_penalty:
        raise _lib.HipBackendError("infer_text=True supports repetition_penalty == 1 only: the reference's processor receives a [B,n,1] "
                                   "history in this mode and mis-broadcasts it (models/processors.py:18-34 with gpt.py:458-467)")
    return sc


class _TopP:                                  # scalar carriers with the attribute names the HF warpers expose
    def __init__(self, top_p, min_tokens_to_keep):
        self.top_p, self.min_tokens_to_keep = float(top_p), int(min_tokens_to_keep)


class _TopK:
    def __init__(self, top_k, min_tokens_to_keep):
        self.top_k, self.min_tokens_to_keep = max(int(top_k), int(min_tokens_to_keep)), int(min_tokens_to_keep)


class _RepPenalty:
    def __init__(self, penalty, max_input_ids, past_window):
        if not isinstance(penalty, float) or not (penalty > 0):
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {penalty}")   # processors.py:9-12
        self.penalty, self.max_input_ids, self.past_window = penalty, int(max_input_ids), int(past_window)


def gen_logits(num_code: int, top_P=0.7, top_K=20, repetition_penalty=1.0):
    """models/processors.py:37-57 -- same construction, scalar carriers instead of HF objects (the hip GPT
    also accepts the real transformers / reference objects: it only reads their attributes)."""
    warpers, processors = [], []
    if top_P is not None:
        warpers.append(_TopP(top_P, 3))
    if top_K is not None:
        warpers.append(_TopK(top_K, 3))
    if repetition_penalty is not None and repetition_penalty != 1:
        processors.append(_RepPenalty(repetition_penalty, num_code, 16))
    return warpers, processors


SAMPLING_KEYS = ("temperature", "top_P", "top_K", "repetition_penalty", "min_new_token", "past_window")


def row_sampling_from_values(base: _lib.SamplerCfg, entry=None, num_vq: int = 4) -> _lib.RowSampling:
    """One utterance's sampling knobs (ctts_row_sampling) = the call's configuration `base` (sampler_cfg_from_objects) with the overrides of
    `entry`, a dict with keys among SAMPLING_KEYS (None: the call's values).  The entry's knobs take the very path of a call's: gen_logits builds
    their objects, sampler_cfg_from_objects reads them -- temperature a scalar or num_vq values; top_P (None = disabled), top_K (None = disabled)
    and repetition_penalty (None or 1 = off) as gen_logits takes them; past_window (1..16, default 16); min_new_token."""
    e = dict(entry or {})
    bad = sorted(set(e) - set(SAMPLING_KEYS))
    if bad:
        raise _lib.HipBackendError(f"sampling_per_row: unknown key(s) {bad}; per-utterance keys are {list(SAMPLING_KEYS)}")
    if "temperature" in e and len(_temperatures(e["temperature"], num_vq)) != num_vq:
        raise _lib.HipBackendError(f"sampling_per_row: temperature has {len(_temperatures(e['temperature'], num_vq))} values (1 or {num_vq})")
    if e.get("top_K") is not None and int(e["top_K"]) < 0:
        raise _lib.HipBackendError(f"sampling_per_row: top_K = {e['top_K']} < 0 (None disables top-k)")
    pen = e.get("repetition_penalty")
    if pen is not None and not (float(pen) > 0):
        raise _lib.HipBackendError(f"sampling_per_row: repetition_penalty = {pen} (must be > 0)")
    w, p = gen_logits(0, top_P=e.get("top_P"), top_K=e.get("top_K"), repetition_penalty=None if pen is None else float(pen))
    c = sampler_cfg_from_objects(e.get("temperature", 1.0), 0, 0, 0, w, p, num_vq)
    src = {k: (c if k in e else base) for k in ("temperature", "top_P", "top_K", "repetition_penalty")}
    r = _lib.RowSampling()
    for i in range(num_vq):
        r.temperature[i] = src["temperature"].temperature[i]
    r.top_p_threshold, r.min_tokens_to_keep = src["top_P"].top_p_threshold, src["top_P"].min_tokens_to_keep
    r.top_k = src["top_K"].top_k
    r.use_penalty, r.past_window = src["repetition_penalty"].use_penalty, src["repetition_penalty"].past_window
    for i in range(17):
        r.penalty_table[i] = src["repetition_penalty"].penalty_table[i]
    if "past_window" in e:
        r.past_window = int(e["past_window"])
    r.min_new_token = int(e["min_new_token"]) if "min_new_token" in e else base.min_new_token
    return r


def row_sampling_array(base: _lib.SamplerCfg, entries, n: int, num_vq: int = 4, infer_text: bool = False):
    """ctypes array [n] of ctts_row_sampling for `entries` (one dict or None per sequence); the engine checks the values (begin / admit_sampling)."""
    if infer_text:
        raise _lib.HipBackendError("sampling_per_row: per-utterance sampling parameters are code mode only (the refine-text pass, infer_text=True, keeps the call's values)")
    entries = list(entries)
    if len(entries) != n:
        raise _lib.HipBackendError(f"sampling_per_row: {len(entries)} entries for {n} sequences")
    return (_lib.RowSampling * n)(*[row_sampling_from_values(base, e, num_vq) for e in entries])


def prompt_groups(prompt_of, n_prompts: int, slots=None, subset=None, n=None, infer_text: bool = False):
    """Index bookkeeping of shared prompt passes (ctts_gpt_share_prompts): `prompt_of[i]` in [0, n_prompts) names the prompt of sequence i.  For the sequences
    `subset` (indices into prompt_of, in seating order; None = all of them) that one begin / admit call seats, returns (prompts, local, leaders):
      prompts   the prompts the subset names, in order of first use -- the rows of emb / mask the call passes
      local     the subset's prompt_of re-indexed into `prompts` (what ctts_gpt_share_prompts takes)
      leaders   per entry of `prompts` the position in the subset of the first sequence naming it: it runs the prompt pass, the others receive a copy.
    Raises HipBackendError on what the engine refuses: a length that differs from the call's `n`, an index out of range, a prompt named by no sequence (checked on
    the whole list), infer_text, and sequences of one group with different adapter `slots` (one per sequence; -1 / None = none)."""
    prompt_of = [int(p) for p in prompt_of]
    n_prompts = int(n_prompts)
    if n is not None and len(prompt_of) != int(n):
        raise _lib.HipBackendError(f"prompt_of: {len(prompt_of)} entries for {int(n)} sequences")
    if infer_text:
        raise _lib.HipBackendError("prompt_of: shared prompt passes are code mode only; the refine-text pass (infer_text=True) runs every prompt")
    for i, p in enumerate(prompt_of):
        if not 0 <= p < n_prompts:
            raise _lib.HipBackendError(f"prompt_of[{i}]={p} is out of range: the call has {n_prompts} prompts")
    missing = sorted(set(range(n_prompts)) - set(prompt_of))
    if missing:
        raise _lib.HipBackendError(f"prompt_of: prompt {missing[0]} is named by no sequence")
    if slots is not None and len(slots) != len(prompt_of):
        raise _lib.HipBackendError(f"prompt_of: {len(slots)} adapter slots for {len(prompt_of)} sequences")
    sub = list(range(len(prompt_of))) if subset is None else [int(i) for i in subset]
    prompts, local, leaders, where = [], [], [], {}
    for j, i in enumerate(sub):
        p = prompt_of[i]
        if p not in where:
            where[p] = len(prompts)
            prompts.append(p)
            leaders.append(j)
        elif slots is not None:
            a, b = slots[sub[leaders[where[p]]]], slots[i]
            a, b = (-1 if a is None or int(a) < 0 else int(a)), (-1 if b is None or int(b) < 0 else int(b))
            if a != b:
                raise _lib.HipBackendError(f"prompt_of: sequences {sub[leaders[where[p]]]} and {i} share prompt {p} but carry different adapter slots ({a}, {b}); "
                                           "the prompt pass depends on the adapter: a group shares one slot or none")
        local.append(where[p])
    return prompts, local, leaders


def compact_size(n_live: int) -> int:
    """Decode-batch size used for `n_live` unfinished sequences (finished-row compaction, ctts_gpt_compact): every size up to 16, then
    multiples of 2 up to 32, of 4 up to 64, of 8 beyond -- a captured decode graph exists per batch size, so the sizes are quantised;
    the padding rows are finished sequences left in the batch."""
    n = max(int(n_live), 1)
    if n <= 16:
        return n
    q = 2 if n <= 32 else (4 if n <= 64 else 8)
    return (n + q - 1) // q * q


def compact_keep(live) -> Optional[List[int]]:
    """The one compaction rule (generate() and SessionBook.plan; each has its own threshold for asking): `live[r]` = decode row r still decodes.  Returns the rows
    to keep, ascending -- the live ones and, up to compact_size of their number, the first finished ones as padding -- or None when the batch stays as it is."""
    rows = [r for r, f in enumerate(live) if f]
    target = compact_size(len(rows))
    if not rows or target >= len(live):
        return None
    return sorted(rows + [r for r, f in enumerate(live) if not f][:target - len(rows)])


class RowBook:
    """Continuous batching bookkeeping (the row level of SessionBook): which utterance sits in which decode row.  Every seating gets a ticket; the row
    states the engine reports ({fin, end} per row, ctts_gpt_rows_enqueue) arrive one or two chunks late and are interpreted through the
    ticket layout that was current when the report was ENQUEUED -- a report taken before an admission or a compaction can neither finish the
    row's new occupant nor be confused by rows having moved."""

    def __init__(self):
        self.row_tk: List[Optional[int]] = []      # ticket per current decode row (None: the row's utterance is done, the row is free)
        self.tickets = {}                          # live ticket -> [utterance, attempt, current row]
        self._next = 0

    def seat(self, row: int, utt: int, attempt: int = 0) -> int:
        tk = self._next
        self._next += 1
        if row == len(self.row_tk):
            self.row_tk.append(tk)
        else:
            assert self.row_tk[row] is None, "seat: the row is occupied"
            self.row_tk[row] = tk
        self.tickets[tk] = [utt, attempt, row]
        return tk

    def layout(self) -> list:
        return list(self.row_tk)

    def free_rows(self) -> List[int]:
        return [r for r, tk in enumerate(self.row_tk) if tk is None]

    def live_rows(self) -> List[int]:
        return [r for r, tk in enumerate(self.row_tk) if tk is not None]

    def report(self, layout, states, ensure_non_empty: bool, max_restarts: int):
        """`states` = [(fin, end)] per row of `layout`.  Returns ([(utterance, tokens generated)] completed, [(utterance, next attempt)] to admit
        again: their first token was EOS, gpt.py:496-525)."""
        done, again = [], []
        for tk, (fin, end) in zip(layout, states):
            if tk is None or not fin or tk not in self.tickets:
                continue
            utt, att, row = self.tickets.pop(tk)
            self.row_tk[row] = None
            if (fin & 2) and end == 0 and ensure_non_empty and att + 1 < max_restarts:
                again.append((utt, att + 1))
            else:
                done.append((utt, int(end)))
        return done, again

    def compact(self, keep: List[int]) -> None:
        """rows `keep` (ascending) become rows 0..len(keep)-1 (ctts_gpt_compact)"""
        self.row_tk = [self.row_tk[r] for r in keep]
        for nr, tk in enumerate(self.row_tk):
            if tk is not None:
                self.tickets[tk][2] = nr


class SessionPlan:
    """What DecodeSession.step does to the decode batch next (SessionBook.plan): `begin` / `admit` = [(row, ticket)], `grow` = rows to append first
    (ctts_gpt_grow), `lanes` = the KV lanes those rows get (the engine picks the same ones), `compact` = rows to keep (ctts_gpt_compact) or None."""

    def __init__(self, begin=(), grow=0, lanes=(), admit=(), compact=None):
        self.begin, self.grow, self.lanes, self.admit, self.compact = list(begin), int(grow), list(lanes), list(admit), compact

    def __bool__(self):
        return bool(self.begin or self.grow or self.admit or self.compact is not None)


class SessionBook:
    """Bookkeeping of continuous batching (DecodeSession: GPT.open_session and GPT.generate_many), pure Python: tickets, the queue, which output slot an
    utterance writes to and when the slot is free again, the mirror of the decode rows' KV lanes, and the decision what to do with the batch next -- seat queued
    utterances in free rows, then in rows obtained by growing the batch up to `rows`, else (nothing queued) shrink it by the compact_size rule.  Row reports are
    interpreted by a RowBook, whose "utterance" is the session ticket.

    The policy of a request that is known in full (generate_many), off by default:
      own_slots   ticket k writes output slot k, also when ensure_non_empty seats it again: slots are never recycled (release() frees none), the queue alone bounds
                  plan(), and the batch opens at min(queued, rows) rows and never grows
      admit_min   free rows are held back until an admission pays for its prompt pass: with `free` the free rows of the B current ones and `since_free` the plans
                  in a row that saw a free row, queued utterances are seated only if len(free) >= min(admit_min, queued), since_free >= 4 or len(free) == B; a
                  held-back plan is empty (no compaction while something is queued).  1 = seat at once.

    Streaming (submit(stream="exact" | "eager")): every row report carries the live rows' token counts, and from them the book derives the sample windows
    that are due (take_windows): (ticket, slot, tokens seen, s0, s1, final).  The windows of a ticket are consecutive and disjoint; the final one comes with
    the utterance's completion or cancel and carries everything not yet emitted (it may be empty).
      exact   s1 = settled_samples(tokens seen): the samples no later token can change, so the concatenation IS the finished utterance's waveform; a window
              is due once `stream_batch` tokens' worth (2 hop samples a token) of newly settled samples exist
      eager   the rule of infer(stream=True, continuous=True): once `stream_batch` new tokens exist, the window runs to the end of the PREFIX waveform, at
              most `stream_speed` samples -- the reference's semantics: a window's tail is computed against the zero padding behind the prefix"""

    def __init__(self, rows: int, out_slots: int, max_batch: int, max_seq: int, max_new_token: int, ensure_non_empty: bool = True, max_restarts: int = 64,
                 compact: bool = True, max_new_text: Optional[int] = None, stream_batch: int = 24, stream_speed: int = 12000, hop: int = 256,
                 halo_frames: int = 105, own_slots: bool = False, admit_min: int = 1):
        if not (1 <= int(rows) <= int(max_batch)):
            raise ValueError(f"session: rows={rows} outside 1..max_batch={max_batch}")
        if int(out_slots) < 1:
            raise ValueError(f"session: out_slots={out_slots} (at least one)")
        self.rows, self.max_batch, self.max_seq, self.max_new = int(rows), int(max_batch), int(max_seq), int(max_new_token)
        self.ensure_non_empty, self.max_restarts, self.compact = bool(ensure_non_empty), int(max_restarts), bool(compact)
        # text utterances (mode "text": refine-text rows beside the code rows) have a token limit of their own, at most the code rows'; None = the session serves none
        if max_new_text is not None and not (1 <= int(max_new_text) <= self.max_new):
            raise ValueError(f"session: the text rows' max_new_token={max_new_text} must be 1..max_new_token={self.max_new} of the code rows")
        self.max_new_text = None if max_new_text is None else int(max_new_text)
        self.book = RowBook()
        self.lanes: List[int] = []                 # KV lane of every current decode row (the engine's row_seq)
        self.own_slots, self.admit_min, self._since_free = bool(own_slots), max(1, int(admit_min)), 0
        self.free_slots = [] if self.own_slots else list(range(int(out_slots)))
        self.live: List[tuple] = []                # (ticket, tokens so far) of the rows the last report showed decoding
        self.queue: List[int] = []                 # tickets waiting for a row (and an output slot), in order of service
        self.utts = {}                             # ticket -> dict(utt_id, T, limit, attempt, slot, row_tk, cancelled, mode)
        self.begun = False
        self._next = 0
        self._to_cancel: List[int] = []            # seated tickets whose cancel the device has not seen yet
        self._dropped: List[int] = []              # tickets cancelled while queued: delivered by the next step
        if int(stream_batch) < 1 or int(stream_speed) < 1:
            raise ValueError(f"session: stream_batch={stream_batch} / stream_speed={stream_speed} (at least 1)")
        self.stream_batch, self.stream_speed, self.hop, self.halo_frames = int(stream_batch), int(stream_speed), int(hop), int(halo_frames)
        self._windows: List[tuple] = []            # windows the reports made due since the last take_windows()
        self._lookback = {}                        # ticket -> stream_lookback (kept until its final window is built: the ticket itself is released first)

    # -- requests ---------------------------------------------------------------------------------
    def submit(self, T: int, utt_id: int, limit: Optional[int] = None, mode: str = "code", stream: Optional[str] = None, stream_batch: Optional[int] = None,
               stream_lookback: int = 0) -> int:
        """`stream_lookback` (stream="exact" only): samples before each window's s0 that its consumer reads again -- a resampler's left taps; the windows stay
        the same (s0, s1), DecodeSession vocodes them from max(0, s0 - stream_lookback) (SessionWindow.v0).
        `mode` "code" or "text": a text utterance takes a row, a KV lane and an output slot like a code utterance (one index space: a slot is held by one
        utterance of either kind); only its token limit is the text rows' own.  `stream` None, "exact" or "eager" (code utterances): sample windows become due
        while it decodes; `stream_batch` defaults to the session's"""
        T = int(T)
        if mode not in ("code", "text"):
            raise ValueError(f"submit: mode={mode!r} (\"code\" or \"text\")")
        if stream not in (None, "exact", "eager"):
            raise ValueError(f"submit: stream={stream!r} (None, \"exact\" or \"eager\")")
        if stream is not None and mode == "text":
            raise ValueError("submit: stream= is for code utterances; a text row produces no audio")
        if stream_batch is not None and (stream is None or int(stream_batch) < 1):
            raise ValueError(f"submit: stream_batch={stream_batch} needs stream= and a value of at least 1")
        if int(stream_lookback) < 0 or (int(stream_lookback) > 0 and stream != "exact"):
            raise ValueError(f"submit: stream_lookback={stream_lookback} needs stream=\"exact\" and a value of at least 0")
        if mode == "text" and self.max_new_text is None:
            raise ValueError("submit: mode=\"text\" needs a session opened with text_rows=...")
        if T < 1 or T + self.max_new > self.max_seq:
            raise ValueError(f"submit: prompt of {T} tokens + max_new_token={self.max_new} exceed max_seq_len={self.max_seq}")
        cap = self.max_new_text if mode == "text" else self.max_new
        lim = cap if limit is None else min(max(int(limit), 1), cap)
        tk = self._next
        self._next += 1
        self.utts[tk] = dict(utt_id=int(utt_id), T=T, limit=lim, attempt=0, slot=None, row_tk=None, cancelled=False, mode=mode, stream=stream,
                             stream_batch=self.stream_batch if stream_batch is None else int(stream_batch), emitted=0, last_n=0)
        if int(stream_lookback) > 0:
            self._lookback[tk] = int(stream_lookback)
        self.queue.append(tk)
        return tk

    def cancel(self, tk: int) -> Optional[str]:
        """"queued": dropped at once (the next step delivers an empty result); "seated": the device cancels it at the next step boundary; None: unknown, already
        delivered or already cancelled"""
        u = self.utts.get(tk)
        if u is None or u["cancelled"]:
            return None
        u["cancelled"] = True
        if tk in self.queue:
            self.queue.remove(tk)
            self._dropped.append(tk)
            return "queued"
        self._to_cancel.append(tk)
        return "seated"

    def cancel_rows(self) -> List[int]:
        """current rows of the seated tickets cancelled since the last call (for ctts_gpt_cancel)"""
        rows = sorted(self.book.tickets[self.utts[tk]["row_tk"]][2] for tk in self._to_cancel
                      if tk in self.utts and self.utts[tk]["row_tk"] in self.book.tickets)
        self._to_cancel = []
        return rows

    def take_dropped(self) -> List[int]:
        out, self._dropped = self._dropped, []
        for tk in out:                             # a streaming ticket cancelled while queued ends with an empty final window
            if self.utts[tk].get("stream"):
                self._windows.append((tk, None, 0, 0, 0, True))
        return out

    def window_v0(self, tk: int, s0: int, final: bool = False) -> int:
        """First sample to vocode for the window of ticket `tk` that starts at s0: max(0, s0 - stream_lookback), s0 itself without a lookback.  `final`: the
        ticket's last window -- its lookback is forgotten."""
        back = self._lookback.pop(tk, 0) if final else self._lookback.get(tk, 0)
        return max(0, int(s0) - back)

    def take_windows(self) -> List[tuple]:
        """[(ticket, slot, tokens seen, s0, s1, final)] made due since the last call, in report order"""
        out, self._windows = self._windows, []
        return out

    def _progress(self, tk: int, n: int) -> None:
        """a live streaming utterance was reported with n tokens written: book the window that is due, if any"""
        from .vocoder import settled_samples
        u = self.utts[tk]
        n, s0 = int(n), u["emitted"]
        if u["stream"] == "exact":
            s1 = settled_samples(n, self.hop, self.halo_frames)
            if s1 - s0 < u["stream_batch"] * 2 * self.hop:
                return
        else:
            total = self.hop * (2 * n - 1) if n > 0 else 0
            if total <= s0 or n - u["last_n"] < u["stream_batch"]:
                return
            s1 = min(s0 + self.stream_speed, total)
        self._windows.append((tk, u["slot"], n, s0, s1, False))
        u["emitted"], u["last_n"] = s1, n

    def _final(self, tk: int, n: int) -> None:
        u = self.utts[tk]
        if u.get("stream"):
            total = self.hop * (2 * int(n) - 1) if n > 0 else 0
            self._windows.append((tk, u["slot"], int(n), min(u["emitted"], total), total, True))
            u["emitted"] = total

    def n_live(self) -> int:
        return len(self.book.tickets)

    def idle(self) -> bool:
        return not self.queue and not self.book.tickets and not self._dropped

    # -- the batch -----------------------------------------------------------------------------------
    def free_lanes(self) -> List[int]:
        used = set(self.lanes)
        return [l for l in range(self.max_batch) if l not in used]

    def _seat(self, row: int, tk: int) -> None:
        u = self.utts[tk]
        u["slot"] = tk if self.own_slots else self.free_slots.pop(0)
        u["row_tk"] = self.book.seat(row, tk, u["attempt"])

    def _unseat(self, u: dict) -> None:
        if u["slot"] is not None and not self.own_slots:
            self.free_slots.append(u["slot"])
            self.free_slots.sort()
        u["slot"] = None

    def plan(self) -> SessionPlan:
        """Decides and books the next change of the batch; the caller carries it out in the order begin | grow, admit | compact."""
        k = len(self.queue) if self.own_slots else min(len(self.queue), len(self.free_slots))
        if not self.begun:
            k = min(k, self.rows)
            if k == 0:
                return SessionPlan()
            take, self.queue = self.queue[:k], self.queue[k:]
            for r, tk in enumerate(take):
                self._seat(r, tk)
                assert self.utts[tk]["slot"] == r      # ctts_gpt_begin writes row r's outputs at index r
            self.lanes = list(range(k))
            self.begun = True
            return SessionPlan(begin=list(enumerate(take)))
        B = len(self.book.row_tk)
        free = self.book.free_rows()
        self._since_free = self._since_free + 1 if free else 0
        if k > 0:
            grow = 0 if self.own_slots else max(0, min(k - len(free), self.rows - B))
            k = min(k, len(free) + grow)
            if k == 0 or not (grow or len(free) >= min(self.admit_min, len(self.queue)) or self._since_free >= 4 or len(free) == B):
                return SessionPlan()
            self._since_free = 0
            lanes = self.free_lanes()[:grow]           # lowest first: after a compaction these are not B ..
            self.lanes += lanes
            rows = free[:k - grow] + list(range(B, B + grow))
            take, self.queue = self.queue[:k], self.queue[k:]
            for r, tk in zip(rows, take):
                self._seat(r, tk)
            return SessionPlan(grow=grow, lanes=lanes, admit=list(zip(rows, take)))
        if not self.queue and self.compact and B >= 2:
            keep = compact_keep([tk is not None for tk in self.book.row_tk])
            if keep is not None:
                self.book.compact(keep)
                self.lanes = [self.lanes[r] for r in keep]
                return SessionPlan(compact=keep)
        return SessionPlan()

    def report(self, layout, states):
        """One row report ([(fin, end)] per row of `layout`, RowBook.report).  Returns [(ticket, tokens, fin bits, cancelled)] of the utterances that ended; those
        whose first token was EOS go back to the head of the queue with their next attempt (a cancelled one ends instead).  The caller clones the results out
        of slot utts[ticket]["slot"] and then calls release(ticket).  `live` = [(ticket, tokens so far)] of the rows this report showed still decoding."""
        fin_of = {self.book.tickets[t][0]: int(fin) for t, (fin, end) in zip(layout, states) if t is not None and fin and t in self.book.tickets}
        self.live = [(self.book.tickets[t][0], int(end)) for t, (fin, end) in zip(layout, states) if t is not None and not fin and t in self.book.tickets]
        for tk, n in self.live:                    # live rows of streaming utterances: the windows their token counts make due
            if self.utts[tk].get("stream"):
                self._progress(tk, n)
        done, again = self.book.report(layout, states, self.ensure_non_empty, self.max_restarts)
        out, back = [], []
        for tk, att in again:
            u = self.utts[tk]
            if u["cancelled"]:
                self._final(tk, 0)
                out.append((tk, 0, 1, True))
                continue
            u["attempt"], u["row_tk"] = att, None
            u["emitted"], u["last_n"] = 0, 0           # (its first token was EOS: nothing was emitted; the next attempt starts over)
            self._unseat(u)
            back.append(tk)
        self.queue = back + self.queue
        for tk, n in done:
            u = self.utts[tk]
            fin = fin_of.get(tk, 1)
            self._final(tk, n)
            out.append((tk, n, fin, bool(u["cancelled"] and not (fin & 2) and n < u["limit"])))
        return out

    def release(self, tk: int) -> None:
        """the utterance's result has been cloned out: its output slot may be written again"""
        self._unseat(self.utts.pop(tk))


# arguments of generate() / generate_many() / infer() that a session refuses by name (GPT.open_session, ChatTTSPlusPipeline.open_session)
SESSION_OUT_OF_SCOPE = {"prompt_of": "shared prompt passes", "share_prompt": "shared prompt passes", "num_candidates": "num_candidates / shared prompt passes",
                        "refine_candidates": "ranked refine candidates",
                        "noise": "caller-supplied noise", "stream": "session-wide streaming windows", "stream_batch": "session-wide streaming windows",
                        "sharded": "infer_sharded", "infer_text": "the refine-text pass inside a code session",
                        "refine_text_only": "the refine-text pass inside a code session", "params_refine_text": "the refine-text pass inside a code session"}


def refuse_out_of_scope(kw: dict, instead: str) -> None:
    """open_session(**kw): a name outside SESSION_OUT_OF_SCOPE is a TypeError as for any function; a named one that asks for the feature (not None / False, not
    the values that mean "off": noise="device", num_candidates=1) is refused with the reason"""
    for name, value in kw.items():
        if name not in SESSION_OUT_OF_SCOPE:
            raise TypeError(f"open_session() got an unexpected keyword argument {name!r}")
        off = value is None or value is False or (name == "noise" and isinstance(value, str) and value == "device") or \
            (name in ("num_candidates", "refine_candidates") and isinstance(value, int) and value == 1)
        if not off:
            per_utt = "; streaming is asked per utterance at submit(stream=\"exact\" | \"eager\")" if name in ("stream", "stream_batch") else ""
            raise _lib.HipBackendError(f"open_session: {SESSION_OUT_OF_SCOPE[name]} ({name}=) is not offered inside a session; {instead}{per_utt}")


TEXT_ROWS_KEYS = ("temperature", "top_P", "top_K", "eos_token", "max_new_token", "min_new_token")


def text_rows_cfg(text_rows, num_vq: int = 4) -> _lib.SamplerCfg:
    """open_session(text_rows=...): the refine pass's sampler configuration (infer_text = 1) from a dict or an object carrying TEXT_ROWS_KEYS -- built the way
    generate(infer_text=True) builds its own: gen_logits for top_P / top_K (no repetition penalty in this mode), sampler_cfg_from_objects for the rest"""
    if isinstance(text_rows, dict):
        bad = sorted(set(text_rows) - set(TEXT_ROWS_KEYS) - {"guide"})      # ("guide": a TextGuide, read by open_session itself)
        if bad:
            raise _lib.HipBackendError(f"open_session: text_rows: unknown key(s) {bad}; the keys are {list(TEXT_ROWS_KEYS)}")
        get = text_rows.get
    else:
        def get(k, d=None):
            return getattr(text_rows, k, d)
    if get("eos_token") is None or get("max_new_token") is None:
        raise _lib.HipBackendError("open_session: text_rows needs eos_token ([Ebreak]) and max_new_token")
    w, p = gen_logits(0, top_P=get("top_P", 0.7), top_K=get("top_K", 20), repetition_penalty=None)
    t = get("temperature", 0.7)
    return sampler_cfg_from_objects(0.7 if t is None else t, int(get("eos_token")), int(get("max_new_token")), int(get("min_new_token", 0) or 0), w, p, num_vq, infer_text=True)


# -- guided refine-text (include/ctts_hip.h "Guided refine-text"): the host side of the contract, pure Python ------------------------------------------------------
GUIDE_MAX_FREE, GUIDE_MAX_SRC, GUIDE_SLOTS = 64, 1020, 1024


class TextGuide:
    """The per-call part of a guide: `free_ids` (at most 64 distinct token ids the model may insert between source tokens -- [uv_break], [laugh], ...) and
    `max_run`, the most consecutive free tokens allowed.  A guided text row emits its source ids in order, free ids interleaved, then EOS."""

    def __init__(self, free_ids, max_run: int = 2):
        ids = [int(i) for i in free_ids]
        if len(ids) > GUIDE_MAX_FREE:
            raise _lib.HipBackendError(f"TextGuide: {len(ids)} free ids (at most {GUIDE_MAX_FREE})")
        if len(set(ids)) != len(ids):
            raise _lib.HipBackendError("TextGuide: a free id is listed twice")
        if any(i < 0 for i in ids):
            raise _lib.HipBackendError("TextGuide: negative free id")
        if int(max_run) < 0:
            raise _lib.HipBackendError(f"TextGuide: max_run={max_run} (must be >= 0)")
        self.free_ids, self.max_run = tuple(ids), int(max_run)

    def check(self, eos: int, vocab: int, who: str = "text_guide") -> None:
        """the refusals that need the call: a free id equal to EOS or outside the text vocabulary"""
        for i in self.free_ids:
            if i == int(eos):
                raise _lib.HipBackendError(f"{who}: free id {i} is the EOS token (the guide ends a row by EOS alone)")
            if i >= int(vocab):
                raise _lib.HipBackendError(f"{who}: free id {i} outside 0..{int(vocab) - 1}")

    def __repr__(self):
        return f"TextGuide(free_ids={list(self.free_ids)}, max_run={self.max_run})"


def check_guide_src(src, limit: int, eos: int, vocab: int, who: str = "guide_src") -> List[int]:
    """One utterance's source ids as a list, or the refusal: empty, longer than the table's record, n + 1 > the row's limit, an id out of range or the EOS"""
    ids = [int(i) for i in (src.tolist() if hasattr(src, "tolist") else src)]
    n = len(ids)
    if n < 1:
        raise _lib.HipBackendError(f"{who}: an empty source (n == 0); pass None for an unguided utterance")
    if n > GUIDE_MAX_SRC:
        raise _lib.HipBackendError(f"{who}: a source of {n} ids (at most {GUIDE_MAX_SRC})")
    if n + 1 > int(limit):
        raise _lib.HipBackendError(f"{who}: a source of {n} ids needs {n + 1} tokens (the source and EOS), the row's limit is {int(limit)}")
    for i in ids:
        if i < 0 or i >= int(vocab):
            raise _lib.HipBackendError(f"{who}: source id {i} outside 0..{int(vocab) - 1}")
        if i == int(eos):
            raise _lib.HipBackendError(f"{who}: source id {i} is the EOS token")
    return ids


def guide_free_ok(cur: int, run: int, t: int, limit: int, n: int, max_run: int) -> bool:
    """May the row insert a free token at its own step t?  Only while the source still to come and the EOS fit behind it"""
    if run >= max_run:
        return False
    if cur < n:
        return (limit - t) - ((n - cur) + 1) > 0          # slack > 0
    return limit - t > 1


def guide_standin(cur: int, n: int, src, eos: int) -> int:
    """the id the automaton needs next: what the race returns when every ratio is 0 or NaN"""
    return int(src[cur]) if cur < n else int(eos)


def guide_allowed(cur: int, run: int, t: int, limit: int, n: int, max_run: int, src, free_ids, eos: int) -> List[int]:
    """The allowed set A of the row's step t, ascending: {src[cur]} (EOS once the source is out) plus the free set while guide_free_ok"""
    a = {guide_standin(cur, n, src, eos)}
    if guide_free_ok(cur, run, t, limit, n, max_run):
        a.update(int(f) for f in free_ids)
    return sorted(a)


def guide_eos_removable(cur: int, run: int, t: int, limit: int, n: int, max_run: int, free_ids) -> bool:
    """The min_new_token rule removes EOS only while another element of A remains (EOS is in A only once the source is out)"""
    return len(free_ids) > 0 and guide_free_ok(cur, run, t, limit, n, max_run)


def guide_step(cur: int, run: int, t: int, limit: int, n: int, max_run: int, idx: int, src=None, eos: int = -1):
    """The automaton's update after the draw of `idx` at step t: (cur, run, finished).  A source match takes precedence when src[cur] is also a free id."""
    if cur < n and int(idx) == int(src[cur]):
        return cur + 1, 0, False
    if int(idx) == int(eos):
        return cur, run, True
    return cur, run + 1, False


def resolve_guides(text_guide, guide_src, n: int, infer_text: bool, eos: int, vocab: int, limits, who: str = "generate"):
    """generate*(text_guide=, guide_src=): the sources per sequence (a list of n lists / None), or None when the call has no guide.  Refused here: a guide on a code
    call, sources without the per-call part, a wrong count, and per sequence what check_guide_src refuses against the sequence's own limit."""
    if text_guide is None:
        if guide_src is not None and any(s is not None for s in guide_src):
            raise _lib.HipBackendError(f"{who}: guide_src without text_guide (guides without the per-call part): pass text_guide=TextGuide(free_ids, max_run)")
        return None
    if not isinstance(text_guide, TextGuide):
        raise _lib.HipBackendError(f"{who}: text_guide must be a TextGuide")
    if not infer_text:
        raise _lib.HipBackendError(f"{who}: text_guide is for the refine-text pass (infer_text=True); a guide on a code row is not offered")
    text_guide.check(eos, vocab, who)
    srcs = [None] * n if guide_src is None else list(guide_src)
    if len(srcs) != n:
        raise _lib.HipBackendError(f"{who}: guide_src has {len(srcs)} entries for {n} sequences")
    return [None if s is None else check_guide_src(s, limits[i], eos, vocab, f"{who}: guide_src[{i}]") for i, s in enumerate(srcs)]


def guide_arrays(slots, srcs):
    """(out_slots, src_concat, src_off) int32 arrays of one ctts_gpt_set_guides call; srcs[i] None / empty = slot i is unguided (a fresh, empty record)"""
    off, cat = [0], []
    for s in srcs:
        cat.extend([] if s is None else [int(i) for i in s])
        off.append(len(cat))
    return (np.ascontiguousarray(slots, dtype=np.int32), np.ascontiguousarray(cat if cat else [0], dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32))


@dataclass(repr=False, eq=False)
class SessionResult:
    """One utterance a DecodeSession delivered: clones, independent of the session's output buffers (a request's driver, whose output slots are never rewritten,
    hands out views)."""
    ticket: int
    utt_id: int
    ids: torch.Tensor
    hiddens: Optional[torch.Tensor] = None
    logprobs: Optional[torch.Tensor] = None
    sampled_logprobs: Optional[torch.Tensor] = None
    final_logprobs: Optional[torch.Tensor] = None
    finished_by_eos: bool = False
    cancelled: bool = False
    attempt: int = 0              # first-token-EOS regenerations before this result (ensure_non_empty)
    mode: str = "code"            # "text": a refine-text utterance -- ids is [n] (as generate(infer_text=True) returns them), no hiddens; log-probs [n] / [n] / [2]
                                  #   only where the session was opened with return_text_logprobs (return_logprobs stays code-only)


@dataclass(repr=False, eq=False)
class SessionWindow:
    """One sample window of a streaming utterance that a DecodeSession.step made due (take_windows): samples [s0, s1) of the waveform, to be vocoded from tokens
    tok0 .. tok0 + len(ids) -- the receptive field of the window and no more.  `hiddens` / `ids` are VIEWS of the session's output slot while the utterance is
    live (it holds the slot, and rows below n_tokens are written once; use them on the session's stream, behind the decode launches, before the next step) and
    the delivered result's clones for the final window."""
    ticket: int
    n_tokens: int                 # tokens the row report showed (eager: the prefix whose waveform the window is a slice of)
    s0: int
    s1: int
    final: bool
    tok0: int
    ids: torch.Tensor             # int32 [k, 4]
    hiddens: Optional[torch.Tensor] = None
    cancelled: bool = False       # (final windows) the utterance was cancelled
    mode: str = "exact"
    v0: int = -1                  # first sample to vocode: max(0, s0 - stream_lookback), the tokens cover [v0, s1); s0 without a lookback

    def __post_init__(self):
        if self.v0 < 0:
            self.v0 = self.s0


class OutBuffers:
    """The output buffers of a generate state, indexed [output slot][token] -- ids, hiddens, the (raw, sampled) log-probs laid out like ids, the text rows' ids of
    a session, finish / end_idx per slot -- and the GenIO that names them.  Uninitialised: only [s, :end_idx[s]] is ever read, and every one of those rows was
    written by the step that produced it (the default max_new_token = 2048 made zero-filling a 201 MB write per call at batch 32)."""

    def __init__(self, n: int, max_new: int, gpt: "GPT", hidden: bool, logprobs: bool, text_new: Optional[int] = None, text_logprobs: bool = False,
                 infer_text: bool = False):
        """`text_logprobs`: the text rows' (raw, sampled) log-probs [2, n, steps], one value per step, beside the text ids: steps = `text_new` for the text rows of
        a code state, `max_new` for a state whose own mode is `infer_text`; a code state without text rows has none"""
        dev, NVQ = gpt.device, gpt.num_vq
        t_steps = text_new if text_new else (max_new if infer_text else None)
        self.tlps = torch.empty(2, n, t_steps, dtype=torch.float32, device=dev) if (text_logprobs and t_steps) else None
        self.ids = torch.empty(n, max_new, NVQ, dtype=torch.int32, device=dev)
        self.hid = torch.empty(n, max_new, gpt.model_dim, dtype=torch.float32, device=dev) if hidden else None
        self.lps = torch.empty(2, n, max_new, NVQ, dtype=torch.float32, device=dev) if logprobs else None
        self.tids = torch.empty(n, text_new, NVQ, dtype=torch.int32, device=dev) if text_new else None
        self.finish = torch.zeros(n, dtype=torch.int32, device=dev)
        self.end_idx = torch.zeros(n, dtype=torch.int32, device=dev)

    def io(self, n_draws: int, seed: int, utt_ids=None, row_limits=None, noise=None) -> _lib.GenIO:
        """`utt_ids` / `row_limits`: numpy arrays the caller keeps alive over the begin call"""
        return _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr() if self.hid is not None else None, finish=self.finish.data_ptr(),
                          end_idx=self.end_idx.data_ptr(), noise=noise.data_ptr() if noise is not None else None, n_draws=int(n_draws), seed=int(seed),
                          utt_ids=utt_ids.ctypes.data if utt_ids is not None else None, row_limits=row_limits.ctypes.data if row_limits is not None else None)

    def take(self, s: int, n: int, eos: bool, first_column: bool = False, text_row: bool = False):
        """(ids, hiddens, logprobs, sampled_logprobs, final_logprobs) of slot s's first n tokens: the ids as long (gpt.py:295-297), the rest views, None what the
        state does not return.  `first_column`: ids [n] of a refine-text state (gpt.py:298-299); `text_row`: those of a session's text row.  The step that sampled
        EOS wrote its log-probs at index n (its ids are not part of the sequence): final_logprobs, a clone, where `eos` says so and the row exists."""
        t = self.tlps
        tl = (None, None, None) if t is None else (t[0, s, :n], t[1, s, :n], t[:, s, n].clone() if (eos and n < t.shape[2]) else None)
        if text_row:
            return (self.tids[s, :n, 0].to(torch.long), None) + tl
        ids = self.ids[s, :n].to(torch.long)
        ids = ids[:, 0] if first_column else ids
        hid = self.hid[s, :n] if self.hid is not None else None
        if first_column and t is not None:             # a refine-text state: the text sampler's log-probs, one value per step
            return (ids, hid) + tl
        if self.lps is None:
            return ids, hid, None, None, None
        return ids, hid, self.lps[0, s, :n], self.lps[1, s, :n], self.lps[:, s, n].clone() if (eos and n < self.lps.shape[2]) else None


class ReportRing:
    """Two chunks of decode steps in flight: per slot one pinned int32 buffer for each of `sizes`, an event, and the row layout current at enqueue (see RowBook)."""

    def __init__(self, *sizes: int):
        self._bufs = [[torch.zeros(n, dtype=torch.int32).pin_memory() for n in sizes] for _ in range(2)]
        self._evs = [torch.cuda.Event() for _ in range(2)]
        self.pending: List[tuple] = []             # (slot, layout) of the chunks in flight, oldest first
        self.free = self._bufs[0]                  # the buffers of the next push: the caller enqueues its report(s) into them behind the chunk just launched

    def push(self, layout) -> None:
        """the report(s) are enqueued: the layout is remembered and the event recorded on the current stream"""
        slot = 0 if self.free is self._bufs[0] else 1
        self._evs[slot].record()
        self.pending.append((slot, layout))
        self.free = self._bufs[1 - slot]

    def pop(self):
        """waits for the oldest chunk in flight: (its layout, its buffers)"""
        slot, layout = self.pending.pop(0)
        self._evs[slot].synchronize()
        return layout, self._bufs[slot]


class NoiseFeed:
    """The sampler's noise of one generate() call (its docstring names the kinds): `buf` [n_draws, rows, V] on the device, None for "device"; a caller's array
    sets n_draws.  "torch" noise is drawn chunk by chunk ahead of the steps that read it (draw_to) and leaves torch's generator as the reference would (restore)."""

    def __init__(self, gpt: "GPT", noise, n_draws: int, rows: int, V: int, stage_cap: int):
        self.n_draws, self.buf, self._stage, self._states, self._drawn = int(n_draws), None, None, [], 0
        if isinstance(noise, str) and noise == "torch":
            self.buf = torch.empty(self.n_draws, rows, V, dtype=torch.float32, device=gpt.device)
            # pinned [cap, rows, V] staging slots, kept on the engine across calls (pinning is expensive)
            if getattr(gpt, "_stage_key", None) != (rows, V, stage_cap):
                gpt._stage_key, gpt._stage_next = (rows, V, stage_cap), 0
                gpt._stage_bufs = [[torch.empty(stage_cap, rows, V, dtype=torch.float32).pin_memory(), None] for _ in range(3)]
            self._gpt, self._cap, self._stage = gpt, stage_cap, gpt._stage_bufs
        elif not (isinstance(noise, str) and noise == "device"):
            self.buf = torch.as_tensor(noise, dtype=torch.float32).to(gpt.device).contiguous()
            self.n_draws = int(self.buf.shape[0])

    def draw_to(self, n: int) -> None:
        """torch noise: the draws of steps < n are on their way to the device"""
        if self._stage is None or min(n, self.n_draws) <= self._drawn:
            return
        n, g = min(n, self.n_draws), self._gpt
        while self._drawn < n:
            # persistent pinned staging ring (3 slots): exponential_ straight into pinned memory, stream-ordered async
            # upload that lands after the chunk in flight and before the steps that read it; a slot is reused once the
            # copy that last read it has completed
            k = min(n - self._drawn, self._cap)
            slot = g._stage_next % 3
            g._stage_next += 1
            buf, ev = self._stage[slot]
            if ev is not None:
                ev.synchronize()
            for i in range(k):
                self._states.append(torch.random.get_rng_state())
                buf[i].exponential_(1)
            self.buf[self._drawn:self._drawn + k].copy_(buf[:k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(g.device))
            self._stage[slot][1] = ev
            self._drawn += k

    def restore(self, used: int) -> None:
        """Leave torch's CPU generator where the reference would have left it: after `used` multinomial draws."""
        if self._states and used < len(self._states):
            torch.random.set_rng_state(self._states[used])


def resolve_generate(n_prompts: int, max_batch: int, num_vq: int, vocab_code: int, vocab_text: int, fp16_invariant: bool, *, temperature, eos_token, max_new_token=2048,
                     min_new_token=0, logits_warpers=(), logits_processors=(), infer_text=False, noise="auto", seed=None, utt_ids=None, row_limits=None,
                     sampling_per_row=None, prompt_of=None) -> SimpleNamespace:
    """Everything generate() decides before it touches the device, from its arguments and a few engine facts (`n_prompts` = the rows of inputs_ids;
    `fp16_invariant` = an fp16 engine under an invariant option).  Pure but for the seed: one draw from torch's CPU generator, only for device noise without one."""
    B, share = int(n_prompts), None
    if prompt_of is not None:             # B sequences on n_prompts prompts
        prompt_groups(prompt_of, n_prompts, infer_text=infer_text)            # (refusals; emb / mask keep the caller's prompt order)
        share = (np.ascontiguousarray([int(p) for p in prompt_of], dtype=np.int32), int(n_prompts))
        B = int(share[0].size)
        if B > max_batch:
            raise _lib.HipBackendError(f"prompt_of: {B} sequences exceed max_batch={max_batch}")
    V, rows_per_seq = (vocab_text, 1) if infer_text else (vocab_code, num_vq)      # multinomial rows per sequence: [B, V_text] vs [B*4, 626] (gpt.py:444-467)
    sc = sampler_cfg_from_objects(temperature, int(eos_token), int(max_new_token), min_new_token, logits_warpers, logits_processors, num_vq, infer_text=infer_text)
    knobs = row_sampling_array(sc, sampling_per_row, B, num_vq, infer_text) if sampling_per_row is not None else None
    if isinstance(noise, str) and noise == "auto":
        # host draws cost ~21 ns per element and step: 10k elements (4 sequences x 4 x 626) hide behind the GPU step, one
        # 21178-wide refine-text row already does not (measured: 502 vs 423 us/step at batch 1, 1.2 vs 0.5 ms at batch 4)
        # (an fp16 engine under "schedule_invariant" takes device noise only: ctts_gpt_begin refuses a caller's draws there)
        noise = "torch" if (B <= 4 and B * rows_per_seq * V <= 16384 and not fp16_invariant) else "device"
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (isinstance(noise, str) and noise == "device") else 0
    uid_arr = None if utt_ids is None else np.ascontiguousarray([int(u) for u in utt_ids], dtype=np.uint64)
    assert uid_arr is None or uid_arr.size == B, "utt_ids: one id per sequence"
    lim_arr = None if row_limits is None else np.ascontiguousarray([int(u) for u in row_limits], dtype=np.int32)
    assert lim_arr is None or lim_arr.size == B, "max_new_tokens_per_row: one limit per sequence"
    return SimpleNamespace(B=B, share=share, sc=sc, knobs=knobs, noise=noise, seed=int(seed), utt_ids=uid_arr, row_limits=lim_arr, rows_per_seq=rows_per_seq, V=V)


class DecodeSession:
    """The one driver of continuous batching: a generate state kept open while utterances are seated, decoded, delivered and replaced.  GPT.open_session hands it
    out -- utterances are submitted and cancelled while others decode, the decode batch is as wide as the utterances in flight need (it grows, ctts_gpt_grow +
    ctts_gpt_admit, when texts arrive and shrinks, ctts_gpt_compact, when they end), and it holds the engine's busy token until close(); a context manager.
    GPT.generate_many drives one too, with the request policy of SessionBook (`own_slots`, `admit_min`: results are then views of the output slots, which are never
    rewritten), a call-wide refine-text configuration (`sc.infer_text`: results are ids[:, 0]) and shared prompt passes (`share` = (prompt per ticket, prompts,
    adapter slot per ticket)); none of the three is offered by open_session.  Device noise.  Opened with `text_sc` (the refine pass's sampler configuration) a
    code-mode session also serves refine-text utterances as text rows beside the code rows (submit(mode="text"); ctts_gpt_enable_text_rows)."""

    def __init__(self, gpt: "GPT", sc, seed: int, rows: int, out_slots: int, return_hidden: bool, return_logprobs: bool, ensure_non_empty: bool, max_restarts: int = 64,
                 text_sc=None, own_slots: bool = False, admit_min: int = 1, share=None, hold=None, guide: Optional[TextGuide] = None,
                 return_text_logprobs: bool = False):
        self.gpt, self.sc, self.seed = gpt, sc, int(seed)
        self.guide = guide                         # guided refine-text: the call's TextGuide (text rows of a code session, or every row of an infer_text one)
        self.max_new = int(sc.max_new_token)
        self.text_sc = text_sc
        try:
            self.book = SessionBook(rows, out_slots, gpt.max_batch, gpt.max_seq, self.max_new, ensure_non_empty, max_restarts, gpt.compact,
                                    max_new_text=None if text_sc is None else int(text_sc.max_new_token), own_slots=own_slots, admit_min=admit_min)
        except ValueError as e:
            raise _lib.HipBackendError(f"open_session: {e}") from None
        # (the text rows' ids share the slots of `ids`: a slot is held by one utterance of either kind)
        if return_text_logprobs and text_sc is None and not sc.infer_text:
            raise _lib.HipBackendError("return_text_logprobs: a code call without text rows (infer_text=True, or a session opened with text_rows=...)")
        self.out = OutBuffers(out_slots, self.max_new, gpt, return_hidden, return_logprobs, None if text_sc is None else int(text_sc.max_new_token),
                              text_logprobs=bool(return_text_logprobs), infer_text=bool(sc.infer_text))
        self.ids, self.hid = self.out.ids, self.out.hid
        self.chunk = max(4, min(gpt.chunk_steps, gpt.compact_chunk))
        self.batch_trace: List[tuple] = []         # (steps launched, rows) at every change of the row count
        self.admissions: List[tuple] = []          # (steps launched, utterances seated) per admission
        self.compactions: List[tuple] = []         # (steps launched, rows kept) per compaction
        self.shared_prompts: List[tuple] = []      # (rows, prompts) per begin / admit of a state with shared prompt passes
        self.launched = 0
        self._req = {}                             # ticket -> (prompt [T, H] on the device, attended length n <= T, knobs or None, adapter slot or None, mode 0 / 1, guide source or None)
        self._ring = ReportRing(2 * int(rows))      # the row reports of the two chunks in flight
        self._share, self._hold = share, hold
        self._adapters = False                     # an utterance of this session named an adapter slot: every admission names its rows' slots from then on
        self._stream_mode = {}                     # streaming ticket -> "exact" / "eager"
        self._wins: List[SessionWindow] = []       # windows the last step made due
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_open(self):
        if not self._open:
            raise _lib.HipBackendError("DecodeSession: the session is closed")

    # -- requests ---------------------------------------------------------------------------------
    def submit(self, emb: torch.Tensor, mask: torch.Tensor, utt_id: int, limit: Optional[int] = None, sampling=None, adapter_slot: Optional[int] = None,
               mode: str = "code", stream: Optional[str] = None, stream_batch: Optional[int] = None, stream_hidden: bool = True, stream_lookback: int = 0,
               guide_src=None) -> int:
        """`guide_src` (mode="text", sessions opened with text_rows=dict(..., guide=TextGuide)): the utterance's source token ids -- its result is provably these
        ids in order with only the guide's free ids inserted, ended by EOS; None = it samples freely.
        `stream_lookback` (stream="exact"): each window is vocoded from max(0, s0 - stream_lookback) (SessionWindow.v0), for a consumer that filters across
        window boundaries (the output resampler).  `stream` "exact" / "eager" (SessionBook): sample windows of this utterance become due while it decodes, see take_windows(); `stream_batch` tokens between
        windows (default: the session's); `stream_hidden` = the windows are vocoded from hidden rows (needs return_hidden), False = from the ids.
        Queues one utterance: emb [T, H] (GPT.__call__), mask [T] left padded.  `limit` <= max_new_token, `sampling` a dict as in sampling_per_row,
        `adapter_slot` a resident adapter (load_adapter).  `mode` "text" (sessions opened with text_rows=): a refine-text utterance -- its prompt is the refine
        prompt, it samples under the text head with the session's text parameters (no per-utterance `sampling`), and its result's ids are [n].  Returns its ticket."""
        self._check_open()
        g = self.gpt
        if mode not in ("code", "text"):
            raise _lib.HipBackendError(f"submit: mode={mode!r} (\"code\" or \"text\")")
        if mode == "text" and self.text_sc is None:
            raise _lib.HipBackendError("submit: mode=\"text\" needs a session opened with text_rows=... (GPT.open_session)")
        if mode == "text" and sampling is not None:
            raise _lib.HipBackendError("submit: per-utterance sampling parameters are for code utterances; a text utterance keeps the session's text_rows values")
        if stream is not None and mode == "text":
            raise _lib.HipBackendError("submit: stream= is for code utterances; a text row produces no audio")
        if guide_src is not None:
            if mode != "text":
                raise _lib.HipBackendError("submit: guide_src is for text utterances (mode=\"text\"); a guide on a code row is not offered")
            if self.guide is None:
                raise _lib.HipBackendError("submit: guide_src needs a session opened with text_rows=dict(..., guide=TextGuide(...)) (guides without the per-call part)")
            tmax = int(self.text_sc.max_new_token)
            guide_src = check_guide_src(guide_src, tmax if limit is None else min(max(int(limit), 1), tmax), int(self.text_sc.eos_token), g.num_text_tokens, "submit: guide_src")
        if stream is not None and stream_hidden and self.hid is None:
            raise _lib.HipBackendError("submit: stream= vocodes hidden rows: open the session with return_hidden=True (or pass stream_hidden=False to stream from the ids)")
        emb = torch.as_tensor(emb)
        mask = torch.as_tensor(mask).flatten()
        if emb.dim() != 2 or emb.shape[1] != g.model_dim or mask.numel() != emb.shape[0]:
            raise ValueError(f"submit: emb must be [T, {g.model_dim}] and mask [T] (got {tuple(emb.shape)}, {tuple(mask.shape)})")
        _check_left_padded(mask.reshape(1, -1))
        n = int((mask != 0).sum())
        if n < 1:
            raise ValueError("submit: the prompt has no attended token")
        knobs = row_sampling_from_values(self.sc, sampling, g.num_vq) if sampling is not None else None
        slot = -1 if adapter_slot is None or int(adapter_slot) < 0 else int(adapter_slot)
        if slot >= 0 and g.invariant_option():
            raise _lib.HipBackendError(f"submit: per-utterance adapters are outside the {g.invariant_option()} contract; merge the adapter (with_lora) or set the option to 0")
        tk = self._enqueue(emb[emb.shape[0] - n:].to(g.device, dtype=torch.float32).contiguous(), n, utt_id, limit, knobs, slot if slot >= 0 else None, mode,
                           stream, stream_batch, stream_lookback, guide_src=guide_src)
        if stream is not None:
            self._stream_mode[tk] = stream
        return tk

    def _enqueue(self, prompt: torch.Tensor, n: int, utt_id: int, limit, knobs, adapter: Optional[int], mode: str = "code", stream=None, stream_batch=None,
                 stream_lookback: int = 0, guide_src=None) -> int:
        """One ticket: `prompt` [T, H] on the device, of which the last `n` rows are attended (rows before them are the caller's left padding); `adapter` None =
        the utterance names none (an int, -1 included, makes every later seating name its rows' slots)"""
        try:
            tk = self.book.submit(max(int(n), 1), utt_id, limit, mode, stream=stream, stream_batch=stream_batch, stream_lookback=stream_lookback)
        except ValueError as e:
            raise _lib.HipBackendError(str(e)) from None
        self._req[tk] = (prompt, int(n), knobs, adapter, 1 if mode == "text" else 0, guide_src)
        if adapter is not None and not self._adapters:
            self._adapters = True
            if self._hold is not None:
                self._hold.resets.add("adapters")
        return tk

    def cancel(self, ticket: int) -> bool:
        """A queued utterance is dropped at once, a seated one is cancelled on the device at the next step boundary; either is delivered by a later step() with
        cancelled=True and the tokens written so far.  False: unknown ticket, already delivered or already cancelled."""
        self._check_open()
        return self.book.cancel(int(ticket)) is not None

    # -- engine calls -------------------------------------------------------------------------------
    def _prompts(self, tks):
        """The prompts [k, Ta, H] / masks [k, Ta] of one seating, Ta = the longest attended length among them: a ticket whose tensor has Ta rows or more gives its
        last Ta (a request's tickets are rows of the caller's batch and keep the caller's padding rows), a shorter one is zero-padded on the left.  With shared
        prompt passes: one row per prompt the tickets name, and `share` = (prompt per ticket, prompts) for the begin / admit call to stage, or None."""
        g, req = self.gpt, self._req
        rows, share = tks, None
        if self._share is not None:
            prompt_of, n_prompts, slots = self._share
            sel, local, leaders = prompt_groups(prompt_of, n_prompts, slots, subset=tks)
            if len(sel) < len(tks):
                share = (np.ascontiguousarray(local, dtype=np.int32), len(sel))
            self.shared_prompts.append((len(tks), len(sel)))
            rows = [tks[j] for j in leaders]
        Ta = max(1, max(req[tk][1] for tk in rows))
        emb = torch.nn.utils.rnn.pad_sequence([req[tk][0][-Ta:] for tk in rows], batch_first=True, padding_side="left")
        n = torch.as_tensor([req[tk][1] for tk in rows], device=g.device)
        mask = (torch.arange(Ta, device=g.device)[None, :] >= (Ta - n)[:, None]).to(torch.int32)
        return Ta, emb, mask, share

    def _seat(self, seats, st, begin: bool = False):
        """Carries out one seating [(row, ticket)]: the state's first (GPT._begin_state, then the first sample) or ctts_gpt_admit, with the per-row attributes --
        adapter slots, sampling knobs, row modes, shared prompts -- that the call picks up"""
        g, lib, h, utts, req = self.gpt, self.gpt._lib, self.gpt._h, self.book.utts, self._req
        tks = [tk for _, tk in seats]
        k = len(tks)

        def arr(values, dtype=np.int32):
            return np.ascontiguousarray(values, dtype=dtype)

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p)

        rows, uids, lims = arr([r for r, _ in seats]), arr([utts[tk]["utt_id"] for tk in tks], np.uint64), arr([utts[tk]["limit"] for tk in tks])
        outs, atts = arr([utts[tk]["slot"] for tk in tks]), arr([utts[tk]["attempt"] for tk in tks])
        Ta, emb, mask, share = self._prompts(tks)
        slots = arr([-1 if req[tk][3] is None else req[tk][3] for tk in tks]) if self._adapters else None
        knobs = None
        if any(req[tk][2] is not None for tk in tks):
            base = row_sampling_from_values(self.sc, None, g.num_vq)
            knobs = (_lib.RowSampling * k)(*[req[tk][2] or base for tk in tks])
        modes = arr([req[tk][4] for tk in tks])
        guide = getattr(self, "guide", None)        # guided refine-text: every seated slot is named, so a re-used slot never keeps its predecessor's record
        gsrcs = [req[tk][5] for tk in tks] if guide is not None else None
        if not begin:
            if guide is not None:
                g._set_guides(st, outs.tolist(), gsrcs)
            if slots is not None:
                _lib.check(lib.ctts_gpt_admit_adapters(h, k, ptr(rows), ptr(slots), st), "admit_adapters")
            if knobs is not None:         # (re-admissions of ensure_non_empty included: the utterance keeps its own knobs)
                _lib.check(lib.ctts_gpt_admit_sampling(h, k, ptr(rows), knobs, st), "admit_sampling")
            if self.text_sc is not None:
                _lib.check(lib.ctts_gpt_admit_modes(h, k, ptr(rows), ptr(modes), st), "admit_modes")
            try:                          # (the shared prompt passes are staged next to the admit they are for, and cleared whether or not it took them)
                if share is not None:
                    _lib.check(lib.ctts_gpt_share_prompts(h, k, ptr(share[0]), share[1]), "share_prompts")
                _lib.check(lib.ctts_gpt_admit(h, k, ptr(rows), Ta, mask.data_ptr(), emb.data_ptr(), ptr(uids), ptr(lims), ptr(outs), ptr(atts), st), "admit")
            finally:
                lib.ctts_gpt_share_prompts(h, 0, None, 0)
            self.admissions.append((self.launched, k))
            return
        g._begin_state(st, k, Ta, mask, emb, self.sc, self.out.io(self.max_new, self.seed, uids, lims), self.out, knobs=knobs, modes=modes if modes.any() else None,
                       adapters=None if slots is None else slots.tolist(), share=share, text_sc=self.text_sc,
                       guide=None if guide is None else (guide, outs.tolist(), gsrcs))
        _lib.check(lib.ctts_gpt_sample(h, st), "sample")
        self.launched = 1
        self.batch_trace.append((self.launched, k))

    def _result(self, tk: int, n: int, fin: int = 0, cancelled: bool = False, final: bool = True) -> SessionResult:
        """The utterance's first n tokens out of its output slot: clones (views where slots are the tickets' own).  `final`: the utterance ended -- its ticket and
        slot are released; else a view of a live utterance's tokens so far.  A text row: ids [n] as generate(infer_text=True) returns them (gpt.py:298-299), no
        hiddens, no log-probs."""
        u = self.book.utts[tk]
        s, eos, text = u["slot"], bool(fin & 2), u.get("mode", "code") == "text"
        ids, hid, lp, slp, flp = self.out.take(0 if s is None else s, n if s is not None else 0, eos and s is not None, bool(self.sc.infer_text), text)
        if final and not self.book.own_slots:
            hid, lp, slp = (x.clone() if x is not None else None for x in (hid, lp, slp))
        res = SessionResult(ticket=tk, utt_id=u["utt_id"], ids=ids, hiddens=hid, logprobs=lp, sampled_logprobs=slp, final_logprobs=flp, finished_by_eos=eos,
                            cancelled=cancelled, attempt=u["attempt"], mode="text" if text else "code")
        if final:
            self.book.release(tk)
            self._req.pop(tk, None)
        return res

    # -- the loop ---------------------------------------------------------------------------------------
    def _build_windows(self, due, results) -> List[SessionWindow]:
        from .vocoder import window_token_range
        book, by_tk, out = self.book, {r.ticket: r for r in results}, []
        dev = self.gpt.device
        for tk, slot, n, s0, s1, final in due:
            mode = self._stream_mode.get(tk, "exact")
            # a lookback widens the request to [v0, s1): the window stays (s0, s1), clamped as without one
            v0 = book.window_v0(tk, s0, final)
            if final:
                # the finished (or cancelled) utterance IS the prefix: settled to its end; built from the delivered clones, the slot is already released
                self._stream_mode.pop(tk, None)
                r = by_tk[tk]
                a, b, _, v0, s1 = window_token_range(n, v0, s1, book.hop, book.halo_frames)
                s0 = max(v0, min(s0, s1))
                out.append(SessionWindow(tk, n, s0, s1, True, a, r.ids[a:b].to(torch.int32), r.hiddens[a:b] if r.hiddens is not None else None, bool(r.cancelled), mode,
                                         v0))
                continue
            a, b, _, v0, s1 = window_token_range(n, v0, s1, book.hop, book.halo_frames, clamp_tail=(mode != "exact"))
            s0 = max(v0, min(s0, s1))
            out.append(SessionWindow(tk, n, s0, s1, False, a, self.ids[slot, a:b], self.hid[slot, a:b] if self.hid is not None else None, False, mode, v0))
        return out

    def take_windows(self) -> List[SessionWindow]:
        """The SessionWindows the last step() made due, in report order (a ticket's final window comes with its SessionResult)."""
        out, self._wins = self._wins, []
        return out

    @torch.no_grad()
    def step(self) -> List[SessionResult]:
        """One chunk of decode steps is launched and the previous chunk's row report is read (_advance), then the batch is rebalanced (_rebalance).  Returns the
        utterances that ended; the sample windows the step made due for streaming utterances wait in take_windows() (replaced by the next step)."""
        out = self._advance()
        self._rebalance()
        self._wins = self._build_windows(self.book.take_windows(), out)
        return out

    def _advance(self) -> List[SessionResult]:
        """Phase 1 of a step: pending cancels reach the device, one chunk of decode steps is launched with its row report behind it, and the report of the chunk
        before is read (two chunks stay enqueued): finished utterances are delivered, first-token-EOS ones queued again with their next attempt.  With nothing
        live nothing is launched.  `live` = [(ticket, tokens so far)] of the rows that report showed decoding (empty: no report was read)."""
        self._check_open()
        g, lib, h, book = self.gpt, self.gpt._lib, self.gpt._h, self.book
        out = [self._result(tk, 0, 1, True) for tk in book.take_dropped()]
        self.live = []
        if not book.begun or book.idle():
            return out
        with torch.cuda.device(g.device):
            st = g._stream()
            rows = book.cancel_rows()
            if rows:
                arr = np.ascontiguousarray(rows, dtype=np.int32)
                _lib.check(lib.ctts_gpt_cancel(h, len(rows), arr.ctypes.data_as(C.c_void_p), st), "cancel")
            if book.n_live() > 0:
                _lib.check(lib.ctts_gpt_decode(h, self.chunk, 1 if g.use_graph else 0, st), "decode")
                self.launched += self.chunk
                _lib.check(lib.ctts_gpt_rows_enqueue(h, self._ring.free[0].data_ptr(), st), "rows_enqueue")
                self._ring.push(book.book.layout())
                if len(self._ring.pending) == 2:
                    lay, (words,) = self._ring.pop()
                    states = words[:2 * len(lay)].view(-1, 2).tolist()
                    out += [self._result(*r) for r in book.report(lay, states)]
                    self.live = book.live
        return out

    def _rebalance(self) -> None:
        """Phase 2 of a step, SessionBook.plan carried out: the state's first seating, or queued utterances into free rows and into rows the batch grows by, else
        a compaction.  (A request's consumer works between the phases: its vocoder launches stay in front of the admission's prompt pass on the stream.)"""
        g, lib, h, book = self.gpt, self.gpt._lib, self.gpt._h, self.book
        plan = book.plan()
        if not plan:
            return
        with torch.cuda.device(g.device):
            st = g._stream()
            if plan.begin:
                self._seat(plan.begin, st, begin=True)
            if plan.grow:
                _lib.check(lib.ctts_gpt_grow(h, plan.grow, st), "grow")
            if plan.admit:
                self._seat(plan.admit, st)
            if plan.compact is not None:
                karr = np.ascontiguousarray(plan.compact, dtype=np.int32)
                _lib.check(lib.ctts_gpt_compact(h, karr.ctypes.data_as(C.c_void_p), int(karr.size), st), "compact")
                self.compactions.append((self.launched, len(plan.compact)))
            if plan.grow or plan.compact is not None:
                self.batch_trace.append((self.launched, len(book.book.row_tk)))

    def drain(self) -> List[SessionResult]:
        """steps until nothing is queued or live; everything delivered on the way"""
        out = []
        while not self.book.idle():
            out += self.step()
        return out

    def close(self) -> None:
        """Ends the session (utterances still queued or decoding are abandoned) and releases the engine."""
        if not self._open:
            return
        self._open = False
        g = self.gpt
        try:
            if self.book.begun and getattr(g, "_h", None) and g._h.value:
                with torch.cuda.device(g.device):
                    g._end_state(g._stream())
                    g.saturations = g._report_saturations(g._h, g._stream(), "session")
        finally:
            self._hold.release()


class _BusyToken:
    """One generate() at a time per KV cache: shared by every engine bound to the same KV tensor (LoRA-merged siblings, with_lora)."""
    def __init__(self):
        self.owner = None


class EngineHold:
    """The busy token of a loaded engine, taken for one call or one session (GPT._hold) -- engine state (batch, step counters, noise staging ring) and the KV cache,
    shared with LoRA-merged sibling engines, belong to ONE of them at a time.  A context manager; release() hands the token back together with the one sticky
    engine setting a call or session may have made, named in `resets`: "adapters" (set_row_adapters: a later plain call names its own).  Requests that are
    staged for one begin / admit -- sampling knobs, row modes, shared prompts -- are cleared by whoever staged them (GPT._begin_state, DecodeSession._seat)."""

    def __init__(self, gpt: "GPT", busy: str, resets=()):
        if not gpt._finalized:
            raise _lib.HipBackendError("weights not loaded")
        if gpt._busy_token.owner is not None:
            raise _lib.HipBackendError(busy)
        self.gpt, self.resets = gpt, {r for r in resets if r}
        gpt._busy_token.owner = gpt

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def release(self) -> None:
        g = self.gpt
        try:
            if "adapters" in self.resets and getattr(g, "_h", None) and g._h.value:
                g.set_row_adapters(None)
        finally:
            g._busy_token.owner = None


class GPT:
    """See module docstring.  Extra kwargs (ride in the YAML `kwargs`):
    max_batch (<=128), max_seq_len, weight_dtype "fp32" (default, parity) | "fp16" (fast), chunk_steps."""

    Context = Context
    GenerationOutputs = GenerationOutputs

    def __init__(self, gpt_config: dict, num_audio_tokens: int = 626, num_text_tokens: int = 21178, num_vq=4,
                 use_flash_attn=False, **kwargs):
        self.num_vq = num_vq
        self.num_audio_tokens = num_audio_tokens
        self.num_text_tokens = num_text_tokens
        self.gpt_config = dict(gpt_config)
        self.model_dim = int(gpt_config["hidden_size"])
        self.emb_code = [_EmbShim(num_audio_tokens) for _ in range(num_vq)]
        self.max_batch = int(kwargs.get("max_batch", 4))
        self.max_seq = int(kwargs.get("max_seq_len", 4096))
        wd = kwargs.get("weight_dtype", "fp32")        # parity mode by default; "fp16" = fast mode (Modes)
        self.dtype_code = {"fp16": _lib.DTYPE_F16, "float16": _lib.DTYPE_F16, "fp32": _lib.DTYPE_F32, "float32": _lib.DTYPE_F32}[str(wd)]
        self.chunk_steps = int(kwargs.get("chunk_steps", 32))
        self.use_graph = bool(kwargs.get("use_graph", True))
        self.device = torch.device(kwargs.get("device", "cuda"))
        self.gpt = None              # attribute the pipeline swaps for LoRA (pipeline:420-432); unused here
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipBackendError("infer_type='hip' needs a visible MI355X (torch.cuda.is_available() is False); no CPU fallback")
        self._h = C.c_void_p()
        cfg = _lib.GptCfg(hidden=self.model_dim, inter=int(gpt_config["intermediate_size"]),
                          heads=int(gpt_config["num_attention_heads"]), layers=int(gpt_config["num_hidden_layers"]),
                          vocab_code=num_audio_tokens, num_vq=num_vq, max_batch=self.max_batch, max_seq=self.max_seq,
                          dtype=self.dtype_code)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_gpt_create(C.byref(cfg), C.byref(self._h)), "ctts_gpt_create")
        self._finalized = False
        self._kv = None
        self._busy_token = _BusyToken()
        self._lora = []
        # engine options (ctts_gpt_set_option; include/ctts_hip.h lists them): {"prefill_split_rows": 0, ...}; applied before the weights are packed
        self.options = dict(kwargs.get("options") or {})
        for k, v in self.options.items():
            self.set_option(k, v)
        self.compact = bool(kwargs.get("compact", True))      # finished-row compaction at chunk boundaries (batches of >= 8 sequences)
        self.compact_chunk = int(kwargs.get("compact_chunk", 8))   # ... whose chunks are this short: a finished row leaves the batch 1-2 chunks later
        self.shared_prompts = []          # (rows, prompts) per begin / admit of the last generate(prompt_of=...) / generate_many(prompt_of=...) call
        self.model_path = kwargs.get("model_path", None)
        if self.model_path:
            self.from_pretrained(self.model_path)

    def set_option(self, name: str, value: int) -> None:
        """One named engine option (ctts_gpt_set_option): an explicit call, never the environment.  Unknown names are an error."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_gpt_set_option(self._h, str(name).encode(), int(value)), f"set_option({name})")
        self.options[str(name)] = int(value)

    def invariant_option(self) -> Optional[str]:
        """The name under which this engine keeps the batch-invariance contract -- "batch_invariant" (fp32 engines) or its dtype-independent name
        "schedule_invariant" (either dtype; the only setter on fp16 engines) -- or None while neither is on."""
        for name in ("batch_invariant", "schedule_invariant"):
            if self.options.get(name, 0):
                return name
        return None

    def get_option(self, name: str) -> int:
        """The effective value of an engine option (ctts_gpt_get_option)."""
        v = C.c_int(0)
        _lib.check(self._lib.ctts_gpt_get_option(self._h, str(name).encode(), C.byref(v)), f"get_option({name})")
        return int(v.value)

    # -- nn.Module-like surface ------------------------------------------------------------------
    def eval(self):
        return self

    def to(self, device=None, dtype=None):
        return self

    @property
    def busy(self) -> bool:
        """A generate() generator is live on this engine or on one that shares its KV cache."""
        return getattr(self, "_busy_token", None) is not None and self._busy_token.owner is not None

    def close(self, _force: bool = False):
        """Destroys the engine handle (packed weights, workspaces, graphs) now instead of at garbage collection; the KV
        tensor is released with the last engine that shares it.  Refused while a generate() generator of THIS engine is live (its
        native handle is in use): exhaust or close the generator first."""
        owner = getattr(getattr(self, "_busy_token", None), "owner", None)
        if not _force and owner is not None and (owner is self or getattr(owner, "gpt", None) is self):
            raise _lib.HipBackendError("GPT.close(): a generate() generator or a session (open_session) is still live on this engine; exhaust or close it first")
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ctts_gpt_destroy(self._h)
            self._h = C.c_void_p()
        self._finalized = False
        self._kv = None

    def __del__(self):
        try:
            self.close(_force=True)
        except Exception:
            pass

    def from_pretrained(self, file_path: str):
        self.load_state_dict(torch.load(file_path, weights_only=True, mmap=True))      # gpt.py:84-85

    def add_lora(self, layer: int, target: str, A, B, scale: float):
        """peft merge rule W += scale * B @ A (pipeline:420-432) applied before finalize.  `target`: q_proj k_proj v_proj o_proj (768 x 768), gate_proj up_proj
        (3072 x 768) or down_proj (768 x 3072); A is [r, in], B [out, r] for the target's own (out, in), checked here (the engine reads both by these sizes)."""
        self._check_lora(layer, target, A, B)
        self._lora.append((layer, target, np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32), float(scale)))

    def _check_lora(self, layer, target, A, B, r_max=None) -> None:
        """Layer, target and A / B shapes of one adapter matrix pair against this engine's widths; errors name layer and target."""
        H, I, L = int(self.gpt_config["hidden_size"]), int(self.gpt_config["intermediate_size"]), int(self.gpt_config["num_hidden_layers"])
        try:
            check_lora_shapes(layer, target, A, B, H, I)
        except ValueError as e:
            raise _lib.HipBackendError(str(e)) from None
        if not 0 <= int(layer) < L:
            raise _lib.HipBackendError(f"LoRA: layer {layer} ({target}) out of range: the engine has {L} layers")
        r = np.shape(A)[0]
        if r_max is not None and r > r_max:
            raise _lib.HipBackendError(f"LoRA: layer {layer} {target}: r = {r} > {r_max} (per-utterance adapters; a merged adapter, with_lora(), takes any rank)")

    @staticmethod
    def _known_key(k: str, layers: int, num_vq: int) -> bool:
        """The 196 keys of the reference's GPT state dict; the engine's ctts_gpt_set_weight is strict about them."""
        import re
        m = re.fullmatch(r"gpt\.layers\.(\d+)\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj|input_layernorm|post_attention_layernorm)\.weight", k)
        if m:
            return int(m.group(1)) < layers
        if k in ("gpt.norm.weight", "emb_text.weight", "head_text.parametrizations.weight.original0", "head_text.parametrizations.weight.original1"):
            return True
        m = re.fullmatch(r"emb_code\.(\d+)\.weight", k) or re.fullmatch(r"head_code\.(\d+)\.parametrizations\.weight\.original[01]", k)
        return bool(m) and int(m.group(1)) < num_vq

    def load_state_dict(self, sd, strict: bool = True, _share_kv: Optional[torch.Tensor] = None, _busy_token=None):
        """strict=True (default, like the reference's load_state_dict, gpt.py:84-85): an unexpected key is an error.  strict=False: keys the
        engine does not know (e.g. `...rotary_emb.inv_freq` buffers of older transformers exports) are skipped and returned in
        `self.unexpected_keys`; missing keys are an error either way (the engine cannot run without them)."""
        if self._finalized:
            raise _lib.HipBackendError("weights already loaded")
        keep = []
        self.unexpected_keys = [k for k in sd if not self._known_key(k, int(self.gpt_config["num_hidden_layers"]), self.num_vq)]
        if self.unexpected_keys and strict:
            raise _lib.HipBackendError(f"load_state_dict(strict=True): unexpected key(s) {self.unexpected_keys[:4]}{' ...' if len(self.unexpected_keys) > 4 else ''}")
        if _busy_token is not None:
            self._busy_token = _busy_token
        for k, v in sd.items():
            if k in self.unexpected_keys:
                continue
            a = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float32)
            a = np.ascontiguousarray(a)
            keep.append(a)
            _lib.check(self._lib.ctts_gpt_set_weight(self._h, k.encode(), a.ctypes.data_as(C.c_void_p), a.size), f"set_weight({k})")
        for (layer, target, A, B, scale) in self._lora:
            _lib.check(self._lib.ctts_gpt_merge_lora(self._h, layer, target.encode(), A.ctypes.data_as(C.c_void_p),
                                                     B.ctypes.data_as(C.c_void_p), A.shape[0], scale), "merge_lora")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_gpt_finalize(self._h), "ctts_gpt_finalize")
            rope = rope_table(self.max_seq)
            _lib.check(self._lib.ctts_gpt_set_rope(self._h, rope.ctypes.data_as(C.c_void_p), self.max_seq), "set_rope")
            nbytes = self._lib.ctts_gpt_kv_bytes(self._h)
            # torch owns the KV cache; LoRA-merged siblings borrow the base engine's (one generate() runs at a time)
            self._kv = _share_kv if (_share_kv is not None and _share_kv.numel() >= nbytes) else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(self._lib.ctts_gpt_bind_kv(self._h, self._kv.data_ptr(), nbytes), "bind_kv")
        self._finalized = True
        self._ctor = dict(gpt_config=self.gpt_config, num_audio_tokens=self.num_audio_tokens, num_text_tokens=self.num_text_tokens,
                          num_vq=self.num_vq, max_batch=self.max_batch, max_seq_len=self.max_seq,
                          weight_dtype="fp16" if self.dtype_code == _lib.DTYPE_F16 else "fp32", chunk_steps=self.chunk_steps,
                          use_graph=self.use_graph, device=str(self.device), options=dict(self.options))
        self._sd_host = {k: v for k, v in sd.items() if k not in self.unexpected_keys}        # kept for LoRA-merged siblings (pipeline:420-432)
        return self

    def with_lora(self, adapters) -> "GPT":
        """A sibling engine whose weights carry W += scale * B @ A on every projection the adapter names -- q/k/v/o and gate / up / down, like peft's
        merge_and_unload (pipeline:420-432); the base engine stays untouched, like the reference's gpt_org swap (pipeline:424,465-470).  A merged adapter is
        just weights: every engine mode (fp16, the persistent launch, batch_invariant) serves it."""
        g = GPT(**self._ctor)
        for (layer, target, A, B, scale) in adapters:
            g.add_lora(layer, target, A, B, scale)
        g.load_state_dict(self._sd_host, _share_kv=self._kv, _busy_token=self._busy_token)     # one KV cache -> one busy token
        return g

    # -- per-utterance LoRA: adapters resident beside the packed weights, one slot (or none) per sequence -------------
    def load_adapter(self, slot: int, adapters) -> None:
        """`adapters` = [(layer, target, A[r,in], B[out,r], scale)] as returned by pipeline.load_lora_adapter; replaces whatever the slot held.  Targets: q/k/v/o_proj
        and gate / up / down_proj, r <= 16, shapes checked against the target's (out, in).  The tables of the three MLP targets (737 KB per layer and slot) are
        allocated when the first of them is loaded."""
        if not self._finalized:
            raise _lib.HipBackendError("weights not loaded")
        for (layer, target, A, B, scale) in adapters:
            self._check_lora(layer, target, A, B, r_max=16)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_gpt_clear_adapter(self._h, int(slot)), "clear_adapter")
            for (layer, target, A, B, scale) in adapters:
                A = np.ascontiguousarray(A, dtype=np.float32); B = np.ascontiguousarray(B, dtype=np.float32)
                _lib.check(self._lib.ctts_gpt_set_adapter(self._h, int(slot), int(layer), target.encode(), A.ctypes.data_as(C.c_void_p),
                                                          B.ctypes.data_as(C.c_void_p), int(A.shape[0]), float(scale)), "set_adapter")

    def set_row_adapters(self, slots) -> None:
        """Adapter slot (or -1 / None) per sequence for the following generate() calls; None switches the per-row path off.  With it
        every projection the row's adapter names evaluates W x + scale * B (A x) per row (q/k/v/o -- decode: inside the projection launches, lora_worker.h; prompt pass: two
        more launches per layer.  gate / up / down: two more launches per layer, decode and prompt pass, while a live row's slot holds such a target; decode steps then take the
        launch chain at every row count).
        Not under options={"batch_invariant": 1} / {"schedule_invariant": 1}: per-utterance adapters are outside the contract (a merged adapter, with_lora(), is covered)."""
        with torch.cuda.device(self.device):
            if slots is None:
                _lib.check(self._lib.ctts_gpt_set_row_adapters(self._h, None, 0), "set_row_adapters")
                return
            inv = self.invariant_option()
            if inv and any(s is not None and int(s) >= 0 for s in slots):
                raise _lib.HipBackendError(f"set_row_adapters: per-utterance adapters are outside the {inv} contract; construct the GPT with "
                                           f"options={{'{inv}': 0}}, or merge the adapter into a sibling engine (with_lora)")
            arr = np.ascontiguousarray([(-1 if s is None else int(s)) for s in slots], dtype=np.int32)
            _lib.check(self._lib.ctts_gpt_set_row_adapters(self._h, arr.ctypes.data_as(C.c_void_p), int(arr.size)), "set_row_adapters")

    # -- get_emb (gpt.py:125-149) ----------------------------------------------------------------
    def __call__(self, input_ids: torch.Tensor, text_mask: torch.Tensor, spk_emb=None, spk_emb_ids: Optional[int] = None) -> torch.Tensor:
        """emb[B,T,H] fp32 on the device, computed by embed_prompt_kernel (ctts_gpt_embed).  With `spk_emb` (a [H] vector, a
        [B,H] table or a base16384 string) the rows whose id == spk_emb_ids are overwritten by F.normalize(spk) in the same
        launch (Tokenizer.apply_spk_emb, tokenizer.py:150-178)."""
        if not self._finalized:
            raise _lib.HipBackendError("weights not loaded")
        ids = input_ids.to(self.device).to(torch.int32).contiguous()
        tm = text_mask.to(self.device).to(torch.int32).contiguous()
        B, T = int(ids.shape[0]), int(ids.shape[1])
        # nn.Embedding raises on an id outside its table (gpt.py:125-149: emb_text on the text rows' first column, emb_code[i] on the code rows);
        # the gather kernel does not check, so the same IndexError is raised here (one reduction + one flag read per prompt)
        tmb = tm.bool()
        bad = ((ids[..., 0] < 0) | (ids[..., 0] >= self.num_text_tokens)) & tmb
        bad = bad | (((ids < 0) | (ids >= self.num_audio_tokens)).any(-1) & ~tmb)
        if bool(bad.any()):
            raise IndexError("index out of range in self")
        emb = torch.empty(B, T, self.model_dim, dtype=torch.float32, device=self.device)
        spk_t, sid = None, -1
        if spk_emb is not None:
            from .. import codec
            v = codec.speaker_to_vector(spk_emb) if (isinstance(spk_emb, str) or torch.as_tensor(spk_emb).dim() == 1) else torch.as_tensor(spk_emb).float()
            v = v.reshape(-1, self.model_dim)
            v = F.normalize(v, p=2.0, dim=1, eps=1e-12)                    # == normalize(dim=0) of each [H] vector
            spk_t = v.expand(B, -1).contiguous().to(self.device)
            sid = int(spk_emb_ids)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ctts_gpt_embed(self._h, ids.data_ptr(), tm.data_ptr(), B, T, spk_t.data_ptr() if spk_t is not None else None,
                                                sid, emb.data_ptr(), self._stream()), "embed")
        return emb

    forward = __call__

    # -- generate (gpt.py:313-569, infer_text=False) ----------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _hold(self, busy: str, *resets) -> EngineHold:
        """Takes the engine for one call (`with`) or one session; `busy` is the refusal while another holds it, `resets` see EngineHold"""
        return EngineHold(self, busy, resets)

    @torch.no_grad()
    def _report_saturations(self, h, st, what: str) -> int:
        """fp16 stores of unbounded values saturate instead of overflowing to inf (fp16 engines: SwiGLU outputs, packed residual; fp32 engines:
        the SwiGLU head / tail images of a prompt pass over more than 64 rows, prefill_split.hip, and of decode batches of >= 9 rows).  A non-zero count means the checkpoint drives
        activations past the fp16 range: the result is finite but clipped -- say so."""
        nsat = C.c_int32(0)
        _lib.check(self._lib.ctts_gpt_saturations(h, C.byref(nsat), st), "saturations")
        n = int(nsat.value)
        if n:
            import warnings
            if self.dtype_code == _lib.DTYPE_F16:
                msg = f"use weight_dtype='fp32' for this checkpoint"
            elif self.invariant_option():
                # the option's contract is one arithmetic per row: switching kernels between calls would break it, so they stay
                msg = ("the fp32 engine keeps silu(gate) * up / 16 and the scaled residual rows as fp16 head / tail images; THIS call's values were clipped there.  "
                       "batch_invariant is on, so the engine keeps these kernels (results stay schedule-independent, and clipped); construct the GPT with "
                       "options={'batch_invariant': 0, 'prefill_split_rows': 0, 'split_decode_rows': 0} to run this checkpoint on the exact fp32 kernels")
            else:
                msg = ("the fp32 engine's prompt passes of more than 64 rows and its decode batches of >= 9 rows keep silu(gate) * up / 16 and the scaled residual rows as fp16 "
                       "head / tail images; THIS call's values were clipped there.  The engine now keeps the exact fp32 kernels (split_decode_rows=0, prefill_split_rows=0) for "
                       "the following calls; construct the GPT with options={'prefill_split_rows': 0, 'split_decode_rows': 0} to keep them from the first call on for this checkpoint")
                for opt in ("split_decode_rows", "prefill_split_rows"):
                    try:
                        if self.get_option(opt) > 0:
                            self.set_option(opt, 0)
                    except Exception:      # noqa: BLE001 (the warning below still tells the caller)
                        pass
            warnings.warn(f"hip GPT (weight_dtype {'fp16' if self.dtype_code == _lib.DTYPE_F16 else 'fp32'}): {n} fp16 stores saturated or were NaN "
                          f"during this {what}; {msg}", RuntimeWarning)
        return n

    def generate(self, emb: torch.Tensor, inputs_ids: torch.Tensor, temperature: torch.Tensor,
                 eos_token: Union[int, torch.Tensor], attention_mask: Optional[torch.Tensor] = None, max_new_token=2048,
                 min_new_token=0, logits_warpers=[], logits_processors=[], infer_text=False, return_attn=False,
                 return_hidden=False, stream=False, show_tqdm=True, ensure_non_empty=True, stream_batch=24,
                 context=None, noise="auto", seed: Optional[int] = None, max_restarts: int = 64, utt_ids=None, max_new_tokens_per_row=None,
                 sampling_per_row=None, return_logprobs=False, prompt_of=None, text_guide=None, guide_src=None, return_text_logprobs=False):
        """`return_text_logprobs` (infer_text=True; a separate opt-in -- `return_logprobs` keeps refusing infer_text): `logprobs` / `sampled_logprobs` are [n] per
        sequence, `final_logprobs` [2] where the row ended by EOS, written by the text sampler (ctts_gpt_set_text_logprob_out); ids are bit-identical without it.
        `text_guide` (a TextGuide; infer_text=True) with `guide_src` = one list of source token ids or None per sequence: a guided sequence's ids are provably
        its source ids in order, with only the guide's free ids inserted, ended by EOS (include/ctts_hip.h "Guided refine-text"); None = the sequence samples freely.
        `prompt_of` (shared prompt passes, ctts_gpt_share_prompts; code mode): a list of length B naming each sequence's prompt; `emb` / `inputs_ids` /
        `attention_mask` then have one row per PROMPT, every per-row argument (`utt_ids`, `max_new_tokens_per_row`, `sampling_per_row`) and every output has length
        B.  The first sequence of a prompt runs the prompt pass, the others receive a copy of its KV lane; `shared_prompts` records (rows, prompts) of the call.
        `return_logprobs`: every yielded GenerationOutputs (the partial ones of stream=True too) carries `logprobs`, `sampled_logprobs` and
        `final_logprobs` for the tokens so far, written by the sampler as it draws them (ctts_gpt_set_logprob_out; code mode only).
        `noise`: "torch" draws q = empty(B*4,V).exponential_() per step from torch's CPU generator -- the very numbers
        torch.multinomial consumes in the reference, so TorchSeedContext(seed) reproduces the CPU path's tokens (costs
        ~21 ns of host time per element: hidden behind the GPU up to batch ~8, 3x the step time at batch 32); "device"
        uses the on-device Philox generator keyed by `seed` (None: one draw from torch's CPU generator, so manual_seed
        still makes the call reproducible); "auto" (default) = "torch" for the batches the reference itself can run
        (<= 4 sequences, pipeline:391-397) as long as a step draws at most 16k numbers (code mode), "device" otherwise
        (larger batches, the 21178-wide refine-text pass); or an array [n_draws, B*4, V].
        `utt_ids` (device noise): one global utterance id per sequence (default 0..B-1) -- the device noise stream of a sequence is keyed by
        (seed, its utterance id, codebook, its own step and regenerate attempt), not by its batch row, so an utterance samples the same
        noise in whatever slice / batch position / rank it is served.  `max_new_tokens_per_row`: per-sequence token limits (<= max_new_token).
        `sampling_per_row`: one dict (keys SAMPLING_KEYS; a missing key keeps the call's value) or None per sequence -- the utterance's own temperature,
        top_P, top_K, repetition_penalty, min_new_token (ctts_gpt_set_row_sampling; code mode only).  eos, max_new_token and the F8 threshold stay per call."""
        if return_attn:
            raise _lib.HipBackendError("return_attn=True is unsupported (the reference's eager attention path is broken, SURVEY F2)")
        if return_logprobs and infer_text:
            raise _lib.HipBackendError("return_logprobs: the refine-text pass (infer_text=True) returns no log-probs; code mode only")
        if return_text_logprobs and not infer_text:
            raise _lib.HipBackendError("return_text_logprobs: a code call without text rows (infer_text=True, or a session opened with text_rows=...)")
        with self._hold("GPT.generate is already running on this engine (or on an engine sharing its KV cache): exhaust or close the previous generator first"):
            call = resolve_generate(int(inputs_ids.shape[0]), self.max_batch, self.num_vq, self.num_audio_tokens, self.num_text_tokens,
                                    self.dtype_code == _lib.DTYPE_F16 and bool(self.invariant_option()), temperature=temperature, eos_token=eos_token,
                                    max_new_token=max_new_token, min_new_token=min_new_token, logits_warpers=logits_warpers, logits_processors=logits_processors,
                                    infer_text=infer_text, noise=noise, seed=seed, utt_ids=utt_ids, row_limits=max_new_tokens_per_row,
                                    sampling_per_row=sampling_per_row, prompt_of=prompt_of)
            limits = [int(call.sc.max_new_token)] * call.B if call.row_limits is None else [min(max(int(v), 1), int(call.sc.max_new_token)) for v in call.row_limits]
            srcs = resolve_guides(text_guide, guide_src, call.B, bool(infer_text), int(call.sc.eos_token), self.num_text_tokens, limits, "generate")
            yield from self._generate(call, emb, inputs_ids, attention_mask, context or Context(), stream, stream_batch, ensure_non_empty, max_restarts,
                                      return_hidden, bool(return_logprobs), guide=None if srcs is None else (text_guide, list(range(call.B)), srcs),
                                      return_text_logprobs=bool(return_text_logprobs))

    def _set_text_guide(self, st, tg: TextGuide) -> None:
        f = np.ascontiguousarray(list(tg.free_ids) or [0], dtype=np.int32)
        _lib.check(self._lib.ctts_gpt_set_text_guide(self._h, f.ctypes.data_as(C.c_void_p), len(tg.free_ids), tg.max_run, st), "set_text_guide")

    def _set_guides(self, st, slots, srcs) -> None:
        """Names the sources of the utterances at output `slots` (srcs[i] None = unguided: a fresh, empty record).  A slot beyond the guide table carries no record
        and needs none while it is unguided; a guided one there is refused by the engine."""
        named = [(int(s), src) for s, src in zip(slots, srcs) if src is not None or int(s) < GUIDE_SLOTS]
        if not named:
            return
        sl, cat, off = guide_arrays([s for s, _ in named], [src for _, src in named])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.ctts_gpt_set_guides(self._h, len(named), p(sl), p(cat), p(off), st), "set_guides")

    def _begin_state(self, st, k: int, T: int, mask, emb, sc, io, out: OutBuffers, knobs=None, modes=None, adapters=None, share=None, text_sc=None, guide=None) -> None:
        """Creates a generate state for k rows (generate() and a session's first seating): stages `adapters` (slot per row; sticky: the caller's EngineHold resets
        it), `knobs` (ctts_row_sampling [k]), `modes` (int32 [k]) and `share` (prompt per row int32 [k], prompts), then ctts_gpt_begin, the text rows, the guide
        (`guide` = (TextGuide, output slots, sources or None per slot)), the log-prob outputs of `out` and the prompt pass.  Nothing staged for a begin outlives
        it, whether or not begin took it: a later plain call finds nothing pending."""
        lib, h = self._lib, self._h
        try:
            if adapters is not None:
                self.set_row_adapters(adapters)
            if knobs is not None:
                _lib.check(lib.ctts_gpt_set_row_sampling(h, knobs, k), "set_row_sampling")
            if modes is not None:
                _lib.check(lib.ctts_gpt_set_row_modes(h, modes.ctypes.data_as(C.c_void_p), k), "set_row_modes")
            if share is not None:
                _lib.check(lib.ctts_gpt_share_prompts(h, k, share[0].ctypes.data_as(C.c_void_p), share[1]), "share_prompts")
            _lib.check(lib.ctts_gpt_begin(h, k, T, mask.data_ptr(), C.byref(sc), C.byref(io), st), "begin")
        finally:
            lib.ctts_gpt_set_row_sampling(h, None, 0)
            lib.ctts_gpt_set_row_modes(h, None, 0)
            lib.ctts_gpt_share_prompts(h, 0, None, 0)
        if text_sc is not None:                    # (after begin, which creates the state; before the first sample, which a begun text row needs it for)
            _lib.check(lib.ctts_gpt_enable_text_rows(h, C.byref(text_sc), out.tids.data_ptr(), st), "enable_text_rows")
        if guide is not None:                      # (after the text rows; before the first sample: begin's guided rows start from their records)
            self._set_text_guide(st, guide[0])
            self._set_guides(st, guide[1], guide[2])
        if out.lps is not None:
            _lib.check(lib.ctts_gpt_set_logprob_out(h, out.lps[0].data_ptr(), out.lps[1].data_ptr(), st), "set_logprob_out")
        tlps = getattr(out, "tlps", None)          # the text rows' log-probs: a separate opt-in (after begin / the text rows, which reset it; before the first sample)
        if tlps is not None:
            _lib.check(lib.ctts_gpt_set_text_logprob_out(h, tlps[0].data_ptr(), tlps[1].data_ptr(), st), "set_text_logprob_out")
        _lib.check(lib.ctts_gpt_prefill(h, emb.data_ptr(), st), "prefill")

    def _end_state(self, st) -> int:
        """The end of a generate state: waits for everything launched and returns the steps taken.  ctts_gpt_progress raises the device give-up word (a persistent
        launch's bounded wait ran out, or a projection tile never got its low-rank term: later launches were no-ops, the sampler drew from stale rows: no audio)"""
        torch.cuda.current_stream(self.device).synchronize()
        steps, alld = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.ctts_gpt_progress(self._h, C.byref(steps), C.byref(alld), st), "progress")
        return steps.value

    def _generate(self, call, emb, inputs_ids, attention_mask, context, stream, stream_batch, ensure_non_empty, max_restarts, return_hidden, return_logprobs, guide=None,
                  return_text_logprobs=False):
        """generate() on a held engine: setup, step 0 with its restarts, the streamed or the pipelined loop, the end of the state"""
        lib, h, dev, B, T = self._lib, self._h, self.device, call.B, int(inputs_ids.shape[1])
        infer_text, max_new = bool(call.sc.infer_text), int(call.sc.max_new_token)
        self.compactions, self.shared_prompts = [], [] if call.share is None else [(B, call.share[1])]
        mask = torch.ones(int(inputs_ids.shape[0]), T, dtype=torch.int32, device=dev) if attention_mask is None else attention_mask.to(dev).to(torch.int32).contiguous()
        emb = emb.to(dev, dtype=torch.float32).contiguous()
        out = OutBuffers(B, max_new, self, return_hidden, return_logprobs, text_logprobs=return_text_logprobs, infer_text=infer_text)
        feed = NoiseFeed(self, call.noise, max_new + max_restarts, B * call.rows_per_seq, call.V, max(int(self.chunk_steps), int(stream_batch) if stream else 1, 1))
        io = out.io(feed.n_draws, call.seed, call.utt_ids, call.row_limits, feed.buf)
        tm = self.host_timing = {}
        t_last = [time.perf_counter()]

        def tick(name):
            now = time.perf_counter()
            tm[name] = tm.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

        with torch.cuda.device(dev):
            st = self._stream()
            tick("setup")
            self._begin_state(st, B, T, mask, emb, call.sc, io, out, knobs=call.knobs, share=call.share, guide=guide)
            tick("begin+prefill")
            # step 0 with the batch-wide ensure_non_empty regenerate (gpt.py:496-525): while a sequence's first token is EOS, every sequence samples again
            used, steps, alld = 0, C.c_int32(0), C.c_int32(0)
            while True:
                feed.draw_to(used + 1)
                _lib.check(lib.ctts_gpt_sample(h, st), "sample")
                used += 1
                _lib.check(lib.ctts_gpt_progress(h, C.byref(steps), C.byref(alld), st), "progress")
                if not bool(out.finish.any().item()):
                    break
                if not (ensure_non_empty and used < max_restarts):
                    feed.restore(used)
                    return                                   # gpt.py:525 bare return
                _lib.check(lib.ctts_gpt_restart(h, st), "restart")
            tick("step0")
            if stream:
                # streaming: synchronous polling; like the reference (gpt.py:531-543) a partial result is yielded whenever the number
                # of generated tokens is a multiple of stream_batch -- also when that step was the last one, so the final yield
                # below can repeat it, exactly as the reference does
                chunk = int(stream_batch)
                while not alld.value and steps.value < max_new and not context.get():
                    n = min(chunk - steps.value % chunk, max_new - steps.value)
                    feed.draw_to(used + n)
                    _lib.check(lib.ctts_gpt_decode(h, n, 1 if self.use_graph else 0, st), "decode")
                    prev = steps.value
                    _lib.check(lib.ctts_gpt_progress(h, C.byref(steps), C.byref(alld), st), "progress")
                    used += steps.value - prev
                    if steps.value == prev and not alld.value:
                        raise _lib.HipBackendError("decode made no progress (device state inconsistent)")
                    if steps.value % chunk == 0 and steps.value > prev:
                        yield self._outputs(out, infer_text)
            else:
                self._pipelined_loop(st, call, feed, context, tick, used - steps.value, steps.value)
                used += self._end_state(st) - steps.value
                tick("final_progress")
            feed.restore(used)             # (before the saturation report, which may warn: torch's generator is left right whatever follows)
            self.saturations = self._report_saturations(h, st, "generate()")
            res = self._outputs(out, infer_text)
            tick("outputs")
            yield res

    def _pipelined_loop(self, st, call, feed: NoiseFeed, context, tick, restarts: int, launched: int) -> None:
        """One chunk stays in flight while the previous chunk's progress words are inspected (no GPU bubble at the poll); steps launched after every sequence
        finished exit at their first instruction on the device.  `restarts` = draws spent on ensure_non_empty regenerations, `launched` = steps so far."""
        lib, h, B, max_new, graph, chunk = self._lib, self._h, call.B, int(call.sc.max_new_token), 1 if self.use_graph else 0, self.chunk_steps
        # finished-row compaction (no counterpart in the reference, where finished rows keep computing until the slowest one ends,
        # gpt.py:527-546): the per-row finish flags travel with the progress words; rows known to have finished are dropped from
        # the decode batch at the next chunk boundary (ctts_gpt_compact), down to the next size of compact_size()
        compacting = self.compact and (not call.sc.infer_text) and B >= 8
        if compacting:
            chunk = max(4, min(chunk, self.compact_chunk))
        ring = ReportRing(4, 2 * B) if compacting else ReportRing(4)
        row_seq, done_seq = list(range(B)), set()      # current decode row -> sequence; the sequences known to have finished
        while True:
            while len(ring.pending) < 2 and launched < max_new and not context.get():
                n = min(chunk, max_new - launched)
                tick("loop_other")
                feed.draw_to(restarts + launched + n)
                tick("draw")
                _lib.check(lib.ctts_gpt_decode(h, n, graph, st), "decode")
                tick("decode_launch")
                launched += n
                _lib.check(lib.ctts_gpt_progress_enqueue(h, ring.free[0].data_ptr(), st), "progress_enqueue")
                if compacting:
                    _lib.check(lib.ctts_gpt_rows_enqueue(h, ring.free[1].data_ptr(), st), "rows_enqueue")
                ring.push(list(row_seq) if compacting else None)
            if not ring.pending:
                break
            tick("loop_other")
            layout, bufs = ring.pop()
            tick("event_wait")
            if int(bufs[0][2]) or int(bufs[0][0]) >= max_new or context.get():
                break
            if compacting:
                flags = bufs[1][:2 * len(layout)].view(-1, 2)[:, 0].tolist()
                done_seq.update(sq for sq, f in zip(layout, flags) if f)
                keep = compact_keep([sq not in done_seq for sq in row_seq])
                if keep is not None:
                    karr = np.ascontiguousarray(keep, dtype=np.int32)
                    _lib.check(lib.ctts_gpt_compact(h, karr.ctypes.data_as(C.c_void_p), int(karr.size), st), "compact")
                    row_seq = [row_seq[r] for r in keep]
                    self.compactions.append((launched, len(row_seq)))

    # -- continuous batching: more utterances than decode rows (no counterpart in the reference) ------------------------------------
    @torch.no_grad()
    def generate_many(self, emb: torch.Tensor, inputs_ids: torch.Tensor, temperature: torch.Tensor, eos_token: Union[int, torch.Tensor],
                      attention_mask: Optional[torch.Tensor] = None, max_new_token=2048, min_new_token=0, logits_warpers=[],
                      logits_processors=[], return_hidden=False, ensure_non_empty=True, context=None, seed: Optional[int] = None,
                      max_restarts: int = 64, utt_ids=None, max_new_tokens_per_row=None, rows: Optional[int] = None, admit_min: Optional[int] = None,
                      on_done=None, infer_text: bool = False, adapter_slots=None, sampling_per_row=None, return_logprobs=False, prompt_of=None,
                      text_guide=None, guide_src=None, return_text_logprobs=False) -> GenerationOutputs:
        """N utterances (left-padded prompts emb[N,T,H], like generate()) through `rows` <= max_batch decode rows: whenever utterances
        finish, queued ones take over their rows (ctts_gpt_admit) instead of the whole slice waiting for its slowest row as the reference's
        slices of 4 do (pipeline:391-397, gpt.py:527-546); once the queue is empty finished rows are compacted away (ctts_gpt_compact).
        Device noise only: an utterance's noise stream is keyed by (seed, its utterance id, its own step, its regenerate attempt), its step
        counter / token limit / outputs are its own, so it produces what generate() produces for it in any slice.  ensure_non_empty
        (gpt.py:496-525) acts per utterance: one whose first token is EOS is admitted again with its next attempt, up to `max_restarts`.
        `on_done(list_of_indices)` is called (on the host, while decoding continues) as utterances complete.
        `adapter_slots` = the resident adapter slot (load_adapter) of every utterance or -1 / None: per-utterance LoRA under row re-use (an admitted
        utterance brings its own adapter, ctts_gpt_admit_adapters).  `sampling_per_row` = one dict of sampling knobs or None per utterance (as in
        generate()): an admitted utterance brings its own knobs (ctts_gpt_admit_sampling).  `return_logprobs`: as in generate() -- the log-prob arrays are
        indexed by utterance like the ids, so admission, compaction and ensure_non_empty re-admission need nothing extra.
        `prompt_of` (as in generate(): N = len(prompt_of) utterances on emb.shape[0] prompts): the utterances each begin / admit call seats are grouped by prompt,
        whatever their number, and each group pays one prompt pass (a group split across two admissions pays two); `shared_prompts` lists (rows, prompts) per call.
        With `adapter_slots`, the utterances of one prompt must carry one slot or none over the WHOLE request (refused up front) -- stricter than the engine, which
        compares only the sequences one call seats: give utterances that differ in their adapter their own prompt rows.
        Returns one GenerationOutputs for all N utterances, in input order."""
        gen = self.generate_many_iter(emb, inputs_ids, temperature, eos_token, attention_mask=attention_mask, max_new_token=max_new_token,
                                      min_new_token=min_new_token, logits_warpers=logits_warpers, logits_processors=logits_processors,
                                      return_hidden=return_hidden, ensure_non_empty=ensure_non_empty, context=context, seed=seed, max_restarts=max_restarts,
                                      utt_ids=utt_ids, max_new_tokens_per_row=max_new_tokens_per_row, rows=rows, admit_min=admit_min, infer_text=infer_text,
                                      adapter_slots=adapter_slots, sampling_per_row=sampling_per_row, return_logprobs=return_logprobs, prompt_of=prompt_of,
                                      text_guide=text_guide, guide_src=guide_src, return_text_logprobs=return_text_logprobs)
        try:
            while True:
                ev = next(gen)
                if on_done is not None:
                    on_done([e[0] for e in ev])
        except StopIteration as stop:
            return stop.value

    @torch.no_grad()
    def generate_many_iter(self, emb, inputs_ids, temperature, eos_token, attention_mask=None, max_new_token=2048, min_new_token=0, logits_warpers=[],
                           logits_processors=[], return_hidden=False, ensure_non_empty=True, context=None, seed=None, max_restarts: int = 64,
                           utt_ids=None, max_new_tokens_per_row=None, rows=None, admit_min=None, infer_text: bool = False, progress: bool = False,
                           adapter_slots=None, sampling_per_row=None, return_logprobs=False, prompt_of=None, text_guide=None, guide_src=None,
                           return_text_logprobs=False):
        """`return_text_logprobs` (infer_text=True): as `return_logprobs`, with the text sampler's one-value-per-step log-probs ([n], [n], [2]).
        `text_guide` / `guide_src`: as in generate() (infer_text=True): an admitted utterance brings its own source (ctts_gpt_set_guides before its admit).
        generate_many as a generator: yields [(utterance index, ids [n,4] long, hiddens [n,768] or None)] for the utterances that completed
        since the last yield -- while the rest keeps decoding (what was yielded is final: its rows were written before the report that showed
        the utterance finished) -- and returns (StopIteration.value) the GenerationOutputs of all N utterances.
        `infer_text=True`: the refine-text pass (gpt.py infer_text: the 21178-way text head, one id per step) through the same row re-use; ids are [n].
        `progress=True` (streaming): between the completion lists the generator also yields ("progress", [(utterance index, tokens so far n, ids[:n],
        hiddens[:n] or None)]) for the utterances still decoding -- the first n tokens of an utterance are final once reported.
        `return_logprobs=True`: every tuple of either kind gains a last element, a GenerationOutputs of that one utterance's tokens so far (ids, hiddens,
        logprobs, sampled_logprobs, final_logprobs: lists of one), and the returned GenerationOutputs carries the three fields for all N."""
        if return_logprobs and infer_text:
            raise _lib.HipBackendError("return_logprobs: the refine-text pass (infer_text=True) returns no log-probs; code mode only")
        if return_text_logprobs and not infer_text:
            raise _lib.HipBackendError("return_text_logprobs: a code call without text rows (infer_text=True, or a session opened with text_rows=...)")
        with self._hold("GPT.generate is already running on this engine (or on an engine sharing its KV cache)", adapter_slots is not None and "adapters"):
            return (yield from self._generate_many(emb, inputs_ids, temperature, eos_token, attention_mask, int(max_new_token), min_new_token, logits_warpers,
                                                   logits_processors, return_hidden, ensure_non_empty, context or Context(), seed, max_restarts, utt_ids,
                                                   max_new_tokens_per_row, rows, admit_min, bool(infer_text), bool(progress), adapter_slots,
                                                   sampling_per_row, bool(return_logprobs), prompt_of, text_guide, guide_src, bool(return_text_logprobs)))

    def _generate_many(self, emb, inputs_ids, temperature, eos_token, attention_mask, max_new_token, min_new_token, logits_warpers, logits_processors,
                       return_hidden, ensure_non_empty, context, seed, max_restarts, utt_ids, row_limits, rows, admit_min, infer_text=False, progress=False,
                       adapter_slots=None, sampling_per_row=None, return_logprobs=False, prompt_of=None, text_guide=None, guide_src=None,
                       return_text_logprobs=False):
        """The request as a client of the DecodeSession driver: prepares the utterances, submits them in their order of service (position j of that order is
        ticket j and output slot j) and translates what the driver delivers into generate_many_iter's events"""
        dev = self.device
        N, T = int(inputs_ids.shape[0]), int(inputs_ids.shape[1])
        pof = None                                # shared prompt passes: utterance -> row of emb / mask
        if prompt_of is not None:
            prompt_groups(prompt_of, N, adapter_slots, infer_text=infer_text)      # (refusals)
            pof = [int(p) for p in prompt_of]
            n_prompts, N = N, len(pof)
        NVQ = self.num_vq
        R = min(N, int(rows) if rows else self.max_batch, self.max_batch)
        sc = sampler_cfg_from_objects(temperature, int(eos_token), max_new_token, min_new_token, logits_warpers, logits_processors, NVQ, infer_text=infer_text)
        knobs = list(row_sampling_array(sc, sampling_per_row, N, NVQ, infer_text)) if sampling_per_row is not None else [None] * N
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        lens = [T] * int(inputs_ids.shape[0]) if attention_mask is None else attention_mask.to(torch.int32).sum(1).cpu().tolist()
        emb = emb.to(dev, dtype=torch.float32).contiguous()
        if pof is not None:
            lens = [lens[p] for p in pof]
        if max(lens) + max_new_token > self.max_seq:
            # (every utterance is admitted with its own prompt, trimmed of padding: the longest one decides)
            raise _lib.HipBackendError(f"generate_many: prompt of {max(lens)} tokens + max_new_token={max_new_token} exceed max_seq_len={self.max_seq}")
        uids = [int(u) for u in utt_ids] if utt_ids is not None else list(range(N))
        lims = [min(max(int(v), 1), max_new_token) for v in row_limits] if row_limits is not None else [max_new_token] * N
        assert len(uids) == N and len(lims) == N
        srcs = resolve_guides(text_guide, guide_src, N, infer_text, int(eos_token), self.num_text_tokens, lims, "generate_many")
        slots = [None] * N
        if adapter_slots is not None:
            slots = [-1 if a is None or int(a) < 0 else int(a) for a in adapter_slots]
            if len(slots) != N or infer_text:
                raise _lib.HipBackendError(f"adapter_slots: {len(slots)} entries for {N} utterances (code mode only)")
        admit_min = max(1, int(admit_min) if admit_min else R // 8)
        # Order of service: longest expected utterance first (LPT list scheduling) -- the request ends when its LAST row does, and a long utterance admitted late
        # decodes alone on a 32-row engine (the 256-utterance request: 2905 steps launched for 2518 ideal ones in arrival order).  The expectation is the row's own
        # token limit where the caller gave one, else the prompt length (longer text, longer audio).  Results do not depend on the order: every output is indexed
        # by utterance and the device noise is keyed by the utterance id.  Default: arrival order ("fifo"): a streaming caller wants its first utterance first.
        if getattr(self, "schedule", "fifo") == "longest_first":      # (ChatTTSPlusPipeline's throughput mode orders the request itself; direct callers opt in)
            back = sorted(range(N), key=(lambda u: (-lims[u], u)) if row_limits is not None else (lambda u: (-lens[u], u)))
        else:
            back = list(range(N))                                  # ticket (= output slot) -> utterance index: every index handed back is mapped through it
        with torch.cuda.device(dev):
            ses = DecodeSession(self, sc, seed, R, N, return_hidden, return_logprobs, ensure_non_empty, max_restarts, own_slots=True, admit_min=admit_min, guide=None if srcs is None else text_guide, return_text_logprobs=return_text_logprobs,
                                share=None if pof is None else ([pof[u] for u in back], n_prompts, [slots[u] for u in back] if adapter_slots is not None else None))
            self.admissions, self.compactions, self.shared_prompts = ses.admissions, ses.compactions, ses.shared_prompts
            for u in back:
                ses._enqueue(emb[u if pof is None else pof[u]], lens[u], uids[u], lims[u], knobs[u], slots[u], guide_src=None if srcs is None else srcs[u])

            def event(r, n=None):
                """one utterance of a yielded list: (index[, tokens so far], ids, hiddens[, its GenerationOutputs so far])"""
                one = (GenerationOutputs(ids=[r.ids], attentions=[], hiddens=[r.hiddens] if r.hiddens is not None else [], logprobs=[r.logprobs],
                                         sampled_logprobs=[r.sampled_logprobs], final_logprobs=[r.final_logprobs]),) if (return_logprobs or return_text_logprobs) else ()
                return (back[r.ticket],) + (() if n is None else (n,)) + (r.ids, r.hiddens) + one

            n_done = 0
            ses._rebalance()                                       # the first R utterances begin
            while n_done < N and not context.get():
                done = ses._advance()
                live = [event(ses._result(tk, n, final=False), n) for tk, n in ses.live if n > 0] if progress else []
                if live:
                    yield ("progress", live)
                n_done += len(done)
                if done:
                    yield [event(r) for r in done]
                ses._rebalance()
            self._end_state(self._stream())
            self.saturations = self._report_saturations(self._h, self._stream(), "generate_many()")
            return self._outputs(ses.out, infer_text, order=np.argsort(np.asarray(back)).tolist())      # input order again

    # -- serving session (ctts_gpt_grow / ctts_gpt_cancel) ------------------------------------------------------------------------
    def open_session(self, temperature, eos_token, max_new_token, min_new_token=0, logits_warpers=[], logits_processors=[], return_hidden=False,
                     return_logprobs=False, seed: Optional[int] = None, rows: Optional[int] = None, out_slots: Optional[int] = None, ensure_non_empty=True,
                     text_rows=None, return_text_logprobs=False, **out_of_scope) -> DecodeSession:
        """`return_text_logprobs` (with `text_rows`): a text utterance's SessionResult carries logprobs / sampled_logprobs [n] and final_logprobs [2] under the text
        head (ctts_gpt_set_text_logprob_out); code rows and `return_logprobs` are unaffected.
        Opens a DecodeSession: a generate state that stays open while utterances are submitted (submit), cancelled (cancel) and delivered (step / drain).  The
        sampling arguments are the call's values, as in generate_many; an utterance may bring its own (submit(sampling=...)).  `rows` <= max_batch bounds the
        decode batch (default max_batch), `out_slots` the utterances whose results are held at once (default 2 * rows; slots are recycled once a result has been
        cloned out).  Holds the engine until close(): generate* and score raise meanwhile.  Not offered inside a session, each refused with a message:
        shared prompt passes / num_candidates, caller-supplied noise, session-wide streaming windows (stream= / stream_batch= here: streaming is asked per utterance at
        submit(stream=...), see take_windows), infer_sharded, and the call-level names of the refine-text
        pass (infer_text, refine_text_only, params_refine_text).  The refine-text pass itself is served INSIDE the session: `text_rows` = a dict (or an object with
        these attributes) of temperature, top_P, top_K, eos_token ([Ebreak]), max_new_token (<= the code rows'), min_new_token makes submit(mode="text") seat
        refine-text utterances as text rows beside the code rows of the one decode batch (ctts_gpt_enable_text_rows); their results carry ids [n]."""
        refuse_out_of_scope(out_of_scope, "use generate() / generate_many() / infer() for it")
        rows = self.max_batch if rows is None else int(rows)
        if not (1 <= rows <= self.max_batch):
            raise _lib.HipBackendError(f"open_session: rows={rows} outside 1..max_batch={self.max_batch}")
        out_slots = 2 * rows if out_slots is None else int(out_slots)
        if out_slots < 1:
            raise _lib.HipBackendError(f"open_session: out_slots={out_slots} (at least one)")
        sc = sampler_cfg_from_objects(temperature, int(eos_token), int(max_new_token), min_new_token, logits_warpers, logits_processors, self.num_vq)
        text_sc = text_rows_cfg(text_rows, self.num_vq) if text_rows is not None else None
        guide = None if text_rows is None else (text_rows.get("guide") if isinstance(text_rows, dict) else getattr(text_rows, "guide", None))
        if guide is not None:
            if not isinstance(guide, TextGuide):
                raise _lib.HipBackendError("open_session: text_rows: guide must be a TextGuide")
            guide.check(int(text_sc.eos_token), self.num_text_tokens, "open_session: text_rows: guide")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        hold = self._hold("GPT.open_session: GPT.generate is already running on this engine (or on an engine sharing its KV cache): exhaust or close "
                          "the previous generator / session first")
        try:
            with torch.cuda.device(self.device):
                ses = DecodeSession(self, sc, seed, rows, out_slots, bool(return_hidden), bool(return_logprobs), bool(ensure_non_empty), text_sc=text_sc, hold=hold, guide=guide,
                                    return_text_logprobs=bool(return_text_logprobs))
        except BaseException:
            hold.release()
            raise
        self._busy_token.owner = ses
        return ses

    # -- teacher-forced scoring (train_lora.py:430-469; ctts_gpt_score) ----------------------------------------------------------
    @torch.no_grad()
    def score(self, emb: torch.Tensor, attention_mask: torch.Tensor, targets: torch.Tensor, n_targets) -> ScoreOutputs:
        """Log-probabilities and argmax of audio-code targets under the raw code heads, in one prompt pass (inference only).  emb [B, T, H] (this engine's
        __call__: text rows and code rows, left padded), attention_mask [B, T] left padded, targets [B, max_targets, 4], n_targets [B]: target j of sequence b
        is predicted by row T - n_b + j (score_inputs builds all four from a prompt and codes).  Positions are cumsum(mask) - 1 as in generate(), so a
        sequence scores the same alone as inside a padded batch.  Per-utterance adapters (set_row_adapters) apply per sequence.  Ends nothing a caller
        holds: refused while a generate() generator is live on this engine or on one sharing its KV cache.  Returns ScoreOutputs on the CPU."""
        return self._score(emb, attention_mask, targets, n_targets, "score", self._lib.ctts_gpt_score, self.num_vq, self.num_audio_tokens)

    def _score(self, emb, attention_mask, targets, n_targets, name, fn, cols, vocab) -> ScoreOutputs:
        """The one path of score (cols = num_vq: targets [B, max_targets, cols], refused on the host outside [0, vocab)) and score_text (cols = vocab = None: targets
        [B, max_targets], passed through to the kernel's NaN / -1) around the C entry point `fn`; `name` prefixes the messages."""
        with self._hold(f"GPT.{name}: a generate() generator is live on this engine (or on an engine sharing its KV cache), whose KV lanes "
                        "scoring would overwrite: exhaust or close it first"):
            dev = self.device
            emb = emb.to(dev, dtype=torch.float32).contiguous()
            if emb.dim() != 3 or emb.shape[2] != self.model_dim:
                raise ValueError(f"{name}: emb must be [B, T, {self.model_dim}] (got {tuple(emb.shape)})")
            B, T = int(emb.shape[0]), int(emb.shape[1])
            mask = torch.as_tensor(attention_mask)
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"{name}: attention_mask must be [{B}, {T}] (got {tuple(mask.shape)})")
            _check_left_padded(mask)
            tg = torch.as_tensor(targets).cpu().to(torch.int64)
            nt = torch.as_tensor(n_targets).cpu().to(torch.int64).flatten()
            tail = (cols,) if cols else ()
            if tg.dim() != 2 + len(tail) or tg.shape[0] != B or tuple(tg.shape[2:]) != tail or nt.numel() != B:
                raise ValueError(f"{name}: targets must be [{', '.join(map(str, (B, 'max_targets') + tail))}] and n_targets [{B}] (got {tuple(tg.shape)}, {tuple(nt.shape)})")
            maxt = int(tg.shape[1])
            for b in range(B):
                n = int(nt[b])
                if n < 1 or n > T or n > maxt:
                    raise ValueError(f"{name}: n_targets[{b}] = {n} outside 1..min(T={T}, max_targets={maxt})")
                t = tg[b, :n]
                if vocab is not None and bool(((t < 0) | (t >= vocab)).any()):
                    raise ValueError(f"{name}: a target of sequence {b} is outside [0, {vocab})")
            if B > self.max_batch or T > self.max_seq:
                raise ValueError(f"{name}: B={B} T={T} exceed max_batch={self.max_batch} / max_seq_len={self.max_seq}")
            msk = mask.to(dev).to(torch.int32).contiguous()
            tgd = tg.to(torch.int32).to(dev).contiguous()
            nta = np.ascontiguousarray(nt.numpy(), dtype=np.int32)
            lp = torch.empty((B, maxt) + tail, dtype=torch.float32, device=dev)
            am = torch.empty((B, maxt) + tail, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(fn(self._h, B, T, msk.data_ptr(), emb.data_ptr(), tgd.data_ptr(), nta.ctypes.data_as(C.c_void_p), maxt, lp.data_ptr(), am.data_ptr(), self._stream()), name)
            lp, am = lp.cpu(), am.cpu().to(torch.long)
            n = nt.tolist()
            lps = [lp[b, :n[b]] for b in range(B)]
            ams = [am[b, :n[b]] for b in range(B)]
            nll, acc, loss, accuracy = score_reduce(lps, ams, [tg[b, :n[b]] for b in range(B)])
            return ScoreOutputs(logprob=lps, argmax=ams, nll=nll, seq_accuracy=acc, loss=loss, accuracy=accuracy)

    @torch.no_grad()
    def score_text(self, emb: torch.Tensor, attention_mask: torch.Tensor, targets: torch.Tensor, n_targets) -> ScoreOutputs:
        """score() under the refine-text head (ctts_gpt_score_text): targets [B, max_targets] text ids, target j of sequence b predicted by row T - n_b + j
        (score_text_inputs builds the four arguments from a refine prompt and refined ids).  logprob[b] / argmax[b] are [n_b]; logprob is the `logprobs` that
        generate(infer_text=True, return_text_logprobs=True) returned for the same tokens.  Refused on an engine without head_text / emb_text."""
        return self._score(emb, attention_mask, targets, n_targets, "score_text", self._lib.ctts_gpt_score_text, None, None)

    @staticmethod
    def _outputs(out: OutBuffers, infer_text: bool = False, order=None) -> GenerationOutputs:
        """All sequences of a generate state (gpt.py:295-305); `order[b]` = the output slot of sequence b (default b).  final_logprobs: where the finish flag is set"""
        n = out.end_idx.cpu().tolist()
        with_lp = out.lps is not None or (infer_text and out.tlps is not None)
        eos = out.finish.cpu().tolist() if with_lp else [0] * len(n)
        rows = [out.take(s, n[s], bool(eos[s]), infer_text) for s in (order if order is not None else range(len(n)))]
        ids, hid, lp, slp, flp = ([r[i] for r in rows] for i in range(5))
        if not with_lp:
            return GenerationOutputs(ids=ids, attentions=[], hiddens=hid if out.hid is not None else [])
        return GenerationOutputs(ids=ids, attentions=[], hiddens=hid if out.hid is not None else [], logprobs=lp, sampled_logprobs=slp, final_logprobs=flp)

    # -- test hooks ------------------------------------------------------------------------------
    def last_logits(self, B: int) -> torch.Tensor:
        out = torch.empty(B, self.num_vq, self.num_audio_tokens, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ctts_gpt_logits(self._h, out.data_ptr(), self._stream()), "logits")
        return out

    DECODE_PLAN_FIELDS = ("B", "splits", "persist", "S", "nbg", "chunks", "dts", "pf_kb", "valu", "wide_blocks", "splitd", "prepack", "xhm", "spd", "down_sk",
                          "fuse_heads", "lora", "form_parts", "form_xh", "form_logits", "form_split", "form_nbg", "form_valu")

    def decode_plan(self) -> dict:
        """The launch plan of a decode step of the current batch on the path of the last planned step (ctts_gpt_debug_read "decode_plan"): host arithmetic only,
        no device work.  `splits` / `persist` are the decode path, `S` .. `lora` the layer plan, `form_*` the residual stream's form for the heads."""
        buf = (C.c_int32 * len(self.DECODE_PLAN_FIELDS))()
        nb = C.c_size_t(0)
        _lib.check(self._lib.ctts_gpt_debug_read(self._h, b"decode_plan", buf, C.sizeof(buf), C.byref(nb), None), "debug_read(decode_plan)")
        if nb.value != C.sizeof(buf):
            raise _lib.HipBackendError(f"decode_plan: the library returned {nb.value} bytes, this wrapper knows {len(self.DECODE_PLAN_FIELDS)} fields")
        return dict(zip(self.DECODE_PLAN_FIELDS, (int(v) for v in buf)))

    # per pass height: the layer plan's prompt fields, the attention kind (PROMPT_ATTN_KINDS) and per projection a GEMM kind (PROMPT_GEMM_KINDS) and `sliced`
    _PROMPT_HEIGHT_FIELDS = ("nbg", "prepack", "pfg", "pfs", "anchor", "lora", "attn", "qkv", "qkv_sliced", "o", "o_sliced", "gu", "gu_sliced", "down", "down_sliced")
    PROMPT_PLAN_FIELDS = ("passes", "rows_full", "rows_last", "pre_T") + _PROMPT_HEIGHT_FIELDS + tuple("last_" + f for f in _PROMPT_HEIGHT_FIELDS)
    PROMPT_ATTN_KINDS = ("row", "mfma", "mfma_anchor", "split")
    PROMPT_GEMM_KINDS = ("tile_norm", "tile_packed", "pfg0", "pfg1", "pfg2", "split64", "ring4", "ring2", "pp3", "pp4")

    def prompt_plan(self) -> dict:
        """The launch plans of the prompt passes of the last prefill / score call (ctts_gpt_debug_read "prompt_plan"): host arithmetic only, no device work.
        `passes` passes, the full ones `rows_full` rows high, the last `rows_last`; the unprefixed fields describe a full pass, `last_*` the last pass (the same
        plan when the call is one pass).  `attn` indexes PROMPT_ATTN_KINDS, `qkv` / `o` / `gu` / `down` index PROMPT_GEMM_KINDS."""
        buf = (C.c_int32 * len(self.PROMPT_PLAN_FIELDS))()
        nb = C.c_size_t(0)
        _lib.check(self._lib.ctts_gpt_debug_read(self._h, b"prompt_plan", buf, C.sizeof(buf), C.byref(nb), None), "debug_read(prompt_plan)")
        if nb.value != C.sizeof(buf):
            raise _lib.HipBackendError(f"prompt_plan: the library returned {nb.value} bytes, this wrapper knows {len(self.PROMPT_PLAN_FIELDS)} fields")
        return dict(zip(self.PROMPT_PLAN_FIELDS, (int(v) for v in buf)))

    def step_bytes(self, B: int, mean_ctx: float) -> float:
        return float(self._lib.ctts_gpt_step_bytes(self._h, B, float(mean_ctx)))
