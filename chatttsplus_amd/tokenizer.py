"""Tokenizer wrapper (host side, CPU text work -- out of the kernel scope) with the call
surface of the reference's chattts_plus/models/tokenizer.py:19-137: wraps the pickled BertTokenizerFast,
left-pads a batch to [B,T,num_vq] ids + attention/text masks, and exposes the special-token ids the
pipeline needs.  The speaker / prompt codecs live in chatttsplus_amd/codec.py."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import codec


class Tokenizer:
    def __init__(self, model_path=None, tokenizer=None, **kwargs):
        if tokenizer is None:
            # the reference stores a pickled BertTokenizerFast object (tokenizer.py:27-30): needs weights_only=False
            tokenizer = torch.load(model_path, map_location="cpu", mmap=True, weights_only=False)
        self._tokenizer = tokenizer
        self.len = len(tokenizer)
        self.spk_emb_ids = tokenizer.convert_tokens_to_ids("[spk_emb]")
        self.break_0_ids = tokenizer.convert_tokens_to_ids("[break_0]")
        self.eos_token = tokenizer.convert_tokens_to_ids("[Ebreak]")
        self.decode = self._tokenizer.batch_decode

    @torch.inference_mode()
    def encode(self, text: List[str], num_vq: int, prompt_str: Union[None, str, Sequence[Optional[str]]] = None,
               device="cpu") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """tokenizer.py:49-137: ids replicated over num_vq, LEFT padding, optional audio-prompt codes appended
        (text_mask = 0 there).  `prompt_str` may also be a list with one entry per text (a str or None; no counterpart in the
        reference, whose prompt is one per call): row i is its text ids followed by ITS codes, rows are left-padded to the longest
        total.  A list of equal strings gives exactly what the one string gives."""
        if prompt_str is not None and not isinstance(prompt_str, str):
            prompt_str = list(prompt_str)
            if len(prompt_str) != len(text):
                raise ValueError(f"encode: {len(prompt_str)} prompt strings for {len(text)} texts")
            if any(p != prompt_str[0] for p in prompt_str):
                return self._encode_ragged(text, num_vq, prompt_str, device)
            prompt_str = prompt_str[0] if prompt_str else None
        prompt = codec.decode_prompt(prompt_str) if prompt_str is not None else None
        prompt_size = 0
        if prompt is not None:
            assert prompt.size(0) == num_vq, "prompt dim 0 must equal to num_vq"
            prompt_size = prompt.size(1)
        ids_l, att_l = [], []
        for t in text:
            x = self._tokenizer(t, return_tensors="pt", add_special_tokens=False, padding=True)   # == encode_plus (tokenizer.py:70-72)
            ids_l.append(x["input_ids"].squeeze(0))
            att_l.append(x["attention_mask"].squeeze(0))
        T = max(i.size(0) for i in ids_l) + prompt_size
        B = len(ids_l)
        input_ids = torch.zeros(B, T, dtype=ids_l[0].dtype)
        attention_mask = torch.zeros(B, T, dtype=att_l[0].dtype)
        for i in range(B):
            n = ids_l[i].size(0)
            input_ids[i, T - prompt_size - n: T - prompt_size] = ids_l[i]
            attention_mask[i, T - prompt_size - n: T - prompt_size] = att_l[i]
            if prompt_size:
                attention_mask[i, T - prompt_size:] = 1
        text_mask = attention_mask.bool()
        new_input_ids = input_ids.unsqueeze(-1).expand(-1, -1, num_vq).clone()
        if prompt_size:
            text_mask[:, T - prompt_size:] = False
            new_input_ids[:, T - prompt_size:] = prompt.t().unsqueeze(0).expand(B, -1, -1)
        return new_input_ids.to(device), attention_mask.to(device), text_mask.to(device)

    def _encode_ragged(self, text: List[str], num_vq: int, prompt_strs: List[Optional[str]], device):
        """encode() with one audio prompt (or None) per row: each row, stripped of its left padding, is the batch-1 encode of that row."""
        cache = {}
        ids_l, att_l, prm_l = [], [], []
        for t, ps in zip(text, prompt_strs):
            x = self._tokenizer(t, return_tensors="pt", add_special_tokens=False, padding=True)
            ids_l.append(x["input_ids"].squeeze(0))
            att_l.append(x["attention_mask"].squeeze(0))
            if ps is not None and ps not in cache:
                cache[ps] = codec.decode_prompt(ps)
                assert cache[ps].size(0) == num_vq, "prompt dim 0 must equal to num_vq"
            prm_l.append(None if ps is None else cache[ps])
        sizes = [0 if p is None else int(p.size(1)) for p in prm_l]
        T = max(i.size(0) + s for i, s in zip(ids_l, sizes))
        B = len(ids_l)
        input_ids = torch.zeros(B, T, num_vq, dtype=ids_l[0].dtype)
        attention_mask = torch.zeros(B, T, dtype=att_l[0].dtype)
        text_mask = torch.zeros(B, T, dtype=torch.bool)
        for i in range(B):
            n, s = ids_l[i].size(0), sizes[i]
            input_ids[i, T - s - n: T - s] = ids_l[i].unsqueeze(-1)
            attention_mask[i, T - s - n: T - s] = att_l[i]
            text_mask[i, T - s - n: T - s] = att_l[i].bool()
            if s:
                input_ids[i, T - s:] = prm_l[i].t().to(input_ids.dtype)
                attention_mask[i, T - s:] = 1
        return input_ids.to(device), attention_mask.to(device), text_mask.to(device)

    def apply_spk_emb(self, emb, spk_emb, input_ids, device=None):
        return codec.apply_spk_emb(emb, spk_emb, input_ids, self.spk_emb_ids)

    _decode_spk_emb = staticmethod(codec.decode_spk_emb)
    _encode_spk_emb = staticmethod(codec.encode_spk_emb)
    _decode_prompt = staticmethod(codec.decode_prompt)
    _encode_prompt = staticmethod(codec.encode_prompt)
