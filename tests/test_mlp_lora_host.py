"""LoRA adapters on the MLP projections (gate_proj / up_proj / down_proj beside q/k/v/o): what runs without a GPU.

1. pipeline.load_lora_adapter on a peft-style directory with all seven targets, and the keys / shapes / config switches it refuses.
2. The inputs of tests/test_gpu_mlp_lora.py themselves: the oracle evaluating W x + s B (A x) on all seven targets (LoraOracle below) gives the token ids of the oracle
   with algebraically merged weights (merge_adapter) and hidden rows within 1e-5 -- a GPU failure there cannot be blamed on the adapters.

The helpers (make_adapter, merge_adapter, LoraOracle) are shared with the GPU tests."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chatttsplus_amd import synth
from oracle import ref_cpu

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP = ("gate_proj", "up_proj", "down_proj")
ALL7 = ATTN + MLP
H, I = 768, 3072


def target_shape(t):
    """(out, in) of the nn.Linear a target names (llama.py:214,737-739)."""
    return {"gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}.get(t, (H, H))


def block_of(t):
    return "mlp" if t in MLP else "self_attn"


def make_adapter(rng, layers, targets, r, std=0.05, scale=2.0):
    """[(layer, target, A[r, in], B[out, r], scale)] with A, B ~ N(0, std^2), drawn layer by layer, target by target."""
    ad = []
    for l in range(layers):
        for t in targets:
            out, inn = target_shape(t)
            A = (rng.standard_normal((r, inn)) * std).astype(np.float32)
            B = (rng.standard_normal((out, r)) * std).astype(np.float32)
            ad.append((l, t, A, B, scale))
    return ad


def merge_adapter(sd, adapter):
    """peft merge_and_unload: W + scale * B A on every matrix the adapter names; a copy, `sd` stays."""
    m = {k: v.copy() for k, v in sd.items()}
    for (l, t, A, B, s) in adapter:
        k = f"gpt.layers.{l}.{block_of(t)}.{t}.weight"
        m[k] = (m[k] + s * (B @ A)).astype(np.float32)
    return m


class LoraOracle(ref_cpu.OracleGPT):
    """OracleGPT whose seven projections evaluate W x + s B (A x) with the adapter kept apart from W (what the per-utterance path computes)."""

    def __init__(self, sd, num_heads, adapter):
        super().__init__(sd, num_heads)
        self.ad = {(l, t): (torch.from_numpy(A), torch.from_numpy(B), float(s)) for (l, t, A, B, s) in adapter}

    def _lin(self, x, l, t):
        y = F.linear(x, self.sd[f"gpt.layers.{l}.{block_of(t)}.{t}.weight"])
        if (l, t) in self.ad:
            A, B, s = self.ad[(l, t)]
            y = y + s * F.linear(F.linear(x, A), B)
        return y

    def forward(self, x, attn_mask, position_ids):
        HD = ref_cpu.HEAD_DIM
        B, q, _ = x.shape
        past = self.kv_len
        Ltot = past + q
        minv = torch.finfo(torch.float32).min
        cache_position = torch.arange(past, Ltot)
        causal = torch.full((q, Ltot), minv)
        if q != 1:
            causal = torch.triu(causal, diagonal=1)
        causal = causal * (torch.arange(Ltot) > cache_position.reshape(-1, 1))
        mask4 = causal[None, None].expand(B, 1, -1, -1).clone()
        pad = (mask4 + attn_mask[:, None, None, :Ltot].float()) == 0
        mask4 = mask4.masked_fill(pad, minv)
        cos, sin = self._rope(position_ids)
        cos = cos[:, None]; sin = sin[:, None]
        for l in range(self.L):
            p = f"gpt.layers.{l}."
            res = x
            h = self._rms(x, self.sd[p + "input_layernorm.weight"])
            qs = self._lin(h, l, "q_proj").view(B, q, self.nh, HD).transpose(1, 2)
            ks = self._lin(h, l, "k_proj").view(B, q, self.nh, HD).transpose(1, 2)
            vs = self._lin(h, l, "v_proj").view(B, q, self.nh, HD).transpose(1, 2)
            qs = qs * cos + self._rotate_half(qs) * sin
            ks = ks * cos + self._rotate_half(ks) * sin
            self.kc[l, :, :, past:Ltot] = ks
            self.vc[l, :, :, past:Ltot] = vs
            K = self.kc[l, :, :, :Ltot]; V = self.vc[l, :, :, :Ltot]
            att = torch.softmax(torch.matmul(qs, K.transpose(-1, -2)) / math.sqrt(HD) + mask4, dim=-1)
            o = torch.matmul(att, V).transpose(1, 2).reshape(B, q, self.H)
            x = res + self._lin(o, l, "o_proj")
            res = x
            h = self._rms(x, self.sd[p + "post_attention_layernorm.weight"])
            x = res + self._lin(F.silu(self._lin(h, l, "gate_proj")) * self._lin(h, l, "up_proj"), l, "down_proj")
        self.kv_len = Ltot
        return self._rms(x, self.sd["gpt.norm.weight"])


# ---- 1. the loader ---------------------------------------------------------------------------------------------------------------------------
def _write_adapter(d, tensors, **cfg):
    from safetensors.numpy import save_file
    d.mkdir(parents=True, exist_ok=True)
    save_file(tensors, str(d / "adapter_model.safetensors"))
    (d / "adapter_config.json").write_text(json.dumps(dict(dict(r=8, lora_alpha=16, peft_type="LORA"), **cfg)))


def _peft_tensors(adapter):
    out = {}
    for (l, t, A, B, _) in adapter:
        out[f"base_model.model.layers.{l}.{block_of(t)}.{t}.lora_A.weight"] = A
        out[f"base_model.model.layers.{l}.{block_of(t)}.{t}.lora_B.weight"] = B
    return out


def test_load_lora_adapter_all_seven_targets(tmp_path):
    from chatttsplus_amd.pipeline import load_lora_adapter
    rng = np.random.Generator(np.random.Philox(key=5))
    ad = make_adapter(rng, 2, ALL7, 8)
    _write_adapter(tmp_path / "ok", _peft_tensors(ad), target_modules=list(ALL7))
    got = {(l, t): (A, B, s) for (l, t, A, B, s) in load_lora_adapter(str(tmp_path / "ok"))}
    assert len(got) == 14
    for (l, t, A, B, _) in ad:
        gA, gB, s = got[(l, t)]
        assert s == 2.0 and gA.dtype == np.float32 and gB.dtype == np.float32
        assert gA.shape == (8, target_shape(t)[1]) and gB.shape == (target_shape(t)[0], 8)
        assert np.array_equal(gA, A) and np.array_equal(gB, B)
    # use_rslora: alpha / sqrt(r)
    _write_adapter(tmp_path / "rs", _peft_tensors(ad), use_rslora=True)
    assert all(abs(s - 16.0 / math.sqrt(8.0)) < 1e-12 for (_, _, _, _, s) in load_lora_adapter(str(tmp_path / "rs")))
    # a key that is no decoder-layer projection: refused, naming the key and the file
    bad = dict(_peft_tensors(ad))
    bad["base_model.model.embed_tokens.lora_A.weight"] = np.zeros((8, 100), np.float32)
    bad["base_model.model.embed_tokens.lora_B.weight"] = np.zeros((768, 8), np.float32)
    _write_adapter(tmp_path / "emb", bad)
    with pytest.raises(ValueError, match=r"embed_tokens") as e:
        load_lora_adapter(str(tmp_path / "emb"))
    assert "adapter_model.safetensors" in str(e.value)
    # what peft really writes for such parts: an embedding adapter (lora_embedding_A / _B) and a modules_to_save copy -- no 'lora_A' in the key, refused all the same
    for name, key, shape in (("pemb", "base_model.model.embed_tokens.lora_embedding_A", (8, 100)), ("mts", "base_model.model.head_code.0.modules_to_save.weight", (626, 768)),
                             ("norm", "base_model.model.layers.0.input_layernorm.weight", (768,))):
        _write_adapter(tmp_path / name, dict(_peft_tensors(ad), **{key: np.zeros(shape, np.float32)}))
        with pytest.raises(ValueError, match=key.split(".")[-2]) as e:
            load_lora_adapter(str(tmp_path / name))
        assert key in str(e.value) and "adapter_model.safetensors" in str(e.value)
    # a lora_B without its lora_A
    lone = dict(_peft_tensors(ad)); del lone["base_model.model.layers.0.mlp.up_proj.lora_A.weight"]
    _write_adapter(tmp_path / "lone", lone)
    with pytest.raises(ValueError, match=r"up_proj\.lora_B"):
        load_lora_adapter(str(tmp_path / "lone"))
    # peft's adapter-name infix is accepted
    named = {k.replace(".weight", ".default.weight"): v for k, v in _peft_tensors(ad).items()}
    _write_adapter(tmp_path / "named", named)
    assert len(load_lora_adapter(str(tmp_path / "named"))) == 14
    # a target under the wrong block
    wrong = {"base_model.model.layers.0.self_attn.gate_proj.lora_A.weight": ad[4][2], "base_model.model.layers.0.self_attn.gate_proj.lora_B.weight": ad[4][3]}
    _write_adapter(tmp_path / "blk", wrong)
    with pytest.raises(ValueError, match=r"self_attn\.gate_proj"):
        load_lora_adapter(str(tmp_path / "blk"))
    # a transposed lora_B of down_proj
    tr = dict(_peft_tensors(ad))
    k = "base_model.model.layers.1.mlp.down_proj.lora_B.weight"
    tr[k] = np.ascontiguousarray(tr[k].T)
    _write_adapter(tmp_path / "tr", tr)
    with pytest.raises(ValueError, match=r"layer 1 down_proj") as e:
        load_lora_adapter(str(tmp_path / "tr"))
    assert "(8, 768)" in str(e.value)
    # DoRA: refused by name
    _write_adapter(tmp_path / "dora", _peft_tensors(ad), use_dora=True)
    with pytest.raises(ValueError, match="use_dora"):
        load_lora_adapter(str(tmp_path / "dora"))


# ---- 2. the GPU tests' inputs: separate evaluation == merged weights on the oracle -------------------------------------------------------------
def merged_inputs():
    """tests/test_gpu_mlp_lora.py, merged adapters: 3 layers, one adapter on all seven targets, r 8."""
    cfg = dict(synth.GPT_REAL); cfg["num_hidden_layers"] = 3
    return cfg, synth.gpt_state_dict(cfg, 1234), [make_adapter(np.random.Generator(np.random.Philox(key=31)), 3, ALL7, 8)]


def per_row_inputs(layers=4):
    """tests/test_gpu_mlp_lora.py, per-utterance adapters, drawn one after the other from Philox key 77 (the seed of
    test_gpu_pipeline.py::test_per_utterance_lora_matches_per_row_merged_oracle): slot 0 all seven targets r 8, slot 1 gate / up / down only r 4, slot 2 q/k/v/o only r 16."""
    cfg = dict(synth.GPT_REAL); cfg["num_hidden_layers"] = layers
    rng = np.random.Generator(np.random.Philox(key=77))
    return cfg, synth.gpt_state_dict(cfg, 1234), [make_adapter(rng, layers, ALL7, 8), make_adapter(rng, layers, MLP, 4), make_adapter(rng, layers, ATTN, 16)]


def score_inputs_adapter():
    """tests/test_gpu_mlp_lora.py, GPT.score: the weights of tests/test_gpu_score.py (4 layers, seed 4321), one adapter on all seven targets, r 8."""
    cfg = dict(synth.GPT_REAL, num_hidden_layers=4)
    return cfg, synth.gpt_state_dict(cfg, 4321), [make_adapter(np.random.Generator(np.random.Philox(key=83)), 4, ALL7, 8)]


CASES = {"merged": merged_inputs, "per_row": per_row_inputs, "per_row_6_layers": lambda: per_row_inputs(6), "score": score_inputs_adapter}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_separate_lora_equals_merged_weights(name):
    """Every adapter the GPU tests load, on the weights they load it beside (and the per-row set also at the 6 layers of the q/k/v/o test it is modelled on): 3 left-padded
    rows, 8 sampled steps, A, B ~ N(0, 0.05^2), scale 2.  The oracle evaluating W x + s B (A x) (LoraOracle) and the oracle with merged weights: identical token
    ids, hiddens within 1e-5; and an adapter with MLP targets moves most token ids away from the base model's, so "the adapter changed nothing" cannot pass by accident.
    (The difference is fp32 rounding and grows with depth and rank: an adapter no GPU test uses -- all seven targets at r 16 over 6 layers, same seed -- measured 1.26e-5
    with identical ids.)"""
    cfg, sd, ads = CASES[name]()
    B, T, N = 3, 14, 8
    ids, mask = synth.prompt_ids(B, T, cfg["num_text_tokens"], 19, pad_left=[0, 3, 5])
    q = torch.from_numpy(np.stack([synth.exp_noise(31, i, 4 * B, 626) for i in range(N)]))

    def run(o):
        emb = o.embed(torch.from_numpy(ids), torch.ones(B, T, dtype=torch.bool))
        return o.generate(emb, torch.from_numpy(ids), ref_cpu.SamplerParams(min_new_token=N), attention_mask=torch.from_numpy(mask), max_new_token=N, noise=ref_cpu.ArrayNoise(q))
    base = run(ref_cpu.OracleGPT(sd, 12))
    for ai, ad in enumerate(ads):
        merged, sep = run(ref_cpu.OracleGPT(merge_adapter(sd, ad), 12)), run(LoraOracle(sd, 12, ad))
        worst, moved = 0.0, 0
        for b in range(B):
            assert torch.equal(merged.ids[b], sep.ids[b]), f"adapter {ai} row {b}: W x + s B (A x) and (W + s B A) x sample different tokens"
            worst = max(worst, float((merged.hiddens[b] - sep.hiddens[b]).abs().max()))
            moved += int((merged.ids[b] != base.ids[b]).sum())
        print(f"{name} adapter {ai} ({len(ad) // int(cfg['num_hidden_layers'])} targets, r {ad[0][2].shape[0]}): max |d hidden| {worst:.3e}, {moved} of {B * N * 4} ids moved")
        assert worst <= 1e-5, (name, ai, worst)
        if any(t in MLP for (_, t, _, _, _) in ad):
            assert moved >= B * N * 4 // 2, "the adapter changes too little to test anything"
