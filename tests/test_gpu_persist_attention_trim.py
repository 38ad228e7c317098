"""The persistent decode launch after the attention workgroups' critical path was trimmed (persist_layer.hip, "attention trim": the next layer's cached K / V rows
are requested behind a third workgroup barrier, B3, that wave 8 joins behind its last hand-off of the layer): the link moves memory requests off the path between
"q gathered" and "granule published" and changes no operand, rounding or order of an addition, so every output bit must be the one the launch produced before it.

The cases reach every path of the attention workgroups (12 new tokens, device noise with a fixed seed):
  * one row, prompts of 200, 380, 520 and 700 tokens: the register keys only, the LDS tail, two key shares with the merge hop, two shares with a tail;
  * one row, 700 tokens with persistent_splits=1: ONE share of 384 + 256 prefetched keys and a streamed remainder -- the path that keeps the old order;
  * two rows, 520 tokens, one row left-padded by 500: two shares per row, the short row's of about ten keys each (the shares are cut per row, so neither is empty)
    beside the long row's of 260;
  * five rows, 380 tokens;
  * six and eight rows, 150 and 340 tokens: the two-item workgroups (192 register keys, the LDS tail, the streamed part);
  * fp32 engines, and fp16 engines up to 5 rows.
Each case asserts
  * the launch's error word is 0 and the launch ran,
  * against the launch chain (persistent_rows=0) what tests/test_gpu_persist_phase_trim.py asks for: fp32 token ids identical and hiddens <= 5e-5; fp16: the hiddens of
    the steps whose inputs are still identical (the agreeing leading tokens + 1) within 2e-3 relative rms,
  * a SHA-1 over the rows' id and hidden bytes equals the constant below.  The constants were recorded by running exactly these cases (this file, unchanged but for
    the table) against a library built from the commit BEFORE the trim (CTTS_HIP_LIB), on an MI355X; the launch is bitwise reproducible from run to run."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from chatttsplus_amd import _lib, synth

pytestmark = pytest.mark.gpu

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
N, SEED = 12, 11
PADS = [0, 4, 9, 2, 13, 1, 7, 3]

# (rows, prompt, left pads, persistent_splits)
SHAPES = [(1, 200, None, 0), (1, 380, None, 0), (1, 520, None, 0), (1, 700, None, 0), (1, 700, None, 1), (2, 520, (0, 500), 0), (5, 380, None, 0),
          (6, 150, None, 0), (6, 340, None, 0), (8, 150, None, 0), (8, 340, None, 0)]
CASES = [(wd, B, P, pads, splits) for wd in ("fp32", "fp16") for (B, P, pads, splits) in SHAPES if wd == "fp32" or B <= 5]

# (weight dtype, rows, prompt, persistent_splits) -> SHA-1 of the parent commit's ids and hiddens
PARENT_SHA1 = {
    ('fp32', 1, 200, 0): "8c852bc11e287254ad3311eae8ff014a93ada13c",
    ('fp32', 1, 380, 0): "df6397434824e5e56c32d75ace261957721f42c5",
    ('fp32', 1, 520, 0): "5d82605819fcf5535aa586599742f7650fb99cf1",
    ('fp32', 1, 700, 0): "7166827b06177248e04ab39196ca5b1f3bb58693",
    ('fp32', 1, 700, 1): "493898d11d231ed724a0f25e766e3ab2a50d3f2d",
    ('fp32', 2, 520, 0): "2d7505964c06d12c192827bc938db79b8a1c965f",
    ('fp32', 5, 380, 0): "32959b5c55e23cf0e0af24454e67d4b96b404850",
    ('fp32', 6, 150, 0): "a7859dd887539e4fc0dbfb5ebbf8d26610feb064",
    ('fp32', 6, 340, 0): "888629018361158110865e181106e70b1005693e",
    ('fp32', 8, 150, 0): "a17196c4bbbb67b3555f7b3e8d4c5d953c023b37",
    ('fp32', 8, 340, 0): "929c1bd56e90a0aa8a00147dc8b9a18fea56c3e1",
    ('fp16', 1, 200, 0): "beb7de2023d0a0bb17e8ac96a73d5e2dd781a0b9",
    ('fp16', 1, 380, 0): "31720bc4d545cab4a666b873b654703e71971c17",
    ('fp16', 1, 520, 0): "91a996f6559053b119267889eb5db3b493858386",
    ('fp16', 1, 700, 0): "2ffd30da19ff3b789fcb95d207f048bf7afe743d",
    ('fp16', 1, 700, 1): "ebd6173e12b6f12169c23f1ae8d2839109eb52dc",
    ('fp16', 2, 520, 0): "a0cd3f3ac3320afb657fe0b5f68ad5b3c4d4daf8",
    ('fp16', 5, 380, 0): "dd2ef98c2273f9c5df35759358bc44d99e438a5d",
}


@pytest.fixture(scope="module")
def engines():
    from chatttsplus_amd.hip_models import GPT
    made = {}

    def get(wd):
        if wd not in made:
            g = GPT(LLAMA, max_batch=8, max_seq_len=768, weight_dtype=wd)
            g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
            made[wd] = g
        return made[wd]

    yield get
    for g in made.values():
        g.close()


def _state(g):
    buf = np.zeros(8, dtype=np.uint8)
    got = C.c_size_t(0)
    _lib.check(g._lib.ctts_gpt_debug_read(g._h, b"pl_state", buf.ctypes.data_as(C.c_void_p), 8, C.byref(got), g._stream()), "debug_read")
    w = buf.view(np.uint32)
    return int(w[0]), int(w[1])                     # launch counter, error word


def _gen(g, B, P, pads):
    ids, mask = synth.prompt_ids(B, P, 21178, 4321, pad_left=list(pads) if pads is not None else PADS[:B])
    emb = g(torch.from_numpy(ids), torch.ones(B, P, dtype=torch.bool))
    res = list(g.generate(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=N, min_new_token=N,
                          logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="device", seed=SEED))[-1]
    return [i.cpu() for i in res.ids], [h.cpu() for h in res.hiddens]


def _sha1(ids, hid):
    h = hashlib.sha1()
    for i, x in zip(ids, hid):
        h.update(np.ascontiguousarray(i.numpy()).astype(np.int64).tobytes())
        h.update(np.ascontiguousarray(x.numpy()).astype(np.float32).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("wd,B,P,pads,splits", CASES,
                         ids=[f"{wd}-{B}rows-prompt{P}{'-padded' if pads else ''}{'-splits%d' % s if s else ''}" for wd, B, P, pads, s in CASES])
def test_trimmed_attention_leaves_every_output_bit_as_it_was(engines, wd, B, P, pads, splits):
    g = engines(wd)
    default_rows, default_splits = g.get_option("persistent_rows"), g.get_option("persistent_splits")
    try:
        g.set_option("persistent_splits", splits)
        g.set_option("persistent_rows", 0)
        ref_ids, ref_h = _gen(g, B, P, pads)
        g.set_option("persistent_rows", 8)
        e0, _ = _state(g)
        ids, hid = _gen(g, B, P, pads)
        e1, err = _state(g)
    finally:
        g.set_option("persistent_rows", default_rows)
        g.set_option("persistent_splits", default_splits)
    digest = _sha1(ids, hid)
    print(f"attention_trim case=({wd!r}, {B}, {P}, {splits}) sha1={digest} error_word={err} launches={e1 - e0}")
    assert err == 0, f"error word {err}"
    assert e1 > e0, "the persistent launch did not run"
    for b in range(B):
        if wd == "fp32":
            same = torch.equal(ids[b], ref_ids[b])
            herr = float((hid[b] - ref_h[b]).abs().max())
            print(f"  row {b}: ids identical {same}, hidden max abs err {herr:.3g}")
            assert same, f"row {b}: token ids differ from the launch chain"
            assert herr <= 5e-5, f"row {b}: hidden {herr} away from the launch chain"
        else:
            # steps 0..same have the same inputs on both paths (step s consumes the tokens before it): those hiddens are comparable
            same = int((ids[b] == ref_ids[b]).all(-1).to(torch.int32).cumprod(0).sum())
            n = min(same + 1, N)
            rel = float((hid[b][:n] - ref_h[b][:n]).pow(2).mean().sqrt() / ref_h[b][:n].pow(2).mean().sqrt())
            print(f"  row {b}: {same} leading tokens identical, hidden rel rms err {rel:.3g} over {n} steps")
            assert rel <= 2e-3, f"row {b}: hidden states {rel} away from the fp16 launch chain over the {n} steps with identical inputs"
    assert digest == PARENT_SHA1[(wd, B, P, splits)], "the outputs are not bit-identical to the parent commit's"
