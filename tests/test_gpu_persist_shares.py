"""The decode path of a step (key splits of the attention, key shares of the persistent launch) follows that step's own context, not the length of the
ctts_gpt_decode call it is launched in: one generation decoded as a single call, as 32-step calls (generate()'s default) and as 4-step calls runs the same
kernels at every step, so token ids, hidden rows and the KV cache are bit-identical.  The contexts cross the persistent launch's share boundaries (one share
up to 512 keys at one row; two shares beyond) inside one call."""
import pytest
import torch

from chatttsplus_amd import synth

pytestmark = pytest.mark.gpu

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)


@pytest.fixture(scope="module")
def gpt():
    from chatttsplus_amd.hip_models import GPT
    g = GPT(LLAMA, max_batch=2, max_seq_len=1024, weight_dtype="fp32")
    g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
    yield g
    g.close()


def _gen(g, B, P, N, chunk):
    ids, mask = synth.prompt_ids(B, P, 21178, 4321)
    emb = g(torch.from_numpy(ids), torch.ones(B, P, dtype=torch.bool))
    saved = g.chunk_steps
    g.chunk_steps = chunk
    try:
        res = list(g.generate(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=N,
                              min_new_token=N, logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="device", seed=11))[-1]
    finally:
        g.chunk_steps = saved
    torch.cuda.synchronize()
    return res.ids, res.hiddens, g._kv.clone()


@pytest.mark.parametrize("B,P", [(1, 48), (1, 460), (2, 48), (2, 460)])
def test_a_generation_is_bit_identical_however_its_decode_calls_are_chunked(gpt, B, P):
    g = gpt
    assert g.get_option("persistent_rows") >= B
    N = 512
    ref_ids, ref_h, ref_kv = _gen(g, B, P, N, N)          # one ctts_gpt_decode call for steps 1..511
    for chunk in (32, 4):
        ids, hid, kv = _gen(g, B, P, N, chunk)
        for b in range(B):
            assert torch.equal(ids[b], ref_ids[b]), f"B={B} P={P} chunk={chunk}: row {b} token ids differ from the single-call decode"
            assert torch.equal(hid[b], ref_h[b]), f"B={B} P={P} chunk={chunk}: row {b} hidden rows differ from the single-call decode"
        assert torch.equal(kv, ref_kv), f"B={B} P={P} chunk={chunk}: KV cache differs from the single-call decode"
