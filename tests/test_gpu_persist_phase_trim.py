"""The persistent decode launch after its phases' in-workgroup critical paths were trimmed (persist_layer.hip, "phase trim": the one-row kernels announce a
gather before its norm sums, B1 is the hardware barrier, the act publish shifts by DPP): the trim moves work off the path between "gather complete" and "granule published" and changes no arithmetic, so every output bit must be
the one the launch produced before it.

Each case (1, 2, 5, 6, 8 rows; fp32 and fp16 engines; prompt 40, 24 new tokens, device noise with a fixed seed; one case with per-utterance adapters on the
q / k / v / o projections of 2 rows) asserts
  * the launch's error word is 0 and the launch ran,
  * against the launch chain (persistent_rows=0) the agreement tests/test_gpu_persistent.py asks for: fp32 token ids identical and hiddens <= 5e-5.  An fp16 engine's
    launch chain rounds its MFMA operands to fp16 and the persistent launch does not, so their sampled tokens part sooner or later (on the commit before the trim as
    well: row 1 of the 2-row case after one token); there the hiddens of the steps whose inputs are still identical (the agreeing leading tokens + 1) are held to
    that file's fp16 tolerance, 2e-3 relative rms,
  * a SHA-1 over the rows' id and hidden bytes equals the constant below.  The constants were recorded by running exactly these cases (this file, unchanged
    but for the table) on a build of the commit BEFORE the trim, on an MI355X; the launch is bitwise reproducible from run to run
    (test_persistent_launch_replay_is_bitwise_reproducible_and_graph_equals_eager), so they are properties of the arithmetic, not of a run."""
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
P, N, SEED = 40, 24, 11
PADS = [0, 4, 9, 2, 13, 1, 7, 3]

# (weight dtype, rows, adapters) -> SHA-1 of the parent commit's ids and hiddens
PARENT_SHA1 = {
    ('fp32', 1, False): "6acb36dec47c13a7b010e670c96eb4ee70d57ff6",
    ('fp32', 2, False): "9a427c8a6eb4ba6455571774318bfb9637746cbd",
    ('fp32', 5, False): "662a69a49cae911ccbe099ef1af1b5d20ca24f73",
    ('fp32', 6, False): "05fdd9131ed12f7b4f23594aed298d5d664750a7",
    ('fp32', 8, False): "64ab432999d72f17c82c93c1c3d755f8929043ea",
    ('fp16', 1, False): "4836c4cebcd8511188d65d73f0c1abe33b57f784",
    ('fp16', 2, False): "ff2cebc919b9b9d51285e6e6349f2386109b0bf9",
    ('fp16', 5, False): "ebcd7c6540756b0adbdeb798bc1d477e9ad7d328",
    ('fp16', 6, False): "8c5cd5d7a410af07c5b5a27dd329760c0048fa37",
    ('fp16', 8, False): "f475852e0be9399ed4be55ce104b449f4a954e88",
    ('fp32', 2, True): "025e028bafc06059f7fad770b5b24585b247f284",
}


@pytest.fixture(scope="module")
def engines():
    from chatttsplus_amd.hip_models import GPT
    made = {}

    def get(wd):
        if wd not in made:
            g = GPT(LLAMA, max_batch=8, max_seq_len=96, weight_dtype=wd)
            g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
            rng = np.random.Generator(np.random.Philox(key=53))
            for slot, rank in enumerate((8, 16)):
                g.load_adapter(slot, [(l, t, (rng.standard_normal((rank, 768)) * 0.05).astype(np.float32), (rng.standard_normal((768, rank)) * 0.05).astype(np.float32), 2.0 - 0.5 * slot)
                                      for l in range(20) for t in ("q_proj", "k_proj", "v_proj", "o_proj")])
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


def _gen(g, B, slots):
    g.set_row_adapters(slots)
    try:
        ids, mask = synth.prompt_ids(B, P, 21178, 4321, pad_left=PADS[:B])
        emb = g(torch.from_numpy(ids), torch.ones(B, P, dtype=torch.bool))
        res = list(g.generate(emb, torch.from_numpy(ids), torch.tensor([0.3] * 4), 625, attention_mask=torch.from_numpy(mask), max_new_token=N, min_new_token=N,
                              logits_warpers=LW, logits_processors=LP, return_hidden=True, noise="device", seed=SEED))[-1]
    finally:
        g.set_row_adapters(None)
    return [i.cpu() for i in res.ids], [h.cpu() for h in res.hiddens]


def _sha1(ids, hid):
    h = hashlib.sha1()
    for i, x in zip(ids, hid):
        h.update(np.ascontiguousarray(i.numpy()).astype(np.int64).tobytes())
        h.update(np.ascontiguousarray(x.numpy()).astype(np.float32).tobytes())
    return h.hexdigest()


CASES = [(wd, B, False) for wd in ("fp32", "fp16") for B in (1, 2, 5, 6, 8)] + [("fp32", 2, True)]


@pytest.mark.parametrize("wd,B,adapters", CASES, ids=[f"{wd}-{B}rows{'-adapters' if ad else ''}" for wd, B, ad in CASES])
def test_trimmed_phases_leave_every_output_bit_as_it_was(engines, wd, B, adapters):
    g = engines(wd)
    default_rows = g.get_option("persistent_rows")
    slots = [0, 1] if adapters else None
    try:
        g.set_option("persistent_rows", 0)
        ref_ids, ref_h = _gen(g, B, slots)
        g.set_option("persistent_rows", 8)
        e0, _ = _state(g)
        ids, hid = _gen(g, B, slots)
        e1, err = _state(g)
    finally:
        g.set_option("persistent_rows", default_rows)
    digest = _sha1(ids, hid)
    print(f"phase_trim case=({wd!r}, {B}, {adapters}) sha1={digest} error_word={err} launches={e1 - e0}")
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
    assert digest == PARENT_SHA1[(wd, B, adapters)], "the outputs are not bit-identical to the parent commit's"
