"""generate() keeps its engine calls, its bits and torch's generator while its driver is taken apart: every case runs one call with the engine's library wrapped
in a recording proxy and asserts, against the constants below,
  * the trace: every ctts_gpt_* call with its scalar arguments and the contents of its host arrays (compact's keep rows, share_prompts' table, admit / grow /
    cancel's rows, begin's configuration, utterance ids and limits); pointers into device memory are not recorded, and calls that only clear a staged request
    (set_row_sampling(NULL, 0), set_row_modes(NULL, 0), share_prompts(h, 0, NULL, 0), set_row_adapters(None)) are left out: where they happen is not part of the
    contract.  The constant is the trace's SHA-1; the literal trace is printed by every run.
  * a SHA-1 over every sequence's ids, hiddens and (where returned) log-probs, of every yielded result, and
  * a SHA-1 of torch.random.get_rng_state() after the call (torch.manual_seed before it).
The trace is deterministic: both loops of generate() block on an event of the oldest chunk in flight and never poll.

Engines: GPT_REAL weights from synth, 20 layers, max_batch 12, max_seq_len 96; fp32 with default options (and one built with compact=False), and one fp16 engine under
schedule_invariant=1.  Prompts of 24 tokens with ragged left padding, max_new_token 20.

The constants were recorded by running exactly these cases (this file, unchanged but for the table) on a build of the commit BEFORE generate()'s driver was
refactored, on an MI355X, once; they are not re-recorded.  The file uses no name that refactor introduced (the staging test, which compares with no recorded
constant, reads engine attributes that commit has under the same names)."""
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
T, N, SEED, TSEED, NU = 24, 20, 29, 1207, 10
_rng = np.random.Generator(np.random.Philox(key=83))
PADS = [int(p) for p in _rng.integers(0, 12, size=NU)]
LIMITS = [int(x) for x in _rng.integers(1, N + 1, size=NU)]
UIDS = list(range(500, 500 + NU))
TEMP = torch.tensor([0.3] * 4)

# case -> (SHA-1 of the trace, SHA-1 of the outputs, SHA-1 of torch's RNG state after the call[, more]) of the parent commit
PARENT = {
    'b1-auto': ('917771f84aca6372b76ef8ca051ba0bcdfb67a27', 'c94fb3ab08e4959c75749076547a052d05cccbf4', '6336330b753d71cd25f750b2b79957dc6fd4b6db'),
    'b4-auto': ('8c69e162746c16b43073b24d9d0530499bfd76e5', '96c1567854ab1e28d60fe65c44bdfc62b660fdd7', '8f6d33168a6a7fb11373698655367aa689e9face'),
    'b5-auto': ('df0f8aa73aa6e69a7816c4a995adbaa1c752f998', 'c8bcdd60fc7ac720a9f0105bd762338f4f8cc80c', '99b41e37d358c7f7a663b38ce36ea21e1f8d3b98'),
    'b1-text': ('bbe0b8f738cbc96c82e78fec69c3c2b653de432c', 'a2c7672a57aacd65c6420de7f31196d48c39e810', '99b41e37d358c7f7a663b38ce36ea21e1f8d3b98'),
    'b2-array': ('7d8a206563f1208de2b576ee8145aedbaf7223f0', '382204e449c03d98842bc63dbd1fccebd282a7af', '9e5269baf295d27e2e1e670692c136fef023a9d5'),
    'b4-stream': ('1d6e9928932247606b4067359d5269480c51eeed', '88be2d00d55bb68939105b46bf423c3aaa9f2930', '8f6d33168a6a7fb11373698655367aa689e9face'),
    'b4-stream-last': ('2e0640f2142467a1ec6a201370fa5a1ef328baf0', '3cc2a03e0caf5435e9985c50f8f751da7fc5ad71', '94cf29bc2d542279000f67c706b7edad3a01e2aa'),
    'b10-compact': ('a0580fbdafa9a2df613f8db150546a33ac130c69', 'c1aa3629078ab9d704e25c6590a63e211e38f9b8', '9e5269baf295d27e2e1e670692c136fef023a9d5', [(17, 6)]),
    'b10-nocompact': ('aabca52d4ac7fe770e257051821491a4c6ba5139', 'c1aa3629078ab9d704e25c6590a63e211e38f9b8', '9e5269baf295d27e2e1e670692c136fef023a9d5', []),
    'b1-restart': ('6bdbebb7609c8226eea60d0267405edc2047739f', '59d17d1d5a1928f8a5a4cd1da1a41bcf6ea81e00', '9e5269baf295d27e2e1e670692c136fef023a9d5'),
    'b1-giveup': ('1fccbd403cc97e7b1e0d4e21b4519dd733a700e2', 'da39a3ee5e6b4b0d3255bfef95601890afd80709', '9e5269baf295d27e2e1e670692c136fef023a9d5'),
    'b6-share-knobs-lp': ('30c770d3afda9fd623c743d7f7d5a89dad7248ba', '92433323fb1b006d2e0fa875d2101dfdf6655bd9', '9e5269baf295d27e2e1e670692c136fef023a9d5'),
    'b3-context': ('bede33afdb149ea60337be4c0ade4a8da2f567b6', '0935538af599d7dbf2b57304156f74d09a9c47c8', '088a8be4f1b7621f817b67da8340b61410fb64f9'),
    'fp16-invariant-b5': ('df0f8aa73aa6e69a7816c4a995adbaa1c752f998', '857ca8d5e10ab949dccf5ff3ac24efaf0b0ef39d', '99b41e37d358c7f7a663b38ce36ea21e1f8d3b98'),
    'session-begin': ('189eca8ff9bc70beefdc69d15be4899fa75018e0', 'b0656e0521af3597065a0548c4e0ee8615a6d366', '9e5269baf295d27e2e1e670692c136fef023a9d5', [(1, 2), (25, 1)]),
}


# ---- the recording proxy -------------------------------------------------------------------------------------------------------------------------
def _addr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if isinstance(x, C.c_void_p):
        return x.value or 0
    return C.addressof(getattr(x, "_obj", x))          # byref(struct), a ctypes array or structure


def _host(x, n, ctype=C.c_int32):
    """the n values of a host array argument (None for NULL)"""
    a = _addr(x)
    return None if not a or int(n) <= 0 else [int(v) for v in (ctype * int(n)).from_address(a)]


def _bytes(x, nbytes) -> str:
    """a host structure (sampler configuration, sampling knobs) by the SHA-1 of its bytes"""
    a = _addr(x)
    return None if not a or nbytes <= 0 else hashlib.sha1(C.string_at(a, nbytes)).hexdigest()[:12]


def _io(x, B):
    io = _lib.GenIO.from_address(_addr(x))
    return (int(io.n_draws), int(io.seed), bool(io.noise), bool(io.hiddens), _host(io.utt_ids, B, C.c_uint64), _host(io.row_limits, B))


_SC, _RS = C.sizeof(_lib.SamplerCfg), C.sizeof(_lib.RowSampling)
# arguments after the handle: a[0] is the first of them
RECORD = {
    "begin": lambda a: (int(a[0]), int(a[1]), _bytes(a[3], _SC), _io(a[4], a[0])),
    "decode": lambda a: (int(a[0]), int(a[1])),
    "compact": lambda a: (int(a[1]), _host(a[0], a[1])),
    "admit": lambda a: (int(a[0]), _host(a[1], a[0]), int(a[2]), _host(a[5], a[0], C.c_uint64), _host(a[6], a[0]), _host(a[7], a[0]), _host(a[8], a[0])),
    "grow": lambda a: (int(a[0]),),
    "cancel": lambda a: (int(a[0]), _host(a[1], a[0])),
    "admit_adapters": lambda a: (int(a[0]), _host(a[1], a[0]), _host(a[2], a[0])),
    "admit_sampling": lambda a: (int(a[0]), _host(a[1], a[0]), _bytes(a[2], int(a[0]) * _RS)),
    "admit_modes": lambda a: (int(a[0]), _host(a[1], a[0]), _host(a[2], a[0])),
    "set_row_sampling": lambda a: (int(a[1]), _bytes(a[0], int(a[1]) * _RS)),
    "set_row_modes": lambda a: (int(a[1]), _host(a[0], a[1])),
    "set_row_adapters": lambda a: (int(a[1]), _host(a[0], a[1])),
    "share_prompts": lambda a: (int(a[0]), _host(a[1], a[0]), int(a[2])),
    "enable_text_rows": lambda a: (_bytes(a[0], _SC),),
    "set_logprob_out": lambda a: (bool(_addr(a[0])), bool(_addr(a[1]))),
}
CLEARS = ("set_row_sampling", "set_row_modes", "set_row_adapters", "share_prompts")      # with NULL / 0: a staged request is cleared


class Recorder:
    """stands in for the engine's library handle: ctts_gpt_* calls are noted in `calls`, everything is passed through"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ctts_gpt_"):
            return fn
        short = name[len("ctts_gpt_"):]

        def call(*args):
            entry = (short,) + RECORD[short](args[1:]) if short in RECORD else (short,)
            if not (short in CLEARS and entry[2] is None):       # (entry[2]: the host array, None for NULL)
                self.calls.append(entry)
            return fn(*args)
        return call


# ---- engines and digests -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from chatttsplus_amd.hip_models import GPT
    made = {}

    def get(name):
        if name not in made:
            g = GPT(LLAMA, max_batch=12, max_seq_len=96, weight_dtype="fp16" if name == "fp16" else "fp32", compact=name != "nocompact",
                    options={"schedule_invariant": 1} if name == "fp16" else None)
            g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
            ids, mask = synth.prompt_ids(NU, T, 21178, 4321, pad_left=PADS)
            emb = g(torch.from_numpy(ids), torch.ones(NU, T, dtype=torch.bool))
            g._lib = Recorder(g._lib)
            made[name] = (g, emb, torch.from_numpy(ids), torch.from_numpy(mask))
        return made[name]

    yield get
    for g, *_ in made.values():
        g.close()


def _sha1(parts) -> str:
    h = hashlib.sha1()
    for p in parts:
        if p is None:
            h.update(b"none")
        elif isinstance(p, torch.Tensor):
            a = p.detach().cpu().numpy()
            h.update(np.ascontiguousarray(a).astype(np.int64 if a.dtype.kind in "iu" else np.float32).tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def _digest(out) -> str:
    """every sequence's ids, hiddens and, where returned, log-prob bytes"""
    parts = []
    for u in range(len(out.ids)):
        parts.append(out.ids[u])
        if out.hiddens:
            parts.append(out.hiddens[u])
        if out.logprobs is not None:
            parts += [out.logprobs[u], out.sampled_logprobs[u], out.final_logprobs[u]]
    return _sha1(parts)


def _run(eng, n, prompts=None, on_yield=None, eos=625, temperature=TEMP, lw=LW, lp=LP, max_new=N, min_new=None, **kw):
    """one generate() call over the first `n` sequences (`prompts`: of a prompt_of call, the first rows of emb): (yielded results, trace, digest, RNG digest)"""
    g, emb, ids, mask = eng
    m = n if prompts is None else prompts
    g._lib.calls = []
    torch.manual_seed(TSEED)
    outs = []
    for o in g.generate(emb[:m], ids[:m], temperature, eos, attention_mask=mask[:m], max_new_token=max_new, min_new_token=max_new if min_new is None else min_new,
                        logits_warpers=lw, logits_processors=lp, return_hidden=True, **kw):
        outs.append(o)
        if on_yield is not None:
            on_yield(o)
    rng = _sha1([torch.random.get_rng_state()])
    return outs, list(g._lib.calls), _sha1([_digest(o) for o in outs]), rng


def _check(case, trace, digest, rng, *more):
    got = (_sha1([trace]), digest, rng) + more
    print(f"generate_driver trace of {case!r}: {trace!r}")
    print(f"generate_driver case: {case!r}: {got!r},")
    assert case in PARENT, "no constant of the parent commit for this case"
    assert got[0] == PARENT[case][0], "the engine calls are not the parent commit's (the trace is printed above)"
    assert got[1] == PARENT[case][1], "the outputs are not bit-identical to the parent commit's"
    assert got[2] == PARENT[case][2], "torch's CPU generator is not left where the parent commit left it"
    assert got[3:] == tuple(PARENT[case][3:])


def _names(trace):
    return [c[0] for c in trace]


def _noise_kind(trace) -> str:
    """what begin was given: a noise buffer (torch's draws or a caller's array) or the device generator"""
    io = next(c for c in trace if c[0] == "begin")[4]
    return "buffer" if io[2] else "device"


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4])
def test_auto_noise_is_torch_up_to_4_sequences(engines, n):
    outs, trace, digest, rng = _run(engines("fp32"), n)
    assert _noise_kind(trace) == "buffer" and len(outs) == 1 and [int(i.shape[0]) for i in outs[0].ids] == [N] * n
    _check(f"b{n}-auto", trace, digest, rng)


def test_auto_noise_is_device_from_5_sequences_and_draws_the_seed(engines):
    outs, trace, digest, rng = _run(engines("fp32"), 5, seed=None)
    assert _noise_kind(trace) == "device"
    torch.manual_seed(TSEED)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert next(c for c in trace if c[0] == "begin")[4][1] == seed, "the seed is one draw from torch's generator"
    assert rng == _sha1([torch.random.get_rng_state()]), "and nothing else was drawn"
    _check("b5-auto", trace, digest, rng)


def test_auto_noise_is_device_for_the_text_head(engines):
    outs, trace, digest, rng = _run(engines("fp32"), 1, eos=21177, temperature=torch.tensor([0.7]), lp=[], infer_text=True)
    assert _noise_kind(trace) == "device" and outs[0].ids[0].dim() == 1
    _check("b1-text", trace, digest, rng)


def test_callers_noise_array_sets_n_draws(engines):
    q = torch.empty(12, 2 * 4, 626).exponential_(1, generator=torch.Generator().manual_seed(5))
    outs, trace, digest, rng = _run(engines("fp32"), 2, noise=q)
    assert next(c for c in trace if c[0] == "begin")[4][:3] == (12, 0, True)
    _check("b2-array", trace, digest, rng)


@pytest.mark.parametrize("max_new, yields", [(20, [6, 12, 18, 20]), (18, [6, 12, 18, 18])], ids=["stream", "stream-last"])
def test_streamed_yields(engines, max_new, yields):
    """a partial result whenever the token count is a multiple of stream_batch, then the final one -- which repeats the last partial one where they coincide"""
    outs, trace, digest, rng = _run(engines("fp32"), 4, stream=True, stream_batch=6, max_new=max_new)
    assert [int(o.ids[0].shape[0]) for o in outs] == yields
    _check("b4-stream" if max_new == 20 else "b4-stream-last", trace, digest, rng)


@pytest.mark.parametrize("name", ["fp32", "nocompact"], ids=["compact", "nocompact"])
def test_10_sequences_with_own_limits(engines, name):
    g = engines(name)[0]
    outs, trace, digest, rng = _run(engines(name), 10, noise="device", seed=SEED, utt_ids=UIDS, max_new_tokens_per_row=LIMITS)
    assert [int(i.shape[0]) for i in outs[-1].ids] == LIMITS
    if name == "fp32":
        sizes = [r for _, r in g.compactions]
        assert sizes and any(a >= 9 and b <= 8 for a, b in zip([10] + sizes, sizes)), f"no compaction from 9 or more rows to 8 or fewer: {g.compactions}"
        assert [c[1] for c in trace if c[0] == "compact"] == sizes
    else:
        assert "compact" not in _names(trace) and "rows_enqueue" not in _names(trace)
    _check(f"b10-{name if name == 'nocompact' else 'compact'}", trace, digest, rng, list(g.compactions) if name == "fp32" else [])


@pytest.mark.parametrize("ensure", [True, False], ids=["restart", "giveup"])
def test_first_token_eos(engines, ensure):
    """the utterance id of test_gpu_gen_logprobs: under its HOT knobs and SEED5 the device noise draws EOS at attempt 0 and not at attempt 1"""
    from tests.test_gpu_gen_logprobs import HOT, SEED5, _restart_uid
    outs, trace, digest, rng = _run(engines("fp32"), 1, min_new=0, noise="device", seed=SEED5, utt_ids=[_restart_uid()], sampling_per_row=[dict(HOT)],
                                    ensure_non_empty=ensure)
    if ensure:
        assert _names(trace).count("restart") == 1 and len(outs) == 1 and int(outs[0].ids[0].shape[0]) >= 1
    else:
        assert outs == [] and "restart" not in _names(trace) and "decode" not in _names(trace)       # the reference's bare return
    _check("b1-restart" if ensure else "b1-giveup", trace, digest, rng)


def test_shared_prompts_knobs_logprobs_then_a_plain_call(engines):
    eng = engines("fp32")
    knobs = [None, dict(temperature=0.7, top_K=5), None, None, dict(repetition_penalty=1.2, past_window=8), None]
    outs, trace, digest, rng = _run(eng, 6, prompts=3, prompt_of=[0, 0, 1, 1, 2, 2], sampling_per_row=knobs, return_logprobs=True, noise="device", seed=SEED)
    assert eng[0].shared_prompts == [(6, 3)] and outs[0].logprobs is not None
    _check("b6-share-knobs-lp", trace, digest, rng)
    outs, trace, digest, rng = _run(eng, 4)                # nothing stayed staged: the plain call is the plain call
    _check("b4-auto", trace, digest, rng)


def test_context_set_by_the_consumer_ends_the_call_at_the_next_chunk(engines):
    g = engines("fp32")[0]
    ctx = g.Context()
    outs, trace, digest, rng = _run(engines("fp32"), 3, stream=True, stream_batch=6, context=ctx, on_yield=lambda o: ctx.set(True))
    assert [int(o.ids[0].shape[0]) for o in outs] == [6, 6] and not g.busy
    _check("b3-context", trace, digest, rng)


def test_fp16_invariant_engine_auto_noise_is_device(engines):
    outs, trace, digest, rng = _run(engines("fp16"), 5, seed=None)
    assert _noise_kind(trace) == "device"
    _check("fp16-invariant-b5", trace, digest, rng)


def test_session_begin_with_a_code_and_a_text_utterance(engines):
    g, emb, ids, mask = engines("fp32")
    g._lib.calls = []
    torch.manual_seed(TSEED)
    with g.open_session(TEMP, 625, N, min_new_token=N, logits_warpers=LW, logits_processors=LP, return_hidden=True, return_logprobs=True, seed=SEED, rows=4,
                        text_rows=dict(eos_token=21177, max_new_token=12, min_new_token=12)) as ses:
        tk = [ses.submit(emb[0], mask[0], UIDS[0]), ses.submit(emb[1], mask[1], UIDS[1], mode="text")]
        res = sorted(ses.drain(), key=lambda r: r.ticket)
        batch_trace = list(ses.batch_trace)
    trace = list(g._lib.calls)
    assert [r.ticket for r in res] == tk and [r.mode for r in res] == ["code", "text"] and [int(r.ids.shape[0]) for r in res] == [N, 12]
    assert _names(trace)[:6] == ["set_row_modes", "begin", "enable_text_rows", "set_logprob_out", "prefill", "sample"]
    parts = []
    for r in res:
        parts += [r.ids, r.hiddens, r.logprobs, r.sampled_logprobs, r.final_logprobs, (r.finished_by_eos, r.cancelled, r.attempt)]
    _check("session-begin", trace, _sha1(parts), _sha1([torch.random.get_rng_state()]), batch_trace)


def test_torch_noise_staging_is_cached_on_the_engine_by_its_shape(engines):
    """the pinned staging slots are keyed (multinomial rows, vocabulary, draws per upload) and pinned once per key, not once per call"""
    g = engines("fp32")[0]
    _run(engines("fp32"), 4)
    key, bufs = g._stage_key, g._stage_bufs
    assert key == (4 * 4, 626, max(g.chunk_steps, 1)) and len(bufs) == 3 and all(b[0].is_pinned() and tuple(b[0].shape) == (key[2],) + key[:2] for b in bufs)
    _run(engines("fp32"), 4)
    _run(engines("fp32"), 5, noise="device", seed=SEED)           # (device noise leaves the slots alone)
    assert g._stage_key == key and g._stage_bufs is bufs
    _run(engines("fp32"), 1)
    assert g._stage_key == (4, 626, key[2]) and g._stage_bufs is not bufs
    _run(engines("fp32"), 1, stream=True, stream_batch=40)       # an upload covers a whole streamed chunk
    assert g._stage_key == (4, 626, 40)


def test_runs_are_bitwise_reproducible(engines):
    """what makes the constants meaningful: the same call twice gives the same trace and the same bits"""
    kw = dict(noise="device", seed=SEED, utt_ids=UIDS, max_new_tokens_per_row=LIMITS)
    a, b = _run(engines("fp32"), 10, **kw), _run(engines("fp32"), 10, **kw)
    assert a[1:] == b[1:]
    a, b = _run(engines("fp32"), 4), _run(engines("fp32"), 4)
    assert a[1:] == b[1:]
