"""generate_many / generate_many_iter served by the DecodeSession driver: the request loop and the session loop are one loop now, and a request must still decode
what it decoded when it had a loop of its own -- the same tokens, hidden rows and log-probs out of the same schedule of admissions and compactions.

Engines: GPT_REAL weights from synth, max_batch 12, max_seq_len 96; fp32 with default options, and one fp16 engine under schedule_invariant=1.  Prompts of 24 tokens
with ragged left padding, max_new_token 20, device noise with a fixed seed, per-utterance limits between 1 and 20.

Each case asserts
  * a SHA-1 over every utterance's ids, hiddens and (where returned) log-prob bytes, and
  * the literal admissions / compactions / shared_prompts lists (sessions: batch_trace; the progress case: a SHA-1 over the yielded events as well)
against the constants below.  They were recorded by running exactly these cases (this file, unchanged but for the table) on a build of the commit BEFORE the request
loop moved onto the driver, on an MI355X.  Runs are bitwise reproducible (test_runs_are_bitwise_reproducible), and on a default-mode engine an utterance's bits depend on
the batch it decoded in, so equal digests also show an equal schedule."""
import hashlib

import numpy as np
import pytest
import torch

from chatttsplus_amd import synth

pytestmark = pytest.mark.gpu

LW = [type("P", (), dict(top_p=0.7, min_tokens_to_keep=3))(), type("K", (), dict(top_k=20))()]
LP = [type("R", (), dict(penalty=1.05, past_window=16, max_input_ids=625))()]
LLAMA = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=20)
T, N, SEED, NU = 24, 20, 29, 14
_rng = np.random.Generator(np.random.Philox(key=71))
PADS = [int(p) for p in _rng.integers(0, 12, size=NU)]
LIMITS = [int(x) for x in _rng.integers(1, N + 1, size=NU)]
UIDS = list(range(300, 300 + NU))
TEMP = torch.tensor([0.3] * 4)

# case -> (SHA-1 of the outputs, the schedule) of the parent commit
PARENT = {
    '4rows-admitNone': ('058184d5fb3c92a340f1825e237c8eb046babc98', ([(17, 3), (25, 1), (41, 3), (57, 3)], [(65, 3), (73, 1)], [])),
    '4rows-admit2': ('f3defde57fa1037e3ae7734927683aadb601b1f7', ([(17, 3), (41, 4), (57, 2), (65, 1)], [(73, 1)], [])),
    '4rows-longest_first': ('dd939ab92123326df533bac175f786b9d755a70b', ([(25, 4), (41, 1), (49, 3), (57, 1), (65, 1)], [(73, 1)], [])),
    '10rows': ('24db6600b34349ea75b6b0a3e821d1a92dcec7cf', ([(17, 4)], [(25, 4), (33, 2)], [])),
    '4rows-eos': ('ac3100b641fd49af4c313496be14bc81a2b358b1', ([(17, 1), (33, 3), (49, 1), (65, 4), (97, 2)], [(105, 2)], [])),
    'prompt_of': ('3c7e1014ce821e9300ada6b9c935a31fc24344f7', ([(17, 3), (25, 1), (41, 1)], [(49, 2)], [(4, 3), (3, 3), (1, 1), (1, 1)])),
    'adapters-sampling': ('599046e4ba88a4b56c317550458d3b64105928fa', ([(17, 3), (25, 1), (41, 3), (57, 3)], [(65, 3), (73, 1)], [])),
    'infer_text': ('3551c4f9620ac0729c5acebcaad456816955e3e2', ([(17, 2), (33, 1), (41, 1)], [(57, 1)], [])),
    'progress-logprobs': ('76cc17ba2cd15b6da145cf0b380ed65a4447cd53', ([(17, 3), (25, 1), (41, 3), (57, 3)], [(65, 3), (73, 1)], [], '5af55f16fc33c9cc4a58434574217c7fb4bae41a')),
    'fp16-invariant': ('bcac9410c1da8ecc8b114a6c6768d86af11537cf', ([(17, 3), (25, 1), (41, 2)], [(49, 3)], [])),
    'session': ('75acad4d6deea6ceae4717f572bb1a3a7208ef2e', [(1, 4), (25, 3), (33, 2)]),
}


@pytest.fixture(scope="module")
def engines():
    from chatttsplus_amd.hip_models import GPT
    made = {}

    def get(wd):
        if wd not in made:
            g = GPT(LLAMA, max_batch=12, max_seq_len=96, weight_dtype=wd, options={"schedule_invariant": 1} if wd == "fp16" else None)
            g.load_state_dict(synth.gpt_state_dict(synth.GPT_REAL, 1234))
            if wd == "fp32":
                rng = np.random.Generator(np.random.Philox(key=53))
                for slot, rank in enumerate((8, 16)):
                    g.load_adapter(slot, [(l, t, (rng.standard_normal((rank, 768)) * 0.05).astype(np.float32), (rng.standard_normal((768, rank)) * 0.05).astype(np.float32),
                                           2.0 - 0.5 * slot) for l in range(20) for t in ("q_proj", "k_proj", "v_proj", "o_proj")])
            ids, mask = synth.prompt_ids(NU, T, 21178, 4321, pad_left=PADS)
            made[wd] = (g, g(torch.from_numpy(ids), torch.ones(NU, T, dtype=torch.bool)), torch.from_numpy(ids), torch.from_numpy(mask))
        return made[wd]

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
    """every utterance's ids, hiddens and, where returned, log-prob bytes"""
    parts = []
    for u in range(len(out.ids)):
        parts.append(out.ids[u])
        if out.hiddens:
            parts.append(out.hiddens[u])
        if out.logprobs is not None:
            parts += [out.logprobs[u], out.sampled_logprobs[u], out.final_logprobs[u]]
    return _sha1(parts)


def _many(eng, n=NU, eos=625, min_new=N, temperature=TEMP, lw=LW, lp=LP, prompts=None, **kw):
    """one generate_many_iter request over the first `n` utterances (`prompts`: the first rows of emb are the prompts of a prompt_of request): the events it
    yielded as (kind, utterance, tokens) and its GenerationOutputs"""
    g, emb, ids, mask = eng
    m = n if prompts is None else prompts
    kw.setdefault("max_new_tokens_per_row", LIMITS[:n])
    gen = g.generate_many_iter(emb[:m], ids[:m], temperature, eos, attention_mask=mask[:m], max_new_token=N, min_new_token=min_new, logits_warpers=lw, logits_processors=lp,
                               seed=SEED, utt_ids=UIDS[:n], **kw)
    events = []
    try:
        while True:
            ev = next(gen)
            if isinstance(ev, tuple) and ev[0] == "progress":
                events += [("progress", int(e[0]), int(e[1])) for e in ev[1]]
            else:
                events += [("done", int(e[0]), int(e[1].shape[0])) for e in ev]
    except StopIteration as stop:
        return events, stop.value


def _check(case, digest, schedule):
    print(f"one_driver case={case!r}: ({digest!r}, {schedule!r}),")
    assert case in PARENT, "no constant of the parent commit for this case"
    assert schedule == PARENT[case][1], "the schedule (admissions, compactions, shared prompts) is not the parent commit's"
    assert digest == PARENT[case][0], "the outputs are not bit-identical to the parent commit's"


def _request(eng, case, hash_events=False, **kw):
    g = eng[0]
    events, out = _many(eng, **kw)
    n = len(out.ids)
    assert sorted(u for k, u, _ in events if k == "done") == list(range(n)), "every utterance is delivered exactly once"
    assert all(int(out.ids[u].shape[0]) == c for k, u, c in events if k == "done"), "what was yielded is final"
    schedule = (list(g.admissions), list(g.compactions), list(g.shared_prompts))
    _check(case, _digest(out), schedule + (_sha1(events),) if hash_events else schedule)
    return events, out


@pytest.mark.parametrize("admit_min", [None, 2], ids=["admit_default", "admit_min2"])
def test_14_utterances_on_4_rows(engines, admit_min):
    _, out = _request(engines("fp32"), f"4rows-admit{admit_min}", rows=4, admit_min=admit_min, return_hidden=True)
    assert [int(i.shape[0]) for i in out.ids] == LIMITS


def test_longest_first_order(engines):
    g = engines("fp32")[0]
    g.schedule = "longest_first"
    try:
        events, out = _request(engines("fp32"), "4rows-longest_first", rows=4, return_hidden=True)
    finally:
        del g.schedule
    assert [int(i.shape[0]) for i in out.ids] == LIMITS, "results come back in input order"


def test_10_rows_compaction_crosses_9_to_8(engines):
    g = engines("fp32")[0]
    _request(engines("fp32"), "10rows", rows=10, return_hidden=True)
    sizes = [r for _, r in g.compactions]
    assert any(a >= 9 and b <= 8 for a, b in zip([10] + sizes, sizes)), f"no compaction from 9 or more rows to 8 or fewer: {g.compactions}"


def test_first_token_eos_is_admitted_again(engines):
    """`eos_token` = a token utterance 3 samples as its very first one (chosen as test_continuous_batching_with_eos_and_regenerate does)"""
    eng = engines("fp32")
    lim = [N] * NU
    _, free = _many(eng, rows=4, max_new_tokens_per_row=lim)
    eos = int(free.ids[3][0, 1])
    _, out = _request(eng, "4rows-eos", eos=eos, min_new=0, rows=4, return_hidden=True, max_new_tokens_per_row=lim)
    assert any(int(i.shape[0]) < N for i in out.ids), "no utterance ended by EOS: the case does not test what it says"
    assert not torch.equal(out.ids[3][:1], free.ids[3][:1]) or out.ids[3].shape[0] == 0
    assert sum(k for _, k in eng[0].admissions) > NU - 4, "no utterance was admitted a second time"


def test_prompt_of_9_utterances_on_3_prompts(engines):
    g = engines("fp32")[0]
    _request(engines("fp32"), "prompt_of", n=9, prompts=3, prompt_of=[0, 1, 2, 0, 0, 1, 2, 2, 1], rows=4, return_hidden=True)
    assert any(p < r for r, p in g.shared_prompts), "no begin / admit call shared a prompt pass"


def test_adapter_slots_with_sampling_per_row(engines):
    slots = [0, None, 1, -1, 0, 1, None, 0, 1, 1, None, 0, -1, 1]
    knobs = [None, dict(temperature=0.7), dict(top_P=0.9, top_K=40), None, dict(repetition_penalty=1.2, past_window=8), dict(top_K=None), None,
             dict(temperature=[0.2, 0.4, 0.6, 0.8]), None, dict(min_new_token=3), dict(top_P=None), None, dict(temperature=1.0, top_K=5), None]
    _request(engines("fp32"), "adapters-sampling", rows=4, adapter_slots=slots, sampling_per_row=knobs, return_hidden=True)


def test_infer_text_6_utterances_on_2_rows(engines):
    _, out = _request(engines("fp32"), "infer_text", n=6, eos=21177, min_new=1, temperature=torch.tensor([0.7]), lp=[], rows=2, infer_text=True)
    assert all(i.dim() == 1 for i in out.ids)


def test_progress_events_with_logprobs(engines):
    """the sequence of yielded events (kind, utterance index, token count) is hashed into the schedule"""
    events, out = _request(engines("fp32"), "progress-logprobs", hash_events=True, rows=4, progress=True, return_logprobs=True, return_hidden=True)
    assert any(k == "progress" for k, *_ in events)


def test_fp16_invariant_engine_10_utterances_on_4_rows(engines):
    _request(engines("fp16"), "fp16-invariant", n=10, rows=4, return_hidden=True)


def test_session_submit_step_cancel_drain(engines):
    """4 submits, two steps, 3 more submits, one cancel of a seated ticket, then drain"""
    g, emb, ids, mask = engines("fp32")
    with g.open_session(TEMP, 625, N, min_new_token=N, logits_warpers=LW, logits_processors=LP, return_hidden=True, return_logprobs=True, seed=SEED, rows=6) as ses:
        tk = [ses.submit(emb[u], mask[u], UIDS[u], limit=LIMITS[u]) for u in range(4)]
        res = ses.step() + ses.step()
        tk += [ses.submit(emb[u], mask[u], UIDS[u], limit=N) for u in range(4, 7)]
        res += ses.step()
        assert ses.cancel(tk[5])
        res += ses.drain()
        trace = list(ses.batch_trace)
    res.sort(key=lambda r: r.ticket)
    assert [r.ticket for r in res] == tk and [r.cancelled for r in res] == [t == tk[5] for t in tk]
    parts = []
    for r in res:
        parts += [r.ids, r.hiddens, r.logprobs, r.sampled_logprobs, r.final_logprobs, (r.finished_by_eos, r.cancelled, r.attempt)]
    _check("session", _sha1(parts), trace)


def test_interrupted_request_leaves_the_engine_free(engines):
    eng = engines("fp32")
    g, emb, ids, mask = eng
    ctx = g.Context()
    gen = g.generate_many_iter(emb, ids, TEMP, 625, attention_mask=mask, max_new_token=N, min_new_token=N, logits_warpers=LW, logits_processors=LP, seed=SEED, utt_ids=UIDS,
                               rows=4, context=ctx, return_hidden=True)
    seen = []
    with pytest.raises(StopIteration):
        while True:
            seen += [int(e[0]) for e in next(gen)]
            ctx.set(True)
    assert 0 < len(seen) < NU, "the request ended at the interrupt, after its first completions"
    assert not g.busy
    out = list(g.generate(emb[:2], ids[:2], TEMP, 625, attention_mask=mask[:2], max_new_token=4, min_new_token=4, logits_warpers=LW, logits_processors=LP, noise="device",
                          seed=SEED))[-1]
    assert [int(i.shape[0]) for i in out.ids] == [4, 4]
