"""The engine's per-row host state (gpt_engine.hip: HostRow, the requests for the next call, the prompt-pass loop, check_rows) against a recording of the commit
before that state became one record per row: tools/engine_rows_trace.py's script -- two lives of a generate state through begin, admit, grow, compact, cancel,
admit_adapters, admit_sampling, admit_modes, enable_text_rows, share_prompts, and three refused calls -- is replayed on the four engines and compared with
tests/golden/engine_rows_trace.json.

Required in all four engines: everything the host decides (return codes, error texts, decode plans, meta_dec, options, row reports) equals the recording.  The output
arrays (ids, finish, end_idx, both log-prob arrays, text ids) equal it bit for bit in the two invariant-mode engines, which is their contract, and in the two
default-mode engines as well: the golden's "parent_runs_agree" records that two recordings of the parent library agreed with each other in every engine, calls and
outputs, so no tolerance is needed (the test fails loudly should a re-recorded golden ever say otherwise)."""
import json
import os

import pytest

from tools import engine_rows_trace as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_rows_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype,inv", T.ENGINES, ids=[T.engine_name(d, i) for d, i in T.ENGINES])
def test_rows_trace_equals_the_parent_recording(golden, dtype, inv):
    name = T.engine_name(dtype, inv)
    assert golden["parent_runs_agree"][name] == dict(calls=True, outputs=True), "the golden's two parent recordings disagree: bit-identity cannot be required of this engine"
    want = golden["engines"][name]
    got = json.loads(json.dumps(T.record(dtype, inv)))
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in want["calls"]], "the script changed: re-record the golden at the parent commit"
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert not (g.get("must_succeed") and g["rc"] != 0), f"{name}: call {i} ({g['call']}) must succeed: {g.get('error')}"
        assert g == w, f"{name}: call {i} ({g['call']}) differs from the recording in {sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))}:\n got  {g}\n want {w}"
    for part, w in want["outputs"].items():
        for arr, d in w.items():
            assert got["outputs"][part][arr] == d, f"{name}: {part}: {arr} differs from the recording: got {got['outputs'][part][arr]}, want {d}"
