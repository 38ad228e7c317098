"""Trace of the engine's per-row host state (chatttsplus_amd/csrc/gpt_engine.hip) through one scripted life of a generate state, driven through the C ABI with the
`Raw` driver of tests/test_gpu_session.py on the 4-layer synthetic engine of tests/test_gpu_score.py.  tests/test_gpu_engine_rows_trace.py replays the script and
compares with the recording in tests/golden/engine_rows_trace.json, which was taken with the library of the commit BEFORE the host state became one record per row.

The script, per engine (fp32 and fp16, each with batch_invariant / schedule_invariant 1 and 0):
  life 1   set_row_sampling (2 of 5 sequences), set_row_adapters (slot 0: q/k/v/o, slot 1: gate/up/down), share_prompts (5 sequences on 3 prompts), begin B = 5, prefill,
           sample; decode 3, cancel row 1, decode 2; compact to rows 0, 2, 4; grow 2; admit_sampling + admit_adapters + share_prompts + admit of 2 utterances on 1 prompt
           into the grown rows; decode 4; compact (drops the last row whose slot holds MLP targets); decode to the end.  Invariant engines leave the adapter calls out --
           the contract refuses them -- and record that refusal once, at begin.
  life 2   set_row_modes seats one text row among 3, enable_text_rows, decode 5, admit_modes + admit of a text utterance into a finished row, decode 4, compact (one
           text row left), decode 2, compact (none left), decode to the end.
  refusals an admit naming a row twice; a begin with a share table of the wrong length -- between an admit_sampling and the admit it was meant for, which still seats
           those knobs: a begin refused before it touches the generate state leaves the admission requests alone; an admit of a text row with knobs.  Each is followed
           by a plain begin that must succeed.
Every compaction keeps a fixed row set (the dropped rows have reached their token limits or were cancelled), so the calls made do not depend on the tokens sampled.
After every call: return code, ctts_last_error() on failure, the options "text_rows_live" / "lora_mlp_live" / "persistent_active" (null where the engine has no such
option), debug_read "meta_dec" for the rows of the batch, ctts_gpt_rows_enqueue's report, after a decode also debug_read "decode_plan".  At the end of each part the output
arrays (ids, finish, end_idx, both log-prob arrays, the text ids) as sha256 digests plus their first values.

    python tools/engine_rows_trace.py --out trace.json                # the four engines (CTTS_HIP_LIB selects the library)
    python tools/engine_rows_trace.py --merge a.json b.json --out tests/golden/engine_rows_trace.json      # two recordings -> the golden, with "parent_runs_agree"
    python tools/engine_rows_trace.py --time --out timing.jsonl       # 3 x 200 ctts_gpt_admit + ctts_gpt_compact pairs, host time per call"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENGINES = [("fp32", 1), ("fp32", 0), ("fp16", 1), ("fp16", 0)]
OPTIONS = ("text_rows_live", "lora_mlp_live", "persistent_active")
TXT_NEW = 20


def engine_name(dtype, inv):
    return f"{dtype}-{'invariant' if inv else 'default'}"


def _engine(dtype, inv):
    from tests.test_gpu_score import engine
    opts = {} if not inv else ({"batch_invariant": 1} if dtype == "fp32" else {"schedule_invariant": 1})
    return engine(dtype, opts, max_batch=8, max_seq=64)      # engines of this trace alone: the adapters loaded below stay out of the other tests' engines


def _digest(t):
    a = t.detach().cpu().contiguous().numpy()
    return dict(shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest(), head=[float(x) if a.dtype.kind == "f" else int(x) for x in a.reshape(-1)[:8]])


def _driver():
    """the class is built on first use: importing this module needs neither torch nor a GPU"""
    import numpy as np
    import torch
    from chatttsplus_amd import _lib
    from chatttsplus_amd.hip_models.gpt import row_sampling_from_values, sampler_cfg_from_objects
    from tests.test_gpu_session import LW, MAX_NEW, T_MAX, TEXT_EOS, FILL_I, Raw

    class Life(Raw):
        """Raw + the calls it lacks, every call recorded"""

        def __init__(self, g, n_out, calls):
            super().__init__(g, n_out)
            self.calls, self.B = calls, 0
            self.tsc = sampler_cfg_from_objects(torch.tensor([0.7]), TEXT_EOS, TXT_NEW, 1, LW, [], 4, infer_text=True)
            self.tids = torch.full((n_out, TXT_NEW, 4), FILL_I, dtype=torch.int32, device=g.device)
            self.pin = torch.zeros(2 * _lib.MAX_BATCH, dtype=torch.int32).pin_memory()

        def arr(self, v, dt=np.int32):
            a = np.ascontiguousarray(v, dtype=dt)
            self.keep.append(a)
            return a.ctypes.data_as(C.c_void_p)

        def knobs(self, entries):
            k = (_lib.RowSampling * len(entries))(*[row_sampling_from_values(self.sc, e, 4) for e in entries])
            self.keep.append(k)
            return k

        def note(self, call, rc, plan=False, **extra):
            rec = dict(call=call, rc=int(rc), **extra)
            if rc != 0:
                rec["error"] = self.lib.ctts_last_error().decode()
            opts = {}
            for name in OPTIONS:
                v = C.c_int(0)
                opts[name] = int(v.value) if self.lib.ctts_gpt_get_option(self.h, name.encode(), C.byref(v)) == 0 else None
            rec["options"] = opts
            if self.lib.ctts_gpt_rows_enqueue(self.h, self.pin.data_ptr(), self.st) == 0:      # (refused without a generate state)
                meta = np.zeros((_lib.MAX_BATCH, 4), dtype=np.int32)
                nb = C.c_size_t(0)
                _lib.check(self.lib.ctts_gpt_debug_read(self.h, b"meta_dec", meta.ctypes.data_as(C.c_void_p), meta.nbytes, C.byref(nb), self.st), "debug_read")      # synchronises
                rec["B"], rec["rows"], rec["meta_dec"] = self.B, self.pin[:2 * self.B].tolist(), meta[:self.B].reshape(-1).tolist()
            else:
                rec["B"] = rec["rows"] = rec["meta_dec"] = None
            if plan:
                v = np.zeros(23, dtype=np.int32)
                nb = C.c_size_t(0)
                prc = self.lib.ctts_gpt_debug_read(self.h, b"decode_plan", v.ctypes.data_as(C.c_void_p), v.nbytes, C.byref(nb), self.st)
                rec["decode_plan"] = v.tolist() if prc == 0 else None
            self.calls.append(rec)
            return rc

        def begin(self, us, uids, lims, B=None, must_succeed=False):
            """prompts `us` of the pool ([P][T] rows: P < B under share_prompts); on success also set_logprob_out, prefill, sample"""
            B = B or len(us)
            e, m = self._sel(us)
            uid, lim = np.ascontiguousarray(uids, dtype=np.uint64), np.ascontiguousarray(lims, dtype=np.int32)
            io = _lib.GenIO(ids=self.ids.data_ptr(), hiddens=self.hid.data_ptr(), finish=self.fin.data_ptr(), end_idx=self.end.data_ptr(), noise=None, n_draws=0,
                            seed=self.seed, utt_ids=uid.ctypes.data, row_limits=lim.ctypes.data)
            rc = self.lib.ctts_gpt_begin(self.h, B, T_MAX, m.data_ptr(), C.byref(self.sc), C.byref(io), self.st)
            if rc == 0:
                self.B = B
            self.note("begin", rc, must_succeed=must_succeed)
            self.prompt = e
            return rc

        def start(self, text_rows=False):
            if text_rows:
                self.note("enable_text_rows", self.lib.ctts_gpt_enable_text_rows(self.h, C.byref(self.tsc), self.tids.data_ptr(), self.st))
            self.note("set_logprob_out", self.lib.ctts_gpt_set_logprob_out(self.h, self.lp[0].data_ptr(), self.lp[1].data_ptr(), self.st))
            self.note("prefill", self.lib.ctts_gpt_prefill(self.h, self.prompt.data_ptr(), self.st))
            self.note("sample", self.lib.ctts_gpt_sample(self.h, self.st))

        def decode(self, n, graph=1):
            self.note(f"decode {n}", self.lib.ctts_gpt_decode(self.h, n, graph, self.st), plan=True)

        def grow(self, n):
            rc = self.lib.ctts_gpt_grow(self.h, n, self.st)
            if rc == 0:
                self.B += n
            return self.note(f"grow {n}", rc)

        def cancel(self, rows):
            return self.note(f"cancel {rows}", self.lib.ctts_gpt_cancel(self.h, len(rows), self.arr(rows), self.st))

        def compact(self, keep):
            rc = self.lib.ctts_gpt_compact(self.h, self.arr(keep), len(keep), self.st)
            if rc == 0:
                self.B = len(keep)
            return self.note(f"compact {keep}", rc)

        def admit(self, rows, us, uids, lims, outs):
            e, m = self._sel(us)
            rc = self.lib.ctts_gpt_admit(self.h, len(rows), self.arr(rows), T_MAX, m.data_ptr(), e.data_ptr(), self.arr(uids, np.uint64), self.arr(lims), self.arr(outs), None, self.st)
            return self.note(f"admit {rows}", rc)

        def share(self, prompt_of, P):
            return self.note(f"share_prompts {prompt_of}", self.lib.ctts_gpt_share_prompts(self.h, len(prompt_of), self.arr(prompt_of) if prompt_of else None, P))

        def row_sampling(self, entries):
            return self.note("set_row_sampling", self.lib.ctts_gpt_set_row_sampling(self.h, self.knobs(entries) if entries else None, len(entries or [])))

        def row_adapters(self, slots):
            return self.note(f"set_row_adapters {slots}", self.lib.ctts_gpt_set_row_adapters(self.h, self.arr(slots) if slots else None, len(slots or [])))

        def row_modes(self, modes):
            return self.note(f"set_row_modes {modes}", self.lib.ctts_gpt_set_row_modes(self.h, self.arr(modes) if modes else None, len(modes or [])))

        def admit_sampling(self, rows, entries):
            return self.note(f"admit_sampling {rows}", self.lib.ctts_gpt_admit_sampling(self.h, len(rows), self.arr(rows), self.knobs(entries), self.st))

        def admit_adapters(self, rows, slots):
            return self.note(f"admit_adapters {rows} {slots}", self.lib.ctts_gpt_admit_adapters(self.h, len(rows), self.arr(rows), self.arr(slots), self.st))

        def admit_modes(self, rows, modes):
            return self.note(f"admit_modes {rows} {modes}", self.lib.ctts_gpt_admit_modes(self.h, len(rows), self.arr(rows), self.arr(modes), self.st))

        def outputs(self):
            steps, alld = C.c_int32(0), C.c_int32(0)
            rc = self.lib.ctts_gpt_progress(self.h, C.byref(steps), C.byref(alld), self.st)
            torch.cuda.synchronize()
            return dict(progress=[int(rc), int(steps.value), int(alld.value)], ids=_digest(self.ids), finish=_digest(self.fin), end_idx=_digest(self.end),
                        logprobs=_digest(self.lp[0]), sampled_logprobs=_digest(self.lp[1]), text_ids=_digest(self.tids))

    return Life, MAX_NEW


def record(dtype, inv):
    """the script on one engine -> {"calls": [...], "outputs": {part: digests}}"""
    from tests.test_gpu_session import _adapter
    Life, MAX_NEW = _driver()
    g = _engine(dtype, inv)
    calls, outputs = [], {}
    try:
        if not inv:
            g.load_adapter(0, _adapter(91, ("q_proj", "k_proj", "v_proj", "o_proj")))
            g.load_adapter(1, _adapter(92, ("gate_proj", "up_proj", "down_proj")))
        # ---- life 1: knobs, adapters, shared prompts; cancel, compact, grow, admit ----------------------------------------------------------
        c = Life(g, 7, calls)
        uids, lims = [500, 501, 502, 503, 504], [24, 24, 24, 6, 10]
        c.row_sampling([None, dict(temperature=0.9), None, dict(temperature=0.5, top_K=10), None])
        c.row_adapters([0, 0, -1, 1, 1])
        c.share([0, 0, 1, 2, 2], 3)
        if inv:      # the contract refuses per-utterance adapters: once, at begin; the call consumed the share table
            c.begin([0, 1, 2], uids, lims, B=5)
            c.row_adapters(None)
            c.share([0, 0, 1, 2, 2], 3)
        c.begin([0, 1, 2], uids, lims, B=5, must_succeed=True)
        c.start()
        c.decode(3)
        c.cancel([1])
        c.decode(2)
        c.compact([0, 2, 4])                         # row 1 was cancelled, row 3 has its 6 tokens
        c.grow(2)
        c.admit_sampling([3], [dict(temperature=0.5)])
        if not inv:
            c.admit_adapters([3, 4], [0, 0])
        c.share([0, 0], 1)
        c.admit([3, 4], [5], [510, 511], [24, 8], [5, 6])
        c.decode(4)
        c.compact([0, 1, 3, 4])                      # row 2 (sequence 4: the last row on the MLP slot) has its 10 tokens
        c.decode(MAX_NEW + 2)
        c.row_sampling(None)
        c.row_adapters(None)
        outputs["life 1"] = c.outputs()
        # ---- life 2: text rows beside code rows ------------------------------------------------------------------------------------------------
        c = Life(g, 4, calls)
        c.row_modes([0, 1, 0])
        c.begin([6, 7, 8], [506, 507, 508], [4, 8, 24], must_succeed=True)
        c.row_modes(None)
        c.start(text_rows=True)
        c.decode(5)
        c.admit_modes([0], [1])
        c.admit([0], [9], [509], [3], [3])           # row 0 has its 4 tokens
        c.decode(4)
        c.compact([1, 2])                            # the admitted text row has its 3 tokens: one text row left (finished: 10 steps, limit 8)
        c.decode(2)
        c.compact([1])                               # the code row alone
        c.decode(MAX_NEW)
        outputs["life 2"] = c.outputs()
        # ---- three refusals, each followed by a plain begin -----------------------------------------------------------------------------------
        c = Life(g, 4, calls)
        us, uids, lims = [10, 11, 12], [520, 521, 522], [24, 24, 24]
        c.begin(us, uids, lims, must_succeed=True)
        c.start()
        c.admit([1, 1], [13, 14], [523, 524], [24, 24], [3, 3])
        c.begin(us, uids, lims, must_succeed=True)
        c.start()
        c.decode(2)
        c.cancel([1])
        c.admit_sampling([1], [dict(temperature=0.9)])
        c.share([0, 0], 1)
        c.begin(us, uids, lims)                      # 2 prompts named, B = 3: refused before the state is touched
        c.admit([1], [13], [523], [24], [3])         # ... and the state goes on, with the knobs named for this admission
        c.decode(6)
        outputs["after the refused begin"] = c.outputs()
        c.begin(us, uids, lims, must_succeed=True)
        c.start(text_rows=True)
        c.decode(2)
        c.admit_sampling([1], [dict(temperature=0.9)])
        c.admit_modes([1], [1])
        c.admit([1], [13], [523], [24], [3])
        c.begin(us, uids, lims, must_succeed=True)
        c.start()
        c.decode(3)
        outputs["refusals"] = c.outputs()
    finally:
        g._lib.ctts_gpt_set_row_sampling(g._h, None, 0)
        g._lib.ctts_gpt_set_row_modes(g._h, None, 0)
        g._lib.ctts_gpt_set_row_adapters(g._h, None, 0)
        g._lib.ctts_gpt_share_prompts(g._h, 0, None, 0)
    return dict(calls=calls, outputs=outputs)


def dumps(doc):
    """one call per line: the golden stays readable in a diff"""
    out = ["{"]
    for k, v in doc.items():
        if k != "engines":
            out.append(f" {json.dumps(k)}: {json.dumps(v)},")
    out.append(' "engines": {')
    names = list(doc["engines"])
    for name in names:
        e = doc["engines"][name]
        out.append(f"  {json.dumps(name)}: {{")
        out.append(f'   "outputs": {json.dumps(e["outputs"])},')
        out.append('   "calls": [')
        out.append(",\n".join("    " + json.dumps(c) for c in e["calls"]))
        out.append("   ]")
        out.append("  }" + ("," if name != names[-1] else ""))
    out.append(" }")
    out.append("}")
    return "\n".join(out) + "\n"


def merge(a, b):
    """two recordings of one library -> the golden: the first, plus where the second differed from it"""
    agree = {}
    for name, ea in a["engines"].items():
        eb = b["engines"][name]
        agree[name] = dict(calls=ea["calls"] == eb["calls"], outputs=ea["outputs"] == eb["outputs"])
    doc = dict(note="recorded by tools/engine_rows_trace.py with the library of the commit before gpt_engine.hip kept one host record per decode row; "
                    "parent_runs_agree: two recordings of that library, compared per engine", parent_runs_agree=agree)
    doc["engines"] = a["engines"]
    return doc


def time_pairs(out):
    """3 x 200 (grow 1 +) ctts_gpt_admit + ctts_gpt_compact on the fp32 default engine at 8 rows: host time inside the two calls, the stream drained between pairs"""
    import numpy as np
    import torch
    Life, _ = _driver()
    g = _engine("fp32", 0)
    lib, PAIRS = g._lib, 200
    for run in range(3):
        c = Life(g, 8, [])
        c.begin(list(range(8)), list(range(600, 608)), [24] * 8)
        c.start()
        assert all(r["rc"] == 0 for r in c.calls), c.calls
        keep, rows, outs = c.arr(list(range(7))), c.arr([7]), c.arr([7])
        t_admit, t_compact = [], []
        for i in range(PAIRS):
            e, m = c._sel([8 + i % 8])
            uid = c.arr([700 + i], np.uint64)
            lim = c.arr([24])
            t0 = time.perf_counter()
            rc1 = lib.ctts_gpt_compact(c.h, keep, 7, c.st)
            t1 = time.perf_counter()
            rc2 = lib.ctts_gpt_grow(c.h, 1, c.st)
            t2 = time.perf_counter()
            rc3 = lib.ctts_gpt_admit(c.h, 1, rows, 14, m.data_ptr(), e.data_ptr(), uid, lim, outs, None, c.st)
            t3 = time.perf_counter()
            assert rc1 == 0 and rc2 == 0 and rc3 == 0, lib.ctts_last_error().decode()
            torch.cuda.synchronize()
            t_compact.append(t1 - t0)
            t_admit.append(t3 - t2)
        rec = dict(tool="engine_rows_trace --time", lib=os.environ.get("CTTS_HIP_LIB", "in-tree"), run=run, pairs=PAIRS, admit_us_median=round(1e6 * float(np.median(t_admit)), 2),
                   compact_us_median=round(1e6 * float(np.median(t_compact)), 2), pairs_total_ms=round(1e3 * (sum(t_admit) + sum(t_compact)), 3))
        print(json.dumps(rec), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--merge", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.merge:
        a, b = (json.load(open(p)) for p in args.merge)
        doc = merge(a, b)
        print(json.dumps(doc["parent_runs_agree"]))
    elif args.time:
        return time_pairs(args.out)
    else:
        doc = dict(lib=os.environ.get("CTTS_HIP_LIB", "in-tree"), engines={})
        for dtype, inv in ENGINES:
            t0 = time.time()
            doc["engines"][engine_name(dtype, inv)] = record(dtype, inv)
            print(engine_name(dtype, inv), len(doc["engines"][engine_name(dtype, inv)]["calls"]), "calls", round(time.time() - t0, 2), "s", flush=True)
    with open(args.out, "w") as f:
        f.write(dumps(doc))


if __name__ == "__main__":
    main()
