"""bench.py's plain run on the GPU: the headline leg only, `--steps` timed steps, and `--dump-outputs` writing the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_same_outputs_twice(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 12 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "tokens/s" and d["dtype"] == "f32"
        assert d["extra"] is None and d["cpu_baseline"] is None and d["rtf_end_to_end"] is None
    n = 3 + (512 - 12) // 2 + 12                                   # untimed steps before the window + the timed ones
    ids = np.load(tmp_path / "a" / "token_ids.npy")
    hid = np.load(tmp_path / "a" / "hiddens.npy")
    assert ids.shape == (1, n, 4) and ids.dtype == np.float64 and ids.min() >= 0 and ids.max() < 626
    assert hid.shape == (1, n, 768) and hid.dtype == np.float32 and np.isfinite(hid).all() and np.abs(hid[0, -1]).max() > 0
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["hiddens.npy", "token_ids.npy"]
    assert np.array_equal(ids, np.load(tmp_path / "b" / "token_ids.npy"))
    assert np.array_equal(hid, np.load(tmp_path / "b" / "hiddens.npy"))
