"""bench.py's plain run: one JSON line with the headline fields, and --dump-outputs writes what the timed call computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    """--steps sets the timed steps; the dumped ids are the timed call's (their tail is the line's greedy_tail) and the dumped logits are its last step's
    (their arg-max is the last id); the plain line carries none of --full's legs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "small", "--steps", "6", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 6 and res["value"] > 0 and abs(res["ms_per_step"] * res["value"] - 1e3) < 1e-6 * 1e3
    assert not {"roofline", "cpu_baseline", "decode_512", "kernels", "prefill"} & set(res)
    ids = np.load(tmp_path / "ids.npy")
    logits = np.load(tmp_path / "logits.npy")
    assert ids.dtype == np.float64 and ids.shape == (6,) and logits.dtype == np.float32
    assert [int(t) for t in ids[-4:]] == res["greedy_tail"]
    assert int(np.argmax(logits)) == int(ids[-1])
