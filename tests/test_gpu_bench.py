"""GPU: bench.py's plain run (set up, warm up, time the steps, print the line) and `--dump-outputs`: the headline keys of
the line, the dumped files, and that the dumped scores are the very ones a `--full` run -- every extra fit and leg around
the timed steps, the oracle check of the timed output among them -- computes for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS = 20000


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(ROWS), "--speakers", "1000",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)] + list(extra),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dump_match_the_full_run(tmp_path):
    plain = _bench(tmp_path / "plain")
    assert plain["metric"] == "PLDA LLR trials/sec" and plain["unit"] == "trials/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f32" and plain["steps"] == 3 and plain["warmup"] == 1 and plain["full"] is False
    assert plain["ms_per_step"] > 0
    assert abs(plain["value"] * plain["ms_per_step"] / 1e3 - ROWS * ROWS) <= 1e-9 * ROWS * ROWS   # value = trials / step time
    assert plain["roofline"]["launches"] == 3
    for k in ("oracle_check", "cpu_baseline", "eer", "znorm_stats", "transform", "bf16x3_arm", "targetdim150", "end_to_end",
              "fit_skewed"):
        assert k not in plain, k
    files = {f: np.load(tmp_path / "plain" / f) for f in ("scores.npy", "score_rows.npy", "score_cols.npy")}
    S, rows, cols = files["scores.npy"], files["score_rows.npy"], files["score_cols.npy"]
    assert S.dtype == np.float32 and rows.dtype == cols.dtype == np.float64
    assert S.shape == (rows.size, cols.size) == (1024, 4096) and np.isfinite(S).all()
    assert rows[0] == cols[0] == 0 and rows[-1] == cols[-1] == ROWS - 1 and (np.diff(rows) > 0).all()

    full = _bench(tmp_path / "full", "--full", "--no-cpu")
    assert full["full"] is True and full["oracle_check"]["within_1e-4"] is True and "fit_skewed" in full
    for f, a in files.items():
        np.testing.assert_array_equal(np.load(tmp_path / "full" / f), a)
