"""bench.py end to end at a small size: a plain run prints the headline without the --full figures, --steps sets the number of
timed steps, and --dump-outputs writes the same arrays on every run with the same arguments (what lets two builds of the project
be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, INNER, MESHLETS = 3, 2, 200_000
NAMES = ["counters", "hiz_sample", "indices_late", "visibility_mask", "visible_early", "visible_late"]


def plain_run(tmp_path, tag):
    env = dict(os.environ, OXC_BENCH_FULL=str(tmp_path / f"{tag}_full.json"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--meshlets", str(MESHLETS),
           "--inner-reps", str(INNER), "--dump-outputs", str(tmp_path / tag)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    a = plain_run(tmp_path, "a")
    assert a["metric"] == "meshlets/s culled" and a["unit"] == "meshlets/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    assert a["steps"] == STEPS and a["config"]["frames_timed"] == STEPS * INNER and a["config"]["meshlets_per_gpu"] == MESHLETS
    assert a["ms_per_step"] > 0 and a["value"] > 0
    assert abs(a["ms_per_step"] - a["config"]["ms_per_frame"] * INNER) <= 1e-3 * a["ms_per_step"]
    assert a["roofline"] is None and a["cpu_baseline"] is None and "bit_match" not in a  # the --full figures stay out of a plain run
    b = plain_run(tmp_path, "b")
    assert sorted(f[:-4] for f in os.listdir(tmp_path / "a")) == NAMES
    arrays = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    for n, x in arrays.items():
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, np.load(tmp_path / "b" / f"{n}.npy")), n  # same arguments, same inputs, same outputs
    assert sum(x.nbytes for x in arrays.values()) <= 64 << 20
    total, early, late, index_count = arrays["counters"]
    assert total == MESHLETS and early == arrays["visible_early"].size and late == arrays["visible_late"].size and late > 0
    assert arrays["indices_late"].size == min(index_count, 1 << 20) and arrays["visibility_mask"].size >= (MESHLETS + 31) // 32
    assert np.all(np.diff(arrays["visible_late"]) >= 0) and arrays["visible_late"].max() < MESHLETS
