"""bench.py's command line: a plain run prints ONE result line for the
headline q7 workload, --steps sets the number of timed steps, and
--dump-outputs writes the last timed step's group states, checked here
against a numpy restatement of max(price), count(*) by window over the same
seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_options_present():
    out = subprocess.run([sys.executable, BENCH, "--help"], check=True,
                         capture_output=True, text=True).stdout
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out, f"bench.py --help lacks {opt}"


@pytest.mark.gpu
def test_plain_run_one_line_and_dump(tmp_path):
    steps, warmup, seed = 2, 1, 1
    dump = tmp_path / "out"
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps),
         "--warmup", str(warmup), "--seed", str(seed),
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"plain run printed {len(lines)} lines"
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in res, f"result line lacks {k}"
    assert res["steps"] == steps and res["warmup"] == warmup
    assert res["config"]["workload"] == "nexmark_q7"
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    rows = steps * res["config"]["rows_per_step"]
    assert res["value"] == pytest.approx(
        rows / (steps * res["ms_per_step"] * 1e-3), rel=1e-9)
    # what --full adds is absent from a plain run
    assert res["checkpoint"] is None and res["cpu_baseline"] is None

    sys.path.insert(0, REPO)
    import bench

    w, p = bench.make_q7_epoch(np.random.default_rng(seed), 0, 64)
    keys, first, counts = np.unique(w, return_index=True, return_counts=True)
    assert np.all(np.diff(w) >= 0)  # reduceat below needs contiguous groups
    want_max = np.maximum.reduceat(p, first)
    # every step (warmup included) re-applies the same epoch of rows
    want_count = counts * (steps + warmup)

    got = {n: np.load(dump / f"{n}.npy")
           for n in ("q7_window", "q7_max_price", "q7_count")}
    for a in got.values():
        assert a.dtype == np.float64
    np.testing.assert_array_equal(got["q7_window"], keys.astype(np.float64))
    np.testing.assert_array_equal(got["q7_max_price"],
                                  want_max.astype(np.float64))
    np.testing.assert_array_equal(got["q7_count"],
                                  want_count.astype(np.float64))
