"""bench.py's command line: a plain run does the headline alone, --full adds the legs, checks and baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv", [[], ["--full"], ["--full", "--no-cpu-baseline", "--gpus", "2", "--dump-outputs", "d"],
                                  ["--no-cpu-baseline", "--side-steps", "0", "--sides-out", "s.json"]])
def test_other_form_gets_the_same_options(argv):
    """An N > 1 run that falls back to the other multi-GPU form hands its child every option, --full included."""
    import bench
    a = bench.parse(argv)
    child = vars(bench.parse(bench._forwarded_args(a)))
    assert child.pop("no_fallback") is True
    want = vars(a)
    want.pop("no_fallback")
    assert child == want


def test_full_is_off_by_default():
    import bench
    assert bench.parse([]).full is False
    assert bench.parse(["--full"]).full is True


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(lib_built, tmp_path):
    """A plain run prints the contract keys and the headline's roofline, writes --dump-outputs, and runs no other leg."""
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "300000", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(dump)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3 and line["full"] is False
    assert line["roofline"]["bytes_per_launch"] > 0
    assert set(line["roofline"]) & {"section_8d_kernel", "other_filter_copy", "encoder_minilm", "encoder_bge"} == set()
    for key in ("cpu_baseline", "sides", "sides_file"):
        assert key not in line, key
    assert line["recall_at_10"] is None
    assert set(line["wall_s"]) == {"headline (build + timed steps)"}
    ids, nf = np.load(dump / "ids.npy"), np.load(dump / "n_found.npy")
    assert ids.shape == (256, 10) and (nf == 10).all()
    assert ((ids >= 1) & (ids <= 300000)).all()
