"""A plain bench.py run (no --full): the result line carries the headline and nothing that needs work of its own, and
--dump-outputs writes what the last timed step computed -- float32 / float64 arrays, at most 64 MB, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args):
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(lines[0])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(a)])
    run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(b)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    for key in ("roofline", "stages_ms_per_launch", "ref_checksum", "cpu_baseline", "parity_check", "slice_search"):
        assert key not in line, "%s is --full's" % key
    da, db = load(a), load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 1000 * 1000
    assert da["recon_y"].shape == (1088, 1920) and da["recon_u"].shape == (544, 960)
    assert da["me_mv"].shape == (8160, 41, 2) and da["luma_levels"].shape == (8160, 16, 16)
    assert sorted(da) == sorted(db)
    for k in da:
        assert da[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(da[k], db[k]), "%s differs between two runs with the same arguments" % k
    # the step really coded something: vectors found, coefficients left, a picture that is not flat
    assert np.abs(da["me_mv"]).sum() > 0 and np.abs(da["luma_levels"]).sum() > 0 and da["recon_y"].std() > 1
