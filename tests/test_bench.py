"""bench.py as it is run for every change: a plain run (set-up, warm-up, the timed steps, the line) and the outputs of its last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--size", "40", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("newton_iterations_per_sec", "iter/s", True, "f64")
    assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    for k in ("roofline", "roofline_solver", "solver", "contact", "cpu_baseline", "roofline_large"):  # --full only
        assert k not in d, k

    from ipc_amd import scene
    V0, _ = scene.make_mat(40)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {"positions", "search_direction", "gradient", "state_scalars"}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert got["positions"].shape == V0.shape and got["search_direction"].shape == V0.shape and got["gradient"].shape == V0.shape
    assert np.abs(got["positions"] - V0).max() > 0  # the twist moved the sheet
    assert got["state_scalars"].shape == (8,)
