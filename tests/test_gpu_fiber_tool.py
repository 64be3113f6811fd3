"""`tools/run_scene.py --fields` on a tiny scene whose shape carries `fiber ... activate ... ramp`: the files gain the cell data `fiberStretch` and `fiberDir`,
the ramp contracts the cube step by step; the same scene without the keyword writes the files it always wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ipc_amd import scene, vtu_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
HEAD = "shapes input 1\ncube.msh 0 1 0  0 0 90  1 1 1"
TAIL = "\ndensity 1000\nstiffness 1e5 0.4\ntime 1 0.02\nturnOffGravity\n"
FIBER = " fiber 5e4 dir 1 0 0 activate 0.3 ramp 0.06"


def _run(tmp_path, name, text):
    (tmp_path / f"{name}.txt").write_text(text)
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_scene.py"), str(tmp_path / f"{name}.txt"), "--root", str(tmp_path), "--steps", str(STEPS), "--out", str(out),
           "--fields", str(out / "fields")]
    os.makedirs(out, exist_ok=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return [vtu_io.read_vtu(out / "fields" / f"fields{n + 1}.vtu") for n in range(STEPS)]


def test_fields_carry_the_fibre_stretch_and_direction(gpu_lib, tmp_path):
    V, F = scene.make_box(2, 2, 2, size=(0.1, 0.1, 0.1), origin=(-0.05, -0.05, -0.05))
    gpu_lib.lib.save_tet_mesh(tmp_path / "cube.msh", V, F)
    R = _run(tmp_path, "fibred", HEAD + FIBER + TAIL)
    nT = len(F)
    mean = []
    for n, r in enumerate(R):
        assert list(r["cell_data"]) == ["stress", "von_mises", "J", "fiberStretch", "fiberDir"]
        l, t = r["cell_data"]["fiberStretch"], r["cell_data"]["fiberDir"]
        assert l.shape == (nT,) and t.shape == (nT, 3) and np.all(np.isfinite(l)) and np.all(np.abs(np.linalg.norm(t, axis=1) - 1.0) <= 1e-14)
        # dir 1 0 0 of the file, turned by the shape line's 90 degrees about z: along y (an unturned direction would have t_y near 0); the moving cube tilts it a little
        assert np.all(np.abs(t[:, 1]) > 0.999)
        mean.append(float(l.mean()))
    print(f"mean fibre stretch per step: {mean}")
    assert 1.0 > mean[0] > mean[1] > mean[2] > 0.75  # act = 0.1, 0.2, 0.3 at the ends of the three steps: the cube contracts along its fibres
    ext = R[-1]["points"].max(0) - R[-1]["points"].min(0)
    assert ext[1] < 0.095 < 0.1 < ext[0]  # shorter along y, bulging along x
    P = _run(tmp_path, "plain", HEAD + TAIL)
    for r in P:
        assert list(r["cell_data"]) == ["stress", "von_mises", "J"]
        assert "fiberStretch" not in r["cell_data"] and "fiberDir" not in r["cell_data"] and "fiberStretch" not in r["point_data"]
    for n in range(STEPS):
        assert "fiber" not in open(tmp_path / "plain" / "fields" / f"fields{n + 1}.vtu").read()
