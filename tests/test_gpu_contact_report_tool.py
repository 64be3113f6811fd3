"""`tools/run_scene.py --contact-report`: the file it writes, and that a run with the flag ends where a run without it ends."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ipc_amd import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
TEXT = "shapes input 2\ncube.msh 0 0.504 0  0 0 0  1 1 1\ncube.msh 0.25 1.507 0  0 0 0  1 1 1\n\nselfFric 0.1\n\nground 0.1 0\n"


def test_tool_writes_the_report_and_takes_the_same_steps(gpu_lib, tmp_path):
    V, F = scene.make_box(2, 2, 2, size=(1.0, 1.0, 1.0), origin=(-0.5, -0.5, -0.5))
    gpu_lib.lib.save_tet_mesh(tmp_path / "cube.msh", V, F)
    (tmp_path / "scene.txt").write_text(TEXT)
    status = []
    for name, extra in (("with", ["--contact-report", str(tmp_path / "rep")]), ("without", [])):
        out = tmp_path / name
        os.makedirs(out)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_scene.py"), str(tmp_path / "scene.txt"), "--root", str(tmp_path), "--steps", str(STEPS),
               "--status-every", str(STEPS), "--out", str(out)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        status.append(open(out / f"status{STEPS}").read())
    assert status[0] == status[1]  # positions, velocities, accelerations: 20 digits each
    a = np.loadtxt(tmp_path / "rep" / "contact.txt", ndmin=2)
    assert a.shape[1] == 29 and set(a[:, 0]) <= set(range(1, STEPS + 1)) and a.shape[0] > 0
    last = a[a[:, 0] == STEPS]
    assert np.all(np.diff(last[:, 1]) >= 0) and np.all(last[last[:, 2] >= 0][:, 1] <= last[last[:, 2] >= 0][:, 2])
    assert np.all(last[:, 9] < 1e-4)  # squared distances below the scene's dHat
