"""`tools/run_scene.py --fields` and the writer behind it (`scene_script.FieldsWriter`) on the layout of tutorialExamples/2cubesFall.txt -- two unit cubes
above a ground plane with friction, self-contact with friction, a cube of the scene helpers in place of the reference's mesh file -- placed so that contact
happens within the first steps: the lower cube starts 4e-3 above the ground, the upper one 3e-3 above the lower (both a little more than the barrier's
reach, sqrt(dHat) = 2.6e-3) and 0.25 to the side, so that it overhangs.

The tool runs in a child process; the same steps are taken in this process with the writer called by hand, where the step's kappa, dHat, the lagged friction
set and the positions the step started from are at hand.  Checked: the .vtu reads back; its cell and point stress are what `Context.elastic_stress` gives on
the `status<N>` of the same step; the contact-force field is, entry by entry, minus the barrier gradient of that state's constraint set at the step's kappa,
the set is not empty, the force pushes the upper cube up and the lower one down by the same amount; the friction field is not zero, equals minus the lagged
friction gradient, takes energy out of the step's motion, sums to zero and respects Coulomb's bound mu sum lambda; and a run with the writer takes the same
steps as a run without it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss, vtu_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 6
MU = 0.1
TEXT = f"shapes input 2\ncube.msh 0 0.504 0  0 0 0  1 1 1\ncube.msh 0.25 1.507 0  0 0 0  1 1 1\n\nselfFric {MU}\n\nground 0.1 0\n"
EPS = 2.0 ** -52


def make_scene(gpu_lib, tmp_path, restart=None):
    cfg = ss.SceneConfig.parse(TEXT, str(tmp_path))
    if restart:
        cfg.restart = restart
    return cfg, ss.assemble(cfg, gpu_lib.lib.read_tet_mesh)


def run_steps(gpu_lib, tmp_path, folder):
    """STEPS steps in this process; folder: write the fields of every step there.  Returns what the checks need."""
    cfg, sc = make_scene(gpu_lib, tmp_path)
    c = ss.apply(sc, gpu_lib.Context(0))
    try:
        w = ss.FieldsWriter(folder, sc, True, MU) if folder else None
        its = []
        for step in range(STEPS):
            sc.before_step(c, step * cfg.dt)
            x_prev = np.asarray(c.get_positions()).copy()
            its.append(c.solve_timestep(1000))
            assert its[-1] < 1000
            if w:
                # what the writer is to reproduce, asked BEFORE it runs: the step's parameters and the lagged friction set
                st, fs = c.state(), c.friction_state()
                path, n_invalid = w.write(c, step + 1, x_prev)
                assert n_invalid == 0 and os.path.basename(path) == f"fields{step + 1}.vtu"
        out = dict(its=its, x=np.asarray(c.get_positions()).copy(), v=c.kinematics()["velocity"].copy())
        if w:
            nV = sc.V.shape[0]
            g_fric = c.friction_gradient_add(x_prev, fs["fricDHat"], MU).reshape(nV, 3)  # (on the lagged set, before the constraint set is touched)
            sets = c.contact_build(st["dHat"])  # the constraint set of the written positions
            out.update(x_prev=x_prev, dHat=st["dHat"], kappa=st["kappa"], fs=fs, n_active=len(sets["active"]) + len(sets["para"]),
                       g_contact=c.contact_gradient_add(st["dHat"], st["kappa"], projectDBC=False).reshape(nV, 3),
                       g_half=c.contact_gradient_add(st["dHat"], 0.5 * st["kappa"], projectDBC=False).reshape(nV, 3),
                       g_fric=g_fric, node_ranges=list(sc.node_ranges))
        return out
    finally:
        c.close()


def test_fields_of_two_cubes_in_contact(gpu_lib, tmp_path):
    V, F = scene.make_box(2, 2, 2, size=(1.0, 1.0, 1.0), origin=(-0.5, -0.5, -0.5))
    gpu_lib.lib.save_tet_mesh(tmp_path / "cube.msh", V, F)
    (tmp_path / "scene.txt").write_text(TEXT)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_scene.py"), str(tmp_path / "scene.txt"), "--root", str(tmp_path), "--steps", str(STEPS),
           "--status-every", "3", "--out", str(tmp_path), "--fields", str(tmp_path / "fields"), "--fields-every", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "fields")) == ["fields3.vtu", "fields6.vtu"]  # every third step
    R = vtu_io.read_vtu(tmp_path / "fields" / f"fields{STEPS}.vtu")
    cfg, sc = make_scene(gpu_lib, tmp_path, restart=str(tmp_path / f"status{STEPS}"))
    nV, nT = sc.V.shape[0], sc.T.shape[0]
    assert R["points"].shape == (nV, 3) and np.array_equal(R["tets"], sc.T)
    assert list(R["cell_data"]) == ["stress", "von_mises", "J"]
    assert list(R["point_data"]) == ["stress", "von_mises", "velocity", "contact_force", "friction_force"]
    assert R["cell_data"]["stress"].shape == (nT, 6) and R["point_data"]["stress"].shape == (nV, 6) and R["point_data"]["contact_force"].shape == (nV, 3)
    # the stress of the same state from the checkpoint of the same step
    c = ss.apply(sc, gpu_lib.Context(0))  # (loads the checkpoint before precompute)
    try:
        assert np.asarray(c.get_positions()).tobytes() == np.asfortranarray(R["points"]).tobytes()  # 20 digits in the checkpoint, repr in the .vtu
        elem, node, n_invalid = c.elastic_stress()
        assert n_invalid == 0
        assert np.ascontiguousarray(elem[:, :6]).tobytes() == R["cell_data"]["stress"].tobytes()
        assert elem[:, 6].tobytes() == R["cell_data"]["von_mises"].tobytes() and elem[:, 7].tobytes() == R["cell_data"]["J"].tobytes()
        assert np.ascontiguousarray(node[:, :6]).tobytes() == R["point_data"]["stress"].tobytes()
        assert c.kinematics()["velocity"].tobytes() == R["point_data"]["velocity"].tobytes()
        assert R["cell_data"]["von_mises"].max() > 0.0  # the cubes are loaded by now
    finally:
        c.close()

    # the same steps in this process, the writer called by hand after each
    A = run_steps(gpu_lib, tmp_path, str(tmp_path / "fields_inproc"))
    Q = vtu_io.read_vtu(tmp_path / "fields_inproc" / f"fields{STEPS}.vtu")
    for k in ("stress", "von_mises", "velocity", "contact_force", "friction_force"):  # the tool writes what the writer writes: same steps, same bits
        assert Q["point_data"][k].tobytes() == R["point_data"][k].tobytes(), k
    assert Q["points"].tobytes() == R["points"].tobytes() and Q["cell_data"]["stress"].tobytes() == R["cell_data"]["stress"].tobytes()

    # contact forces: minus the barrier gradient of a non-empty set, at the step's kappa
    f, g = R["point_data"]["contact_force"], A["g_contact"]
    assert A["n_active"] > 0 and A["kappa"] > 0.0 and A["dHat"] > 0.0 and np.any(g)
    top = np.abs(g).max()
    print(f"step {STEPS}: {A['n_active']} constraints, kappa {A['kappa']:.4g}, dHat {A['dHat']:.4g}, max |barrier gradient| {top:.4g}")
    assert np.abs(f + g).max() <= 64.0 * EPS * top  # the same kernel on the same state: a fixed summation order, at most a last bit from the copy's sign
    assert np.abs(A["g_half"] - 0.5 * g).max() <= 64.0 * EPS * top  # linear in kappa: another kappa would not have passed the line above
    n0, n1, n2 = A["node_ranges"][:3]
    up, down = f[n1:n2].sum(0), f[n0:n1].sum(0)  # on the upper cube, on the lower cube
    assert up[1] > 0.0 and down[1] < 0.0  # the barrier pushes the bodies apart
    assert np.all(np.abs(up + down) <= 4.0 * nV * EPS * np.abs(f).sum(0))  # and is internal: action = reaction

    # friction forces: not zero, minus the lagged friction gradient of the step from x_prev to x
    ff, gf, fs = R["point_data"]["friction_force"], A["g_fric"], A["fs"]
    assert fs["n_lagged"] > 0 and fs["fricDHat"] > 0.0 and np.any(ff)
    ftop = np.abs(gf).max()
    print(f"step {STEPS}: {fs['n_lagged']} lagged pairs, eps_v^2 h^2 {fs['fricDHat']:.4g}, sum lambda {fs['lam'].sum():.4g}, max |friction gradient| {ftop:.4g}")
    assert np.abs(ff + gf).max() <= 64.0 * EPS * ftop
    u = A["x"] - A["x_prev"]
    assert float((ff * u).sum()) < 0.0  # dissipative: with x and x_prev exchanged, or the sign wrong, this is positive
    assert np.all(np.abs(ff.sum(0)) <= 4.0 * nV * EPS * np.abs(ff).sum(0) + 1e-300)  # internal
    # Coulomb: a pair's friction force is at most mu lambda on each of its two sides, spread over that side's nodes with weights that sum to one
    assert np.linalg.norm(ff, axis=1).sum() <= 2.0 * MU * fs["lam"].sum() * (1.0 + 1e-9)

    # the writer does not steer the run: without it the same Newton counts, positions and velocities
    B = run_steps(gpu_lib, tmp_path, None)
    assert A["its"] == B["its"] and A["x"].tobytes() == B["x"].tobytes() and A["v"].tobytes() == B["v"].tobytes()
