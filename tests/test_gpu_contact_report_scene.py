"""`ipcgpu_contact_report` on a real scene -- the two cubes above a ground plane of test_gpu_fields_tool.py, self-contact and friction on -- against the
library's own gradients, distances and counts on the sets the stepper holds, and the proof that asking for the report does not change the run."""
import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

pytestmark = pytest.mark.gpu

STEPS = 4
MU = 0.1
TEXT = f"shapes input 2\ncube.msh 0 0.504 0  0 0 0  1 1 1\ncube.msh 0.25 1.507 0  0 0 0  1 1 1\n\nselfFric {MU}\n\nground 0.1 0\n"
EPS = 2.0 ** -52


def run(gpu_lib, tmp_path, with_report, one_component=False):
    cfg = ss.SceneConfig.parse(TEXT, str(tmp_path))
    sc = ss.assemble(cfg, gpu_lib.lib.read_tet_mesh)
    c = ss.apply(sc, gpu_lib.Context(0))
    if one_component:  # the default table: the whole mesh
        c.set_components([sc.V.shape[0]], [sc.T.shape[0]])
    reports, x_prev = [], None
    for step in range(STEPS):
        sc.before_step(c, step * cfg.dt)
        x_prev = np.asarray(c.get_positions()).copy()
        assert c.solve_timestep(1000) < 1000
        if with_report:
            reports.append(c.contact_report(x_prev=x_prev, coef=MU))
    return c, sc, x_prev, reports


def plane_vertices_below(c, sc, cfg_text_root, dHat):
    """surface vertices that are not Dirichlet nodes with dist^2 < dHat to the scene's one half-space at the positions held: the set the stepper's last
    build at these positions holds (HipHalfSpace::build), counted on the host"""
    cfg = ss.SceneConfig.parse(TEXT, cfg_text_root)
    (origin, normal, _mu), = cfg.half_spaces
    x = np.asarray(c.get_positions())
    svi = np.asarray(c.get_surface()[0])
    dist = (x[svi] - origin) @ (normal / np.linalg.norm(normal))
    return svi[dist * dist < dHat]


def test_report_agrees_with_the_gradients_and_does_not_steer_the_run(gpu_lib, tmp_path):
    V, F = scene.make_box(2, 2, 2, size=(1.0, 1.0, 1.0), origin=(-0.5, -0.5, -0.5))
    gpu_lib.lib.save_tet_mesh(tmp_path / "cube.msh", V, F)
    cB, _, _, _ = run(gpu_lib, tmp_path, False)
    xB, vB = np.asarray(cB.get_positions()).copy(), cB.kinematics()["velocity"].copy()
    cB.close()
    c, sc, x_prev, reports = run(gpu_lib, tmp_path, True)
    try:
        assert np.asarray(c.get_positions()).tobytes() == xB.tobytes() and c.kinematics()["velocity"].tobytes() == vB.tobytes()
        rep = reports[-1]
        assert c.contact_report(x_prev=x_prev, coef=MU).tobytes() == rep.tobytes()  # two calls, the same bits
        st, fs = c.state(), c.friction_state()
        dHat, kappa = st["dHat"], st["kappa"]
        print("rows:", [(int(r["a"]), int(r["b"]), int(r["nPP"]), int(r["nPE"]), int(r["nPT"]), int(r["nEE"]), int(r["nMollified"]), float(r["minD2"])) for r in rep])
        pairs = [(int(r["a"]), int(r["b"])) for r in rep]
        assert (0, 1) in pairs and (0, -1) in pairs  # the cubes touch each other, the lower one the ground
        cross = rep[pairs.index((0, 1))]
        assert cross["nPT"] > 0 and cross["nEE"] > 0 and cross["nMollified"] > 0
        assert cross["FA"][1] < 0.0 < cross["FB"][1]  # the barrier pushes the lower cube down and the upper one up
        nV = sc.V.shape[0]
        ends = list(sc.node_ranges)
        x = np.asarray(c.get_positions())
        held = c.contact_held()
        n_hs = c.contact_state()["nHalfSpace"]
        # counts and minimum distance against contact_evaluate on the held tuples
        dA, dP = c.contact_evaluate(held["active"]), c.contact_evaluate(held["para"])
        n_rows = sum(int(r[k]) for r in rep if r["b"] >= 0 for k in ("nPP", "nPE", "nPT", "nEE", "nMollified"))
        assert n_rows == int((dA < dHat).sum() + (dP < dHat).sum()) and n_rows > 0
        dmin = min(float(r["minD2"]) for r in rep if r["b"] >= 0)
        assert abs(dmin - min(dA.min(), dP.min())) <= 1e-10 * dmin
        below = plane_vertices_below(c, sc, str(tmp_path), dHat)  # (the scene has no Dirichlet node)
        assert len(below) > 0 and n_hs >= len(below)
        for comp in range(2):  # exactly the held plane vertices below dHat, per component
            want = int(((below >= ends[comp]) & (below < ends[comp + 1])).sum())
            got = sum(int(r["nPP"]) for r in rep if r["b"] < 0 and r["a"] == comp)
            assert got == want, (comp, got, want)
        # forces per component against minus the gradients (after the report: these calls use the stepper's buffers)
        g = c.contact_gradient_add(dHat, kappa, projectDBC=False).reshape(nV, 3)
        gh = c.halfspace_gradient_add(0, dHat, kappa).reshape(nV, 3)
        gf = c.friction_gradient_add(x_prev, fs["fricDHat"], MU).reshape(nV, 3)
        for comp in range(2):
            n0, n1 = ends[comp], ends[comp + 1]
            F = sum(r["FA"] for r in rep if r["a"] == comp) + sum(r["FB"] for r in rep if r["b"] == comp)
            T = sum(r["TA"] for r in rep if r["a"] == comp) + sum(r["TB"] for r in rep if r["b"] == comp)
            R = sum(r["RA"] for r in rep if r["a"] == comp) + sum(r["RB"] for r in rep if r["b"] == comp)
            tot = g[n0:n1] + gh[n0:n1]
            bound = 4.0 * nV * EPS * (np.abs(g).sum(0) + np.abs(gh).sum(0))
            assert np.all(np.abs(F + tot.sum(0)) <= bound), (comp, F, tot.sum(0), bound)
            tq = np.cross(x[n0:n1], tot)
            tb = 4.0 * nV * EPS * (np.abs(np.cross(x, g)).sum(0) + np.abs(np.cross(x, gh)).sum(0) + np.abs(x).max() * (np.abs(g).sum() + np.abs(gh).sum()))
            assert np.all(np.abs(T + tq.sum(0)) <= tb), (comp, T, tq.sum(0), tb)
            fb = 4.0 * nV * EPS * np.abs(gf).sum(0)
            assert np.all(np.abs(R + gf[n0:n1].sum(0)) <= fb + 1e-300), (comp, R, gf[n0:n1].sum(0))
        # self rows: with the default single component the (0, 0) row holds every tuple of the two lists; an internal force system has no resultant and
        # no moment (translation and rotation invariance of the distances)
        c1, _, xp1, rep1 = run(gpu_lib, tmp_path, True, one_component=True)
        try:
            assert np.asarray(c1.get_positions()).tobytes() == xB.tobytes()
            one = rep1[-1]
            assert [(int(r["a"]), int(r["b"])) for r in one] == [(0, 0), (0, -1)]
            self_rows = 0
            for r in list(rep) + list(one):
                if r["a"] == r["b"]:
                    self_rows += 1
                    assert np.all(np.abs(r["FA"] + r["FB"]) <= 4.0 * nV * EPS * np.abs(g).sum(0)), (r["FA"], r["FB"])
                    tb = 4.0 * nV * EPS * (np.abs(np.cross(x, g)).sum(0) + np.abs(x).max() * np.abs(g).sum())
                    assert np.all(np.abs(r["TA"] + r["TB"]) <= tb), (r["TA"], r["TB"], tb)
                    assert np.any(r["FA"] != 0.0) and np.any(r["TA"] != 0.0)
            assert self_rows >= 1
            s0 = one[0]
            assert sum(int(s0[k]) for k in ("nPP", "nPE", "nPT", "nEE", "nMollified")) == n_rows and int(one[1]["nPP"]) == len(below)
            assert float(s0["minD2"]) == dmin
        finally:
            c1.close()
        assert fs["n_lagged"] > 0 and np.any(cross["RA"] != 0.0)
        W = float(sum(r["W"] for r in rep))
        assert W <= 4.0 * nV * EPS * float(np.abs(gf * (x - x_prev)).sum())
        assert abs(W + float((gf * (x - x_prev)).sum())) <= 4.0 * nV * EPS * float(np.abs(gf * (x - x_prev)).sum())
    finally:
        c.close()
