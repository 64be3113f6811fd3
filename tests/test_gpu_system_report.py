"""The system report on the device (`ipcgpu_opt_set_components` / `ipcgpu_opt_system_report`, `Context.system_report()`; the reference's
`Optimizer::computeSystemEnergy`, Optimizer.cpp:3746-3778): energy, linear momentum and angular momentum about the origin per mesh component.

The yardstick is the NumPy restatement below, summed with `math.fsum`, on inputs the library already exposes: `get_positions()`, the positions the test
saved before the step, the lumped masses of `features()` and `elastic_energy_per_elem()` (pinned on the reference at 1e-12 by test_gpu_vs_reference.py).

Tolerance (derived, not tuned): any summation order of n terms t_i differs from the exact sum by at most (n - 1) eps sum |t_i|, the products inside a term
add a few eps each: |gpu - fsum| <= 4 n 2^-52 sum |t_i| per output, n and sum |t_i| from the restatement's own terms.  The terms are the summands without
cancellation inside them: per element vol psi; per node the kinetic part m |x - xprev|^2 / (2 dt^2) and the potential part -m g . x (two terms: their
difference cancels); per node and axis m (x - xprev) / dt; per node and axis the two products of the cross product.

Gravity: `opt_init(dt, gravity=True)` is (0, -9.80665, 0), the reference's value (Optimizer.cpp:112-115) and the only one the library has; the free-fall
test states its expectation with that number."""
import math

import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
G = np.array([0.0, -9.80665, 0.0])
DT = 0.01
YM, PR, RHO = 1e5, 0.4, 1000.0


def four_components():
    """Four components back to back, far apart: a 9 x 9 x 9-node cube (729 nodes: three 256-slices, the last one partial) WITHOUT its last tetrahedron
    (the Kuhn split gives 3072 = 12 x 256 of them; 3071 is no multiple of 64, so the element slices of every later component start unaligned); a
    2 x 2 x 2-node cube; one triangle without tetrahedra, held by Dirichlet; a 5 x 4 x 3-node cube that gets another density."""
    V1, F1 = scene.make_box(8, 8, 8, size=(1.0, 1.0, 1.0), origin=(-0.5, 0.25, -0.5))
    F1 = F1[:-1]
    assert len(np.unique(F1)) == 729 and F1.shape[0] == 3071 and F1.shape[0] % 64
    V2, F2 = scene.make_box(1, 1, 1, size=(0.3, 0.3, 0.3), origin=(3.0, 0.1, 0.0))
    V3 = np.array([[6.0, -1.0, 0.0], [7.0, -1.0, 0.25], [6.0, -1.0, 1.0]])
    V4, F4 = scene.make_box(4, 3, 2, size=(0.8, 0.6, 0.4), origin=(-4.0, 1.0, 2.0))
    Vs, Fs = [V1, V2, V3, V4], [F1, F2, np.zeros((0, 4), np.int32), F4]
    node_end = np.cumsum([v.shape[0] for v in Vs])
    tet_end = np.cumsum([f.shape[0] for f in Fs])
    off = np.concatenate([[0], node_end[:-1]])
    V = np.vstack(Vs)
    F = np.vstack([f + o for f, o in zip(Fs, off)]).astype(np.int32)
    assert node_end.tolist() == [729, 737, 740, 800] and tet_end.tolist() == [3071, 3077, 3077, 3221]
    return V, F, node_end, tet_end


def make_context(gpu_lib, integration="BE", energy="NH", components=True):
    V, F, node_end, tet_end = four_components()
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=YM, PR=PR, density=RHO)
    tri = np.arange(node_end[1], node_end[2])
    c.set_codim_nodes(tri, [0.3, 0.2, 0.1])
    c.set_energy_type(energy)
    c.set_component_material((node_end[2], node_end[3]), (tet_end[2], tet_end[3]), 2500.0, 2e5, 0.3)
    if components:
        c.set_components(node_end, tet_end)
    # the cubes start stretched about their centres: the elastic part is not zero and the bodies oscillate while they fall
    X = V.copy()
    for v0, v1, s in ((0, node_end[0], 1.05), (node_end[2], node_end[3], 0.96)):
        ctr = X[v0:v1].mean(0)
        X[v0:v1] = ctr + s * (X[v0:v1] - ctr) * np.array([1.0, 1.0 / s, 1.0])
    c.set_positions(X)
    c.opt_init(DT, True)
    if integration == "NM":
        c.set_time_integration("NM")
    c.set_dbc(tri, 1)
    c.set_rel_tol(1e-6)
    c.precompute()
    return c, node_end, tet_end


def restate(c, xprev, node_end, tet_end, dt=DT, g=G):
    """per component and output: (fsum of the terms, 4 n eps sum |t_i|)"""
    x = np.asarray(c.get_positions())
    m = c.features()["mass"]
    epe = c.elastic_energy_per_elem()
    out = []
    for k in range(len(node_end)):
        v0, t0 = (node_end[k - 1], tet_end[k - 1]) if k else (0, 0)
        v1, t1 = node_end[k], tet_end[k]
        xs, d, ms = x[v0:v1], x[v0:v1] - xprev[v0:v1], m[v0:v1]
        p = (ms / dt)[:, None] * d
        terms = {"E": np.concatenate([epe[t0:t1], ms * ((d * d).sum(1) / (dt * dt) / 2.0), -ms * (xs @ g)])}
        for i, a in enumerate("xyz"):
            j, l = (i + 1) % 3, (i + 2) % 3
            terms["M" + a] = p[:, i]
            terms["L" + a] = np.concatenate([xs[:, j] * p[:, l], -xs[:, l] * p[:, j]])
        out.append({key: (math.fsum(t), 4.0 * len(t) * EPS * math.fsum(np.abs(t))) for key, t in terms.items()})
    return out


def compare(report, want, what):
    E, M, L = report
    assert E.shape == (len(want),) and M.shape == L.shape == (len(want), 3)
    for k, w in enumerate(want):
        got = {"E": E[k], **{"M" + a: M[k, i] for i, a in enumerate("xyz")}, **{"L" + a: L[k, i] for i, a in enumerate("xyz")}}
        for key, (ref, bound) in w.items():
            err = abs(got[key] - ref)
            print(f"{what} component {k} {key}: gpu {got[key]!r} fsum {ref!r} |diff| {err:.3e} bound {bound:.3e}")
            assert err <= bound, (what, k, key, got[key], ref, err, bound)


def run_steps(gpu_lib, integration, energy, steps):
    c, node_end, tet_end = make_context(gpu_lib, integration, energy)
    try:
        x0 = np.asarray(c.get_positions()).copy()
        E, M, L = c.system_report()
        assert np.all(M == 0.0) and np.all(L == 0.0)  # after precompute xprev == x: the momenta are exactly zero ...
        want = restate(c, x0, node_end, tet_end)
        compare((E, M, L), want, f"{integration} {energy} precompute")
        m = c.features()["mass"]
        for k in range(4):  # ... and so is the kinetic part: what is left is the elastic and the potential part alone
            v0, t0 = (node_end[k - 1], tet_end[k - 1]) if k else (0, 0)
            rest = np.concatenate([c.elastic_energy_per_elem()[t0:tet_end[k]], -m[v0:node_end[k]] * (x0[v0:node_end[k]] @ G)])
            assert abs(E[k] - math.fsum(rest)) <= 4.0 * len(rest) * EPS * math.fsum(np.abs(rest))
        assert E[0] != 0.0 and E[2] == pytest.approx(9.80665 * 0.6 * -1.0, rel=1e-12)  # the held triangle: potential energy only
        for step in range(steps):
            xprev = np.asarray(c.get_positions()).copy()
            assert c.solve_timestep(100) < 100
            rep = c.system_report()
            compare(rep, restate(c, xprev, node_end, tet_end), f"{integration} {energy} step {step + 1}")
            assert np.all(rep[1][2] == 0.0) and np.all(rep[2][2] == 0.0)  # the Dirichlet triangle does not move
            assert rep[1][0, 1] < 0.0 and rep[1][3, 1] < 0.0  # the cubes fall
    finally:
        c.close()


def test_segment_boundaries_backward_euler_three_steps(gpu_lib):
    run_steps(gpu_lib, "BE", "NH", 3)


def test_segment_boundaries_newmark(gpu_lib):
    run_steps(gpu_lib, "NM", "NH", 1)


def test_segment_boundaries_fixed_corotated(gpu_lib):
    run_steps(gpu_lib, "BE", "FCR", 1)


def test_bit_reproducible(gpu_lib):
    reps = []
    for _ in range(2):
        c, _ne, _te = make_context(gpu_lib)
        try:
            assert c.solve_timestep(100) < 100
            a, b = c.system_report(), c.system_report()
            assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))  # the report changes no state and sums in a fixed order
            reps.append(b"".join(p.tobytes() for p in a))
        finally:
            c.close()
    assert reps[0] == reps[1]  # a second context set up the same way


def test_free_fall_momentum_backward_euler(gpu_lib):
    """A free body under gravity: backward Euler gives x_k - x_{k-1} = k dt^2 g at every node exactly, so sysM_y = g_y M k dt (g_y = -9.80665, see the
    module docstring) and sysM_x = sysM_z = 0, each to the restatement's bound for the y terms (27 nodes, centred on the origin so that the rounding of a
    position is small beside the displacement of a step)."""
    dt = 0.04
    V, F = scene.make_box(2, 2, 2, size=(1.0, 1.0, 1.0), origin=(-0.5, -0.5, -0.5))
    c = gpu_lib.Context(0)
    try:
        c.set_mesh(V, F, YM=YM, PR=PR, density=RHO)
        c.opt_init(dt, True)
        c.set_rel_tol(1e-6)
        c.precompute()
        m = c.features()["mass"]
        Mtot = math.fsum(m)
        assert Mtot == pytest.approx(RHO, rel=1e-12)
        for k in (1, 2, 3):
            xprev = np.asarray(c.get_positions()).copy()
            assert c.solve_timestep(100) < 100
            E, M, L = c.system_report()
            t = m * (np.asarray(c.get_positions())[:, 1] - xprev[:, 1]) / dt
            bound = 4.0 * len(t) * EPS * math.fsum(np.abs(t))
            want = G[1] * Mtot * k * dt
            print(f"step {k}: sysM {M[0]!r} expected y {want!r} |diff| {abs(M[0, 1] - want):.3e} bound {bound:.3e}")
            assert abs(M[0, 1] - want) <= bound
            assert abs(M[0, 0]) <= bound and abs(M[0, 2]) <= bound
    finally:
        c.close()


def test_default_is_one_component_the_whole_mesh(gpu_lib):
    c4, node_end, tet_end = make_context(gpu_lib)
    c1, _, _ = make_context(gpu_lib, components=False)
    try:
        for c in (c4, c1):
            xprev = np.asarray(c.get_positions()).copy()
            assert c.solve_timestep(100) < 100
        four, one = c4.system_report(), c1.system_report()
        assert one[0].shape == (1,) and one[1].shape == one[2].shape == (1, 3)
        whole = restate(c1, xprev, node_end[-1:], tet_end[-1:])
        compare(one, whole, "one component")
        parts = restate(c4, xprev, node_end, tet_end)
        flat1 = np.concatenate([a.ravel() for a in one])
        flat4 = np.concatenate([a.sum(0).ravel() for a in four])
        for i, key in enumerate(["E", "Mx", "My", "Mz", "Lx", "Ly", "Lz"]):
            # each side is within its bound of the exact sum of the same terms; adding the four results rounds three more times
            bound = whole[0][key][1] + sum(p[key][1] for p in parts) + 3 * EPS * sum(abs(p[key][0]) for p in parts)
            assert abs(flat1[i] - flat4[i]) <= bound, (key, flat1[i], flat4[i], bound)
    finally:
        c4.close()
        c1.close()


def test_validation_and_error_codes(gpu_lib):
    V, F, node_end, tet_end = four_components()
    c = gpu_lib.Context(0)
    try:
        c.set_mesh(V, F, YM=YM, PR=PR, density=RHO)
        with pytest.raises(gpu_lib.lib.IpcGpuError, match="ipcgpu error -3"):  # before opt_init: the state error
            c.system_report()
        for bad_nodes, bad_tets in (([729, 700, 740, 800], tet_end), (node_end, [3071, 3077, 3070, 3221]),  # decreasing
                                    ([729, 737, 740, 799], tet_end), ([729, 737, 740, 801], tet_end), (node_end, [3071, 3077, 3077, 3220]),  # last != nV / nT
                                    ([-1, 737, 740, 800], tet_end)):
            with pytest.raises(gpu_lib.lib.IpcGpuError, match="ipcgpu error -1"):
                c.set_components(bad_nodes, bad_tets)
        with pytest.raises(gpu_lib.lib.IpcGpuError, match="ipcgpu error -1"):
            c._chk(c._L.ipcgpu_opt_set_components(c.h, 0, None, None))  # nComp >= 1
        c.set_components([0, 729, 729, 800, 800], [0, 3071, 3071, 3221, 3221])  # empty components are legal
        c.opt_init(DT, True)
        E, M, L = c.system_report()  # legal right after opt_init; the rejected tables above left nothing behind
        assert E.shape == (5,) and E[0] == 0.0 and E[2] == 0.0 and E[4] == 0.0 and E[1] != 0.0 and np.all(M == 0.0) and np.all(L == 0.0)
    finally:
        c.close()
    c = gpu_lib.Context(0)
    try:
        c.set_shard(0, 2)
        c.set_mesh(V, F, YM=YM, PR=PR, density=RHO)
        c.opt_init(DT, True)
        with pytest.raises(gpu_lib.lib.IpcGpuError, match="ipcgpu error -4"):  # multi-rank reports are not implemented
            c.system_report()
    finally:
        c.close()


def test_scene_layer_two_cubes_fall(gpu_lib, tmp_path):
    """tutorialExamples/2cubesFall.txt (two unit cubes at heights 3 and 1, ground and self-contact with friction) with a cube of the scene helpers in
    place of the reference's mesh file, through scene_script.apply for two steps with the report written as `tools/run_scene.py --report` writes it."""
    V, F = scene.make_box(2, 2, 2, size=(1.0, 1.0, 1.0), origin=(-0.5, -0.5, -0.5))
    gpu_lib.lib.save_tet_mesh(tmp_path / "cube.msh", V, F)
    text = "shapes input 2\ncube.msh 0 3 0  0 0 0  1 1 1\ncube.msh 0 1 0  0 0 0  1 1 1\n\nselfFric 0.1\n\nground 0.1 0\n"
    cfg = ss.SceneConfig.parse(text, str(tmp_path))
    sc = ss.assemble(cfg, gpu_lib.lib.read_tet_mesh)
    c = ss.apply(sc, gpu_lib.Context(0))
    try:
        w = ss.ReportWriter(str(tmp_path / "report"))
        w.write(c)
        direct = [c.system_report()]
        for step in range(2):
            sc.before_step(c, step * cfg.dt)
            assert c.solve_timestep(1000) < 1000
            w.write(c)
            direct.append(c.system_report())
        for i, name in enumerate(("sysE.txt", "sysM.txt", "sysL.txt")):
            a = np.loadtxt(tmp_path / "report" / name, ndmin=2)
            assert a.shape == (3, 2 if i == 0 else 6)  # three lines, two components
            assert np.array_equal(a, np.array([d[i].ravel() for d in direct]))
        E, M, L = direct[-1]
        assert np.all(M[:, 1] < 0.0) and E[0] > E[1] > 0.0  # both fall; the upper cube has the larger potential energy
    finally:
        c.close()
