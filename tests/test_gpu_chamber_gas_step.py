"""Gas chambers (ipcgpu_chamber_set_gas) in the stepper and the building blocks: the rank-k correction against a dense solve, a block that swells to the
root of its equilibrium equation, real air on a cloth cube, the momenta of a free gas cube, pumping between steps, a cushion on a plane, the error paths,
and that set_gas(zeros) leaves a constant-only context alone.  Small meshes; the multifrontal solver throughout, rocSOLVER where cheap.

The model is stated in ipc_amd/csrc/chamber_kernels.h; helpers and the line-search floor are those of test_gpu_chamber_step.py."""
import numpy as np
import pytest

import chamber_mp as cm
from codim_common import five_tet_cube, step_context
from test_gpu_attach_step import iterate_bound
from test_gpu_chamber_step import CLOTH, RHO, SIZE, cloth_context, cloth_cube

pytestmark = pytest.mark.gpu

AMBIENT = 1e5


def two_cubes():
    """two cloth cubes that share the face x = SIZE: 12 nodes; the two shared triangles belong to both chambers, with opposite orientation.  The cloth is the
    outer skin (20 triangles): a shell takes no edge with three triangles, so the wall between the chambers is a chamber face without cloth"""
    V = np.vstack([cm.CUBE_X, cm.CUBE_X[[1, 2, 5, 6]] + [1.0, 0.0, 0.0]]) * SIZE + 0.1
    local = np.array([1, 8, 9, 2, 5, 10, 11, 6])  # B's corner i is this node: its x = 0 face is A's x = 1 face
    triA, triB = cm.CUBE_TRI.copy(), local[cm.CUBE_TRI].astype(np.int32)
    keyA = {tuple(sorted(t)) for t in triA.tolist()}
    shared = [t for t in triB.tolist() if tuple(sorted(t)) in keyA]
    assert len(shared) == 2
    keyB = {tuple(sorted(t)) for t in triB.tolist()}
    shell = np.array([t for t in triA.tolist() if tuple(sorted(t)) not in keyB] + [t for t in triB.tolist() if tuple(sorted(t)) not in keyA], dtype=np.int32)
    assert len(shell) == 20
    return V, shell, [triA, triB]


@pytest.mark.parametrize("k,solver", [(1, 0), (1, 1), (2, 0)])
def test_woodbury_correction_against_a_dense_solve(gpu_lib, k, solver):
    """(A + coef sum_c beta_c u_c u_c^T) x = rhs through ipcgpu_chamber_gas_solve -- the stepper's own routine -- against the same matrix built densely in
    NumPy from get_a, chamber_gas_state and chamber_volume_gradient.  Relative residual <= 1e-10, the project's bound for the solver's residual (DESIGN.md
    section 2).  The answer of A alone differs by more than 1e3 times that residual: the correction is in effect.  One node is held, so u_c has projected entries."""
    dt, p = 0.01, 20.0
    if k == 1:
        V, tri = cloth_cube([0.1, 0.1, 0.1])
        shell, chambers = tri, [tri]
    else:
        V, shell, chambers = two_cubes()

    def body(c):
        c.set_shell(shell, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO)
        c.set_chambers(chambers, [p] * k)
    c = step_context(gpu_lib, V, body, solver, None, 1e5, RHO, dt, gravity=False, held=[0])
    c.chamber_set_gas(True, AMBIENT, 1.4)
    c.precompute()
    rng = np.random.default_rng(5)
    c.set_positions(V + 0.002 * (rng.random(V.shape) - 0.5) * (np.arange(len(V)) > 0)[:, None])
    coef = dt * dt
    c.assemble_newton(coef, True)
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    A = A + np.triu(A, 1).T
    assert c.factorize()
    vol, gauge, beta = c.chamber_gas_state()
    U = np.array([c.chamber_volume_gradient(i, True) for i in range(k)])
    assert np.all(beta > 0) and np.all(U[:, :3] == 0.0) and np.all(np.abs(U).max(axis=1) > 0)
    Mfull = A + coef * sum(b * np.outer(u, u) for b, u in zip(beta, U))
    rhs = rng.standard_normal(A.shape[0])
    x = c.chamber_gas_solve(coef, rhs)
    res = np.linalg.norm(Mfull @ x - rhs) / np.linalg.norm(rhs)
    plain = c.solve(rhs)
    apart = np.linalg.norm(x - plain) / np.linalg.norm(x)
    print(f"k {k} solver {solver}: relative residual {res:.3g} (bound 1e-10), cond {np.linalg.cond(Mfull):.3g}, A alone is {apart:.3g} away, "
          f"coef beta |u|^2 {[float(coef * b * u @ u) for b, u in zip(beta, U)]}, gauge {gauge}")
    assert res <= 1e-10
    assert apart > 1e3 * max(res, 1e-16)
    assert np.linalg.norm(x - np.linalg.solve(Mfull, rhs)) <= 1e-10 * np.linalg.cond(Mfull) * np.linalg.norm(x)


@pytest.mark.parametrize("gamma", [1.0, 1.4])
def test_block_with_a_gas_chamber_swells_uniformly(gpu_lib, gamma):
    """The five-tet block of test_block_under_outside_pressure_shrinks_uniformly with its 12 faces as a GAS chamber: p_c at 1 % of the bulk modulus,
    ambient = 10 p_c.  A uniform scaling s is an exact discrete equilibrium, for the reasons given there; per rest volume the static energy is
    psi(s I) + W(s^3 V0) / V0 with dW/dV = -gauge, so s is the root of 3 mu (s - 1/s) + 9 lam ln s / s - 3 s^2 gauge(s^3 V0) = 0, by bisection.  Edge
    ratios within 2 e / rest length of s (e = iterate_bound), as derived there.  chamber_gas_state's volume is within 3 bound 1.01 of s^3 V0 (as there),
    and its gauge within gamma P(V_lo) 3.03 bound of gauge(s^3 V0) by the mean value theorem (|dgauge/dV| V = gamma P, decreasing in V; V_lo the low end)."""
    YM, PR = 1e7, 0.4
    mu, lam = YM / (2 * (1 + PR)), YM * PR / ((1 + PR) * (1 - 2 * PR))
    pc = 0.01 * (lam + 2 * mu / 3)
    amb = 10 * pc
    gauge_of = lambda J: (amb + pc) * J ** (-gamma) - amb  # J = V / V0
    f = lambda s: 3 * mu * (s - 1 / s) + 9 * lam * np.log(s) / s - 3 * s * s * gauge_of(s ** 3)
    a, b = 1.0, 1.1
    assert f(a) < 0 < f(b)
    for _ in range(200):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if f(mid) < 0 else (a, mid)
    s = 0.5 * (a + b)
    V, T = five_tet_cube(SIZE, np.array([0.2, 0.1, 0.3]))
    relTol, dt, steps = 1e-7, 1.0, 4
    from ipc_amd import scene
    skin = scene.surface_tris(T)
    if cm.rest_volume(V, skin, cm.ref_point(V, skin)) < 0:
        skin = skin[:, ::-1]
    c = step_context(gpu_lib, V, lambda c: c.set_chambers([skin], [pc]), 0, T, YM, RHO, dt, gravity=False)
    c.chamber_set_gas([True], [amb], [gamma])
    c.set_rel_tol(relTol)
    c.precompute()
    for _ in range(steps):
        assert c.solve_timestep(200) < 200
    X = c.state()["V"]
    edges = np.array([(i, j) for i in range(8) for j in range(i + 1, 8)])
    rest = np.linalg.norm(V[edges[:, 0]] - V[edges[:, 1]], axis=1)
    ratio = np.linalg.norm(X[edges[:, 0]] - X[edges[:, 1]], axis=1) / rest
    bound = 2 * iterate_bound(relTol, V, dt, steps) / rest.min()
    vol, gauge, beta = c.chamber_gas_state()
    gBound = gamma * (gauge_of(s ** 3 * (1 - 3.03 * bound)) + amb) * 3.03 * bound
    print(f"gamma {gamma}: s {s:.9f}, edge ratios {ratio.min():.9f} .. {ratio.max():.9f}, worst |ratio - s| {np.abs(ratio - s).max():.3g} (bound {bound:.3g}); "
          f"gauge {gauge[0]:.9g} against {gauge_of(s ** 3):.9g} (bound {gBound:.3g}), p_c {pc:.6g}")
    assert s - 1 > 1e2 * bound  # the block really swelled
    assert np.all(np.abs(ratio - s) <= bound)
    assert abs(vol[0] / SIZE ** 3 - s ** 3) <= 3 * bound * 1.01
    assert abs(gauge[0] - gauge_of(s ** 3)) <= gBound and 0 < gauge[0] < pc


def volume_effect(c, e):
    """what a displacement of every node by at most e (per coordinate) can do to the volume, to first order: e |gradV|_1"""
    return e * np.abs(c.chamber_volume_gradient(0, False)).sum()


def test_real_air_on_cloth_holds_the_volume(gpu_lib):
    """The held cloth cube (E h = 100 N / m) with p_c = 20 over an ambient 1e5 (gamma = 1.4), dt = 10, 8 steps: beta gradV gradV^T is 1e4 times every other
    stiffness here.  Every step converges inside solve_timestep(50).  The final volume obeys V0 < V <= V0 (P0 / p_amb)^(1 / gamma) (+ three times the iterate
    bound's effect on the volume): a taut skin needs gauge > 0, and the upper bound is the volume of zero gauge -- both from the model.  The same scene as a
    constant chamber ends above that bound: the law is what holds the volume."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    # (relTol 1e-7: three times the iterate bound's effect on the volume is then 0.4 % of V0, a third of what a constant 20 Pa inflates this cube by)
    relTol, dt, steps, p, gamma = 1e-7, 10.0, 8, 20.0, 1.4
    V0 = SIZE ** 3
    top = V0 * ((AMBIENT + p) / AMBIENT) ** (1 / gamma)
    vols = {}
    for gas in (True, False):
        c = cloth_context(gpu_lib, V, tri, p, 0, dt, held=[0], relTol=relTol)
        if gas:
            c.chamber_set_gas(True, AMBIENT, gamma)
        its = [c.solve_timestep(50 if gas else 300) for _ in range(steps)]
        vols[gas] = c.chamber_gas_state()[0][0]
        eff = volume_effect(c, iterate_bound(relTol, V, dt, steps))
        print(f"gas {gas}: iterations {its}, V / V0 - 1 = {vols[gas] / V0 - 1:.6g} (zero-gauge volume at {top / V0 - 1:.6g}, iterate effect {eff / V0:.3g}), "
              f"gauge {c.chamber_gas_state()[1][0]:.6g}")
        if gas:
            assert all(i < 50 for i in its)
            assert V0 < vols[gas] <= top + 3 * eff
        else:
            assert vols[gas] > top + 3 * eff


def test_free_gas_cube_keeps_its_momenta(gpu_lib):
    """test_free_pressurised_cloth_cube_keeps_its_momenta with the gas law: W depends on the positions through V alone, V is invariant under translation
    and rotation, so the invariance and with it the bounds are the same: |P| <= 2 M e_k / dt, the defect of the angular balance <= 4 M e_k R / dt + 6 M e_k vmax."""
    V, tri = cloth_cube([0.3, 0.2, 0.1])
    relTol, dt, steps, p = 1e-6, 0.01, 10, 20.0
    c = cloth_context(gpu_lib, V, tri, p, 0, dt, relTol=relTol)
    c.chamber_set_gas(True, AMBIENT, 1.4)
    m = c.features()["mass"]
    V0 = c.chamber_gas_state()[0][0]
    prev, vmax, moved, Lprev, vprev, Vmax = V.copy(), 0.0, 0.0, np.zeros(3), np.zeros(V.shape), 0.0
    for k in range(1, steps + 1):
        assert c.solve_timestep(100) < 100
        X = c.state()["V"]
        v = (X - prev) / dt
        prev = X
        vmax = max(vmax, np.linalg.norm(v, axis=1).max())
        e = iterate_bound(relTol, V, dt, k)
        Pm = (m[:, None] * v).sum(axis=0)
        Lm = (m[:, None] * np.cross(X, v)).sum(axis=0)
        R = np.linalg.norm(X, axis=1).max()
        bP, bL = 2 * m.sum() * e / dt, 4 * m.sum() * e * R / dt + 6 * m.sum() * e * vmax
        moved = max(moved, np.abs(m[:4, None] * v[:4]).sum())
        torque = Lm - Lprev - dt * (m[:, None] * np.cross(v, vprev)).sum(axis=0)
        Lprev, vprev = Lm, v
        Vmax = max(Vmax, c.chamber_gas_state()[0][0])
        print(f"step {k}: |P| {np.linalg.norm(Pm):.3g} (bound {bP:.3g}), defect of the angular momentum balance {np.linalg.norm(torque):.3g} (bound {bL:.3g}), "
              f"four nodes' momentum {moved:.3g}, volume / rest - 1 {c.chamber_gas_state()[0][0] / V0 - 1:.3g}")
        assert np.linalg.norm(Pm) <= bP and np.linalg.norm(torque) <= bL
    # the gas holds the volume, so the nodes move far less than under a constant pressure and `moved` stays under the constant test's 1e2 bP; that the
    # zero momentum is a cancellation and not rest shows against the momentum itself: four nodes carry a million times the total
    assert moved > 1e6 * np.linalg.norm(Pm)
    assert V0 < Vmax <= V0 * ((AMBIENT + p) / AMBIENT) ** (1 / 1.4) * (1 + 1e-9)  # the gas expanded, and never past its zero-gauge volume (W rises beyond it)


def test_pumping_between_steps_raises_the_volume(gpu_lib):
    """chamber_set_pressure between steps on a gas chamber pumps gas in: the quasi-static volume (dt = 10, four steps per pressure) is strictly increasing in
    p_c, and a pressure that would make P0 <= 0 is refused and changes nothing."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    relTol, dt = 1e-6, 10.0
    c = cloth_context(gpu_lib, V, tri, 10.0, 0, dt, held=[0], relTol=relTol)
    c.chamber_set_gas(True, AMBIENT, 1.4)
    vols = []
    for p in (10.0, 20.0, 40.0):
        c.chamber_set_pressure(p)
        for _ in range(4):
            assert c.solve_timestep(50) < 50
        vols.append(c.chamber_gas_state()[0][0])
    eff = volume_effect(c, iterate_bound(relTol, V, dt, 12))
    print(f"volumes / V0 - 1: {[v / SIZE ** 3 - 1 for v in vols]}, iterate effect {eff / SIZE ** 3:.3g}")
    assert SIZE ** 3 < vols[0] < vols[1] < vols[2]
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*gas chamber 0"):
        c.chamber_set_pressure(-AMBIENT)
    assert c.chamber_get()["pressure"][0] == 40.0


def test_gas_cushion_comes_to_rest_on_a_plane(gpu_lib):
    """A gas cloth cube with p_c = 0 (filled at ambient pressure) falls 2 mm under gravity onto a half-space, with contact.  Steps converge, nothing
    intersects.  At rest V < V0 and so gauge > p_c = 0: with gauge <= 0 nothing would push the top face up against its weight or the sides out, the
    top would sag and the volume fall below V0, where the gauge is positive -- a contradiction; so the gas carries load.
    The statement is about the state of rest, not about the trajectory that led there, so the margin is not the trajectory's accumulated bound: the last
    iterate lies within delta = 2 tol of its step's minimiser (iterate_bound for k = 0), and what the body still moves per step, `moved`, measured here,
    bounds what the next steps change; to first order both change the volume by at most (delta + 2 moved) |gradV|_1.  The drop to expect is the top face's
    weight per area over the gas stiffness, rho h g / (gamma p_amb) V0 = 9.8 / 1.4e5 x 1e-3 = 7e-8 m^3, less what the walls carry.
    Line-search floor: W's two terms, each p_amb |V - V0| dt^2 = 2.5e-9, nearly cancel at rest and are evaluated to u relative each (ln(V0 / V) through log1p
    of the exact difference: chamber_kernels.hip); beside the gravity potential dt^2 m g y = 1.2e-5 that is nothing, and the floor is the one of a cloth
    cube under gravity, sqrt(2 u 1.2e-5 / m) = 6e-10 against the tolerance 3.4e-9.  (With ln(V0 / V) taken from the quotient the energy carried an
    absolute error u P0 V0 dt^2 = 4e-18, a floor of 3e-8: the sixth step then never reached the tolerance.)"""
    V, tri = cloth_cube([0.1, 0.002, 0.1])
    dt, relTol = 0.02, 1e-6

    def body(c):
        c.set_shell(tri, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO)
        c.set_chambers([tri], [0.0])
    c = step_context(gpu_lib, V, body, 0, None, 1e5, RHO, dt, gravity=True)
    c.chamber_set_gas(True, AMBIENT, 1.4)
    c.set_surface(tri)
    c.enable_self_collision(1e-3)
    c.add_half_space((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1e-3)
    c.set_rel_tol(relTol)
    c.precompute()
    its, prev = [], V.copy()
    for _ in range(25):
        prev = c.state()["V"]
        its.append(c.solve_timestep(300))
        print(f"step {len(its)}: {its[-1]} iterations, volume / V0 - 1 {c.chamber_gas_state()[0][0] / SIZE ** 3 - 1:.3g}, lowest node {c.state()['V'][:, 1].min():.3g}")
        assert its[-1] < 300 and not c.is_intersected()
    vol, gauge, _ = c.chamber_gas_state()
    X = c.state()["V"]
    delta, moved = iterate_bound(relTol, V, dt, 0), np.abs(X - prev).max()
    eff = volume_effect(c, delta + 2 * moved)
    print(f"iterations {its}, lowest node at {X[:, 1].min():.3g}, V / V0 - 1 {vol[0] / SIZE ** 3 - 1:.3g} (delta {delta:.3g}, last step moved {moved:.3g}, "
          f"their effect {eff / SIZE ** 3:.3g}), gauge {gauge[0]:.4g}")
    assert moved <= 10 * delta  # at rest: what a step still moves is of the size of the iterate tolerance
    assert 0.0 < X[:, 1].min() < 2e-3  # it fell and lies on the plane
    assert vol[0] < SIZE ** 3 - eff and gauge[0] > 0.0


def test_error_paths_and_refusals(gpu_lib):
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    E = gpu_lib.IpcGpuError
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=1e5, PR=0.4, density=RHO)
    import ctypes as C
    one = (C.c_int * 1)(1)
    d = (C.c_double * 1)(1.0)
    assert c._L.ipcgpu_chamber_set_gas(c.h, one, d, d, None) == -3  # IPCGPU_ERR_STATE without chambers
    c.set_shell(tri, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO)
    c.set_chambers([tri], [20.0])
    for kw, what in ((dict(ambient=np.nan), "not finite"), (dict(ambient=-1.0), "ambient pressure"), (dict(gamma=0.9), "gamma"), (dict(gamma=np.inf), "not finite"),
                     (dict(ambient=0.0, gamma=1.0, fill_volume=np.nan), "not finite")):
        with pytest.raises(E, match=f"ipcgpu error -1.*chamber 0.*{what}"):
            c.chamber_set_gas(True, **{**dict(ambient=AMBIENT, gamma=1.4), **kw})
    c.chamber_set_pressure(-30.0)
    with pytest.raises(E, match="ipcgpu error -1.*chamber 0.*<= 0"):
        c.chamber_set_gas(True, 30.0, 1.4)
    assert not c.chamber_gas_get()["isGas"].any()  # a refused call changes nothing
    c.chamber_set_pressure(20.0)
    c.chamber_set_gas(True, AMBIENT, 1.4, 2e-3)
    got = c.chamber_gas_get()
    assert got["isGas"].tolist() == [1] and got["ambient"][0] == AMBIENT and got["gamma"][0] == 1.4 and got["fillVolume"][0] == 2e-3
    c.chamber_set_gas(True, AMBIENT, 1.4, -1.0)
    assert c.chamber_gas_get()["fillVolume"][0] == c.chamber_get()["restVolume"][0]
    with pytest.raises(E, match="ipcgpu error -4"):  # the iterative solver with a gas chamber ...
        c.set_solver(2)
    c.chamber_set_gas(False)
    c.set_solver(2)
    with pytest.raises(E, match="ipcgpu error -4"):  # ... and a gas chamber with the iterative solver
        c.chamber_set_gas(True, AMBIENT, 1.4)
    c.chamber_set_gas(False)  # (all constant is no gas chamber: accepted)
    c.set_solver(0)
    # nine gas chambers
    n = 9
    Vn = np.vstack([cm.CUBE_X * SIZE + [0.2 * i, 0.0, 0.0] for i in range(n)])
    c9 = gpu_lib.Context(0)
    c9.set_mesh(Vn, np.zeros((0, 4), dtype=np.int32), YM=1e5, PR=0.4, density=RHO)
    c9.set_chambers([cm.CUBE_TRI + 8 * i for i in range(n)], 20.0)
    with pytest.raises(E, match="ipcgpu error -1.*9 gas chambers"):
        c9.chamber_set_gas(True, AMBIENT, 1.4)
    c9.chamber_set_gas([True] * 8 + [False], AMBIENT, 1.4)
    assert c9.chamber_gas_get()["isGas"].sum() == 8
    vol, gauge, beta = c9.chamber_gas_state()
    assert np.all(np.abs(vol - SIZE ** 3) <= 1e-15) and gauge[8] == 20.0 and beta[8] == 0.0 and np.all(beta[:8] > 0)


def test_set_gas_with_zeros_leaves_a_constant_run_alone(gpu_lib):
    """A constant-only chamber run gives iterates bit-identical to the same run after chamber_set_gas(zeros)."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    out = []
    for call in (False, True):
        c = cloth_context(gpu_lib, V, tri, 20.0, 0, 0.01, held=[0])
        if call:
            c.chamber_set_gas(False, AMBIENT, 1.4)
        its = [c.solve_timestep(100) for _ in range(3)]
        out.append((its, c.state()["V"], c.chamber_energy(), c.chamber_gradient_add()))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] and np.array_equal(out[0][3], out[1][3])
