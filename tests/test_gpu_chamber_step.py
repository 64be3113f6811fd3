"""Pressure chambers in the time stepper and the building blocks: a block under outside pressure, a free and a held pressurised cloth cube, a pressure
schedule, the same scene far from the origin, the damping matrix, the error paths, and that a context without chambers is left alone.  Small meshes; the
multifrontal and the iterative solver where cheap.

LINE_SEARCH_FLOOR (as test_gpu_attach_step.py): the line search compares incremental potentials in fp64, and these now carry dt^2 p V, so it cannot see a
decrease below u E with E ~ dt^2 |p| V; the stepper never gets under |step| ~ sqrt(2 u E / lambda), lambda the softest eigenvalue of the Newton matrix.
Every relative tolerance below is set well above that (the figures are beside each test) and every asserted bound is derived from the tolerance set."""
import numpy as np
import pytest

import chamber_mp as cm
from codim_common import NO_T, five_tet_cube, step_context
from test_gpu_attach_step import iterate_bound

pytestmark = pytest.mark.gpu

SOLVERS = (0, 2)
RHO = 1000.0
SIZE = 0.1
CLOTH = dict(thickness=1e-3, YM=1e5, PR=0.3)  # membrane stiffness E h = 100 N / m


def cloth_cube(lo=(0.0, 0.0, 0.0)):
    return cm.CUBE_X * SIZE + np.asarray(lo, dtype=np.float64), cm.CUBE_TRI.copy()


def cloth_context(gpu_lib, V, tri, p, solver=0, dt=0.01, held=None, chambers=True, relTol=1e-6, damping=None):
    def body(c):
        c.set_shell(tri, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO)
        if chambers:
            c.set_chambers([tri], [p])
    c = step_context(gpu_lib, V, body, solver, None, 1e5, RHO, dt, gravity=False, held=held)
    if damping is not None:
        c.set_damping(damping)
    c.set_rel_tol(relTol)
    c.precompute()
    return c


def dense_newton(c, coef):
    c.assemble_newton(coef, True)
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A + np.triu(A, 1).T


@pytest.mark.parametrize("solver", SOLVERS)
def test_block_under_outside_pressure_shrinks_uniformly(gpu_lib, solver):
    """A free five-tet block whose 12 boundary triangles (the tetrahedra's own faces: with other diagonals the nodal shares of the pressure would differ
    from those of the constant stress, and the equilibrium would not be a uniform scaling) are a chamber at p < 0 (an outside hydrostatic pressure |p| of 1 % of the bulk modulus), no gravity.
    A uniform scaling x -> s x is an exact equilibrium of the discrete system: linear tetrahedra represent it, its stress is the constant
    (dpsi/ds)/(3 s^2) I, and for a closed surface the nodal pressure forces are those of a constant traction.  Per rest volume the static energy is
    psi(s I) + |p| s^3 with the neo-Hookean psi = mu/2 (3 s^2 - 3) - 3 mu ln s + lam/2 (3 ln s)^2 (nh_device.h: P = mu (F - F^-T) + lam ln J F^-T), so s is
    the root of  3 mu (s - 1/s) + 9 lam ln s / s + 3 |p| s^2 = 0, solved here by bisection.  Backward Euler with dt = 1 damps the breathing mode
    (w ~ sqrt(E / rho) / L = 1e3 rad / s) by 1e-3 per step: after 4 steps what remains is the iterate tolerance.  Every edge's length ratio lies within
    2 e / (rest length) of s, e = iterate_bound (two end points, each within e).
    Floor: E ~ dt^2 |p| V = 170, lambda ~ dt^2 K L = 1.7e6: 1.5e-10; the tolerance 1e-7 x 0.17 x 1 = 1.7e-8 is a hundred times that."""
    YM, PR = 1e7, 0.4
    mu, lam = YM / (2 * (1 + PR)), YM * PR / ((1 + PR) * (1 - 2 * PR))
    p = -0.01 * (lam + 2 * mu / 3)
    f = lambda s: 3 * mu * (s - 1 / s) + 9 * lam * np.log(s) / s + 3 * abs(p) * s * s
    a, b = 0.9, 1.0
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
    assert len(skin) == 12
    c = step_context(gpu_lib, V, lambda c: c.set_chambers([skin], [p]), solver, T, YM, RHO, dt, gravity=False)
    c.set_rel_tol(relTol)
    c.precompute()
    assert abs(c.chamber_get()["restVolume"][0] - SIZE ** 3) <= 1e-15
    for k in range(steps):
        assert c.solve_timestep(200) < 200
    X = c.state()["V"]
    edges = np.array([(i, j) for i in range(8) for j in range(i + 1, 8)])
    ratio = np.linalg.norm(X[edges[:, 0]] - X[edges[:, 1]], axis=1) / np.linalg.norm(V[edges[:, 0]] - V[edges[:, 1]], axis=1)
    e = iterate_bound(relTol, V, dt, steps)
    bound = 2 * e / np.linalg.norm(V[edges[:, 0]] - V[edges[:, 1]], axis=1).min()
    print(f"solver {solver}: s {s:.9f}, edge ratios {ratio.min():.9f} .. {ratio.max():.9f}, worst |ratio - s| {np.abs(ratio - s).max():.3g} (bound {bound:.3g})")
    assert 1 - s > 1e2 * bound  # the block really shrank
    assert np.all(np.abs(ratio - s) <= bound)
    vol = c.chamber_state()[0][0]
    assert abs(vol / SIZE ** 3 - s ** 3) <= 3 * bound * 1.01


@pytest.mark.parametrize("solver", SOLVERS)
def test_free_pressurised_cloth_cube_keeps_its_momenta(gpu_lib, solver):
    """A free cloth cube (8 nodes, 12 shell triangles) with p > 0, no gravity, from rest.  The pressure energy of a closed surface is invariant under
    translation and rotation (test_chamber_mp.py), so as for the free spring of test_gpu_attach_step.py the exact discrete trajectory keeps the total
    linear momentum P at zero and obeys L_(k+1) - L_k = dt sum m v_(k+1) x v_k (backward Euler's own term).  Bounds as derived there: every x_k within
    e_k = iterate_bound of the exact discrete trajectory, |P| <= 2 M e_k / dt, the defect of the angular balance <= 4 M e_k R / dt + 6 M e_k vmax.
    Floor: E ~ dt^2 p V = 2e-6, lambda ~ m + dt^2 E h = 0.0175: 1.6e-10; the tolerance 1e-6 x 0.17 x 0.01 = 1.7e-9 is ten times that."""
    V, tri = cloth_cube([0.3, 0.2, 0.1])
    relTol, dt, steps, p = 1e-6, 0.01, 10, 20.0
    c = cloth_context(gpu_lib, V, tri, p, solver, dt, relTol=relTol)
    m = c.features()["mass"]
    V0 = c.chamber_state()[0][0]
    assert abs(V0 - SIZE ** 3) <= 1e-15 and abs(c.chamber_get()["restVolume"][0] - SIZE ** 3) <= 1e-15
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
        Vmax = max(Vmax, c.chamber_state()[0][0])
        print(f"solver {solver} step {k}: |P| {np.linalg.norm(Pm):.3g} (bound {bP:.3g}), defect of the angular momentum balance {np.linalg.norm(torque):.3g} "
              f"(bound {bL:.3g}), four nodes' momentum {moved:.3g}, volume / rest {c.chamber_state()[0][0] / V0:.6f}")
        assert np.linalg.norm(Pm) <= bP and np.linalg.norm(torque) <= bL
    assert moved > 1e2 * bP  # the pressure really moved the nodes: the zero is a cancellation, not rest
    assert Vmax > V0 * (1 + 1e-4)  # the volume rises above the rest volume


def test_held_cloth_cube_comes_to_rest_where_shell_and_pressure_balance(gpu_lib):
    """The cloth cube held by one node, three pressures, backward Euler with dt = 10 for 8 steps.  At the end of a step the Newton residual
    dt^2 (grad W_shell + grad W_chamber) + m (x - xTilde) is at most |H| delta with H the Newton matrix and delta = 2 tol the distance of the iterate from
    the step's minimiser (iterate_bound for one step), and x - xTilde = (x_k - x_(k-1)) - (x_(k-1) - x_(k-2)) is what the motion still does, measured here:
    |grad W_shell + grad W_chamber| <= (|H|_2 delta + max m (|d_k| + |d_(k-1)|) sqrt(3 n)) / dt^2 on the free nodes.  The final volume increases strictly
    with p.  Floor: E ~ dt^2 p V = 4, lambda >= m = 0.0075: 3.4e-7 at the very worst (a mode without any stiffness); the tolerance 1e-6 x 0.17 x 10 = 1.7e-6 is
    five times that."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    relTol, dt, steps = 1e-6, 10.0, 8
    vols = []
    for p in (10.0, 20.0, 40.0):
        c = cloth_context(gpu_lib, V, tri, p, 0, dt, held=[0], relTol=relTol)
        m = c.features()["mass"]
        hist = [V.copy()]
        for k in range(steps):
            assert c.solve_timestep(300) < 300
            hist.append(c.state()["V"])
        g = c.chamber_gradient_add(1.0, True, c.shell_gradient_add(1.0, True)).reshape(-1, 3)
        H = dense_newton(c, dt * dt)
        delta = 2 * relTol * np.linalg.norm(V.max(0) - V.min(0)) * dt
        d1, d0 = np.abs(hist[-1] - hist[-2]).max(), np.abs(hist[-2] - hist[-3]).max()
        bound = (np.linalg.norm(H, 2) * delta + m.max() * (d1 + d0) * np.sqrt(3 * len(V))) / dt ** 2
        vol = c.chamber_state()[0][0]
        vols.append(vol)
        print(f"p {p:g}: |g| on the free nodes {np.linalg.norm(g[1:]):.3g} (bound {bound:.3g}; pressure force per face {p * SIZE ** 2:.3g}), last steps moved "
              f"{d1:.3g}, {d0:.3g}, volume / rest {vol / SIZE ** 3:.6f}")
        assert np.all(g[0] == 0.0) and np.linalg.norm(g[1:]) <= bound
        assert bound < 0.1 * p * SIZE ** 2  # the bound means something: a tenth of one face's pressure force
        assert np.all(hist[-1][0] == V[0])
    assert SIZE ** 3 < vols[0] < vols[1] < vols[2]


def test_pressure_schedule_between_steps(gpu_lib):
    """chamber_set_pressure between steps: a step at p = 0 equals the same step of a context without chambers (a cube with one node held that starts
    stretched, so that it moves without any pressure).  What the two contexts assemble at equal positions -- gradient, matrix, incremental potential --
    agrees to rounding: 64 u of the largest entry, which covers the one thing that may differ, the order of the shell's atomic sums on a cube whose
    entries receive several addends (a chamber with p = 0 launches kernels that write nothing).  The stepped positions are held to the iterate bound of
    one step on both sides and no tighter: an iterate that differs in its last bits may end the Newton iteration one step earlier or later.  Raising p
    afterwards moves the nodes: three more steps end far (a hundred iterate bounds) from where the context without chambers ends."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    x0 = V + 0.02 * (V - V.mean(axis=0))  # stretched by 2 %: the cloth moves without any pressure
    relTol, dt = 1e-6, 0.01
    out, asm = [], []
    for chambers in (True, False):
        c = step_context(gpu_lib, V, lambda c: (c.set_shell(tri, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO), chambers and c.set_chambers([tri], [30.0])),
                         0, None, 1e5, RHO, dt, gravity=False, held=[0], x0=x0)
        c.set_rel_tol(relTol)
        c.precompute()
        if chambers:
            c.chamber_set_pressure(0.0)
            assert c.chamber_get()["pressure"][0] == 0.0 and c.chamber_energy() == 0.0
        asm.append((c.assemble_newton(dt * dt, True, with_gradient=True), c.get_a(), np.array([c.incremental_potential(dt * dt)])))
        assert c.solve_timestep(100) < 100
        out.append(c.state()["V"])
        if chambers:
            withP = c
    for name, a, b in zip(("gradient", "matrix", "incremental potential"), *asm):
        print(f"{name} at p = 0 against no chambers: {np.abs(a - b).max():.3g} (64 u max = {64 * cm.U * np.abs(b).max():.3g})")
        assert np.abs(a - b).max() <= 64 * cm.U * np.abs(b).max() and np.abs(b).max() > 0
    e = iterate_bound(relTol, V, dt, 1)
    print(f"step at p = 0 against no chambers: {np.abs(out[0] - out[1]).max():.3g} (bound {2 * e:.3g}); the step moved {np.abs(out[1] - x0).max():.3g}")
    assert np.abs(out[0] - out[1]).max() <= 2 * e and np.abs(out[1] - x0).max() > 1e2 * e
    # raising the pressure: the next steps differ from the unpressurised continuation (c is the context without chambers)
    withP.chamber_set_pressure([40.0])
    for _ in range(3):
        assert withP.solve_timestep(100) < 100 and c.solve_timestep(100) < 100
    apart = np.abs(withP.state()["V"] - c.state()["V"]).max()
    print(f"three steps at p = 40 against none: {apart:.3g} apart (iterate bound {iterate_bound(relTol, V, dt, 4):.3g})")
    assert apart > 1e2 * iterate_bound(relTol, V, dt, 4)
    assert withP.chamber_get()["pressure"][0] == 40.0
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*not finite"):
        withP.chamber_set_pressure([np.inf])
    assert withP.chamber_get()["pressure"][0] == 40.0


def test_reference_point_follows_the_body(gpu_lib):
    """The held cloth cube at the origin and shifted by (1e3, 0, 0): the same number of Newton iterations +- 1 per step and the same shape, to twice the
    iterate bound plus the rounding of coordinates of size 1e3 (16 u 1e3 covers the shift's own rounding and the steps').  With r_c left at the world
    origin the per-triangle projection would add a stiffness of p x 1e3 against E h = 100 and the counts would differ by far.  After the steps
    chamber_state reports r_c near the body."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    relTol, dt, steps, p = 1e-6, 0.05, 3, 30.0
    shift = np.array([1e3, 0.0, 0.0])
    iters, X = [], []
    for s in (np.zeros(3), shift):
        c = cloth_context(gpu_lib, V + s, tri, p, 0, dt, held=[0], relTol=relTol)
        it = []
        for k in range(steps):
            it.append(c.solve_timestep(200))
            assert it[-1] < 200
        iters.append(it)
        X.append(c.state()["V"] - s)
        r = c.chamber_state()[2][0] - s
        assert np.abs(r - X[-1].mean(axis=0)).max() <= 0.05 * SIZE  # r_c was refreshed at the last step's start: at the body
    e = iterate_bound(relTol, V, dt, steps)
    print(f"iterations {iters[0]} at the origin, {iters[1]} shifted; shapes differ by {np.abs(X[0] - X[1]).max():.3g} (bound {2 * e + 16 * cm.U * 1e3:.3g})")
    assert all(abs(a - b) <= 1 for a, b in zip(*iters))
    assert np.abs(X[0] - X[1]).max() <= 2 * e + 16 * cm.U * 1e3
    assert np.abs(X[0] - V).max() > 1e2 * e


def test_damping_matrix_is_built_without_the_chamber(gpu_lib):
    """The lagged damping matrix D = (damping / dt) x (stiffness Hessians at the lagged positions) is what ipcgpu_assemble_newton adds while damping is on:
    D = A(damping on) - A(damping off) at one state.  precompute() builds D at the start positions.  A context with a PRESSURISED chamber must hold the D
    of the context without chambers -- the chamber's bit is masked out of that assembly; unmasked, D would carry (damping / dt) x the chamber's projected
    Hessian, which chamber_hessian_add reproduces and which is asserted to be far above the tolerance, so the mask alone decides this test.  Tolerance:
    each A carries its entries' rounding and the shell's atomic order (a few u of the largest entry, D included: D dominates A here), and the
    difference adds one more: 64 u max |A|.  Then two damped steps with p = 0 against no chambers, the second on the matrix lagged from the first, to the
    iterate bound on both sides (as test_pressure_schedule_between_steps explains)."""
    V, tri = cloth_cube([0.1, 0.1, 0.1])
    x0 = V + 0.02 * (V - V.mean(axis=0))
    relTol, dt, damping, p = 1e-6, 0.01, 0.1, 30.0
    D, out = [], []
    for chambers in (True, False):
        c = step_context(gpu_lib, V, lambda c: (c.set_shell(tri, CLOTH["thickness"], CLOTH["YM"], CLOTH["PR"], RHO), chambers and c.set_chambers([tri], [p])),
                         0, None, 1e5, RHO, dt, gravity=False, held=[0], x0=x0)
        c.set_damping(damping)
        c.set_rel_tol(relTol)
        c.precompute()
        c.assemble_newton(dt * dt, True)
        on = c.get_a()
        c.set_damping(0.0)
        c.assemble_newton(dt * dt, True)
        off = c.get_a()
        D.append(on - off)
        amax = np.abs(on).max()
        if chambers:
            c.set_zero()
            c.chamber_hessian_add(damping / dt, True)
            unmasked = np.abs(c.get_a()).max()
            c.chamber_set_pressure(0.0)
        c.set_damping(damping)
        for _ in range(2):  # the second step uses the damping matrix lagged from the first
            assert c.solve_timestep(100) < 100
        out.append(c.state()["V"])
    tol = 64 * cm.U * amax
    print(f"damping matrix with a chamber at p = {p:g} against none: {np.abs(D[0] - D[1]).max():.3g} (tolerance {tol:.3g}); largest entry {np.abs(D[1]).max():.3g}; "
          f"an unmasked chamber would add up to {unmasked:.3g}")
    assert np.abs(D[1]).max() > 0 and unmasked > 1e6 * tol
    assert np.abs(D[0] - D[1]).max() <= tol
    e = iterate_bound(relTol, V, dt, 2)
    print(f"damped steps, p = 0 against no chambers: {np.abs(out[0] - out[1]).max():.3g} (bound {2 * e:.3g})")
    assert np.abs(out[0] - out[1]).max() <= 2 * e


def test_error_paths(gpu_lib):
    V, tri = cloth_cube()
    E = gpu_lib.IpcGpuError
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_chambers([tri], [1.0])
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    with pytest.raises(E, match="ipcgpu error -3"):
        c.chamber_set_pressure([1.0])  # no chambers
    c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
    c.set_chambers([tri], [5.0])
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -3.*set_pattern"):
        c.chamber_hessian_add(1.0, True)  # no pattern yet
    c.opt_init(0.01, False)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.system_report()
    with pytest.raises(E, match="ipcgpu error -3"):
        c.set_chambers([tri], [1.0])  # after opt_init
    with pytest.raises(E, match="ipcgpu error -3"):
        c.set_chambers([], [])  # removing them after opt_init, too
    bad = {"not closed": ([tri[:-1]], [1.0]), "inward": ([tri[:, ::-1]], [1.0]), "not finite": ([tri], [np.nan]), "out of range": ([np.where(tri == 7, 8, tri)], [1.0]),
           "repeats a node": ([np.vstack([tri[:-1], [[1, 1, 5]]])], [1.0]), "same direction": ([np.vstack([tri[:-1], tri[-1:, ::-1]])], [1.0])}
    for word, args in bad.items():
        c = gpu_lib.Context(0)
        c.set_mesh(V, NO_T)
        with pytest.raises(E, match="ipcgpu error -1.*chamber 0.*" + word):
            c.set_chambers(*args)
        assert c.chamber_get()["n"] == 0
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_chambers([tri], [1.0])
    c.set_mesh(V, NO_T)  # a new mesh drops the chambers
    assert c.chamber_get()["n"] == 0 and c.chamber_get()["nTri"] == 0


def test_pattern_built_before_set_chambers_is_rebuilt(gpu_lib):
    V, tri = cloth_cube()
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shell(tri[:2], 1e-3, 1e5, 0.3, RHO)
    c.set_pattern()
    n0 = len(c.get_pattern()[1])
    c.set_chambers([tri], [3.0])
    assert len(c.get_pattern()[1]) > n0
    c.opt_init(0.01, False)
    c.set_positions(V + 0.01 * np.random.default_rng(1).standard_normal(V.shape))
    c.chamber_hessian_add(1.0, True)  # every block is there (IPCGPU_ERR_STATE otherwise)


def test_no_chamber_leaves_a_cube_and_cloth_scene_bit_identical(gpu_lib):
    """A block and a one-triangle cloth (a single shell element: every entry receives one addend per kernel, so no atomic sum depends on an order).  Three
    contexts: no call; set_chambers with nCh == 0; a set, replaced by another, then removed.  Pattern, gradient, matrix values, masses and the positions
    after a step agree to the bit, and every query of a context without chambers returns empty results."""
    from ipc_amd import scene
    Vb, Tb = scene.make_bar(3, 2, 2, size=(1.5, 1.0, 1.0))
    nb = len(Vb)
    V = np.vstack([Vb, [[0.0, 3.0, 0.0], [0.3, 3.0, 0.0], [0.0, 3.0, 0.3]]])
    tri = np.array([[nb, nb + 1, nb + 2]])
    skin = scene.surface_tris(Tb)
    if cm.rest_volume(V, skin, cm.ref_point(V, skin)) < 0:
        skin = skin[:, ::-1]
    half = len(skin) // 2
    x = V + 0.01 * np.random.default_rng(3).standard_normal(V.shape)
    out = []
    for mode in range(3):
        c = gpu_lib.Context(0)
        c.set_mesh(V, Tb)
        c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
        m0 = c.features()["mass"]
        if mode == 1:
            c.set_chambers([], [])
        if mode == 2:
            c.set_chambers([skin], [5.0])
            assert c.chamber_get()["n"] == 1 and np.array_equal(c.features()["mass"], m0)
            c.set_chambers([np.vstack([skin[half:], skin[:half]])], [-7.0])
            assert c.chamber_get()["n"] == 1 and c.chamber_get()["nTri"] == len(skin) and c.chamber_get()["pressure"][0] == -7.0
            c.set_chambers([], [])
        assert np.array_equal(c.features()["mass"], m0)
        c.set_positions(x)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(np.vstack([scene.surface_tris(Tb), tri]).astype(np.int32))
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        a = c.get_a()
        assert c.solve_timestep(100) < 100
        out.append((g, a, c.state()["V"], c.get_pattern()[0], c.get_pattern()[1], m0))
        assert c.chamber_get()["n"] == 0 and c.chamber_energy() == 0.0 and c.chamber_energy_per_elem().shape == (0,)
        assert np.array_equal(c.chamber_gradient_add(1.0, True), np.zeros(3 * len(V))) and c.chamber_state()[0].shape == (0,)
        c.chamber_hessian_add(1.0, True)
    for p, q, r in zip(*out):
        assert np.array_equal(p, q) and np.array_equal(p, r)
