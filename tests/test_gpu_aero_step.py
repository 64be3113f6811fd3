"""Wind and air drag in the time stepper: a sheet that falls in still air, a sheet driven by a wind, a one-sided cloth cube in a wind, the lagging rule, a
wind changed between steps, the damping matrix, the error paths, and that a context without aerodynamic surfaces is left alone.  Small meshes; the
multifrontal and the iterative solver where the issue is the stepper.

The sheet: 2 x 2 quads (9 nodes, 8 triangles) of side 1/8 in the plane y = 1 (gravity acts along -y), its corner at (1, 1, 1): binary coordinates, none
of them zero -- the shell's own terms leave forces of the order of 1e-25 N in a flat sheet at rest (the rounding of its rest angles), which move a
coordinate that IS zero by 1e-24 and are absorbed by the rounding of any other, so that "at rest to the bit" below is about the drag alone --, a cloth
of thickness H and density RHO.  Its lumped
masses and its nodal drag shares are both a third of the adjacent triangle areas, so a uniform translation is an exact solution of the discrete system:
every node obeys the scalar recursions stated beside each test, with a = rho_a C / (2 RHO H).  Bounds are iterate_bound of test_gpu_attach_step.py (the
stepper stops within 2 tol of each step's minimiser; the drag only damps the recursion of that error).
LINE_SEARCH_FLOOR (as there): the incremental potential is ~ m (dt^2 g)^2 / 2 = 6e-10 here, lambda >= a nodal mass 1e-4: the line search cannot resolve
steps under sqrt(2 u E / lambda) = 4e-11; the tolerance 1e-6 x 0.35 x 0.01 = 3.5e-9 is ninety times that."""
import numpy as np
import pytest

import aero_mp as am
import chamber_mp as cm
from codim_common import NO_T, step_context
from test_gpu_attach_step import iterate_bound

pytestmark = pytest.mark.gpu

SOLVERS = (0, 2)
G = 9.80665
RHO, H, YM, PR = 30.0, 1e-3, 1e5, 0.3
RHO_A, CN = 1.225, 1.28
DT, REL_TOL = 0.01, 1e-6


def sheet():
    idx = lambda i, j: 3 * i + j
    V = np.array([[1.0 + 0.125 * i, 1.0, 1.0 + 0.125 * j] for i in range(3) for j in range(3)])
    tri = np.array([t for i in range(2) for j in range(2) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))], dtype=np.int32)
    return V, tri


EDGES = np.array(sorted({(min(a, b), max(a, b)) for t in sheet()[1] for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}))


def sheet_context(gpu_lib, solver=0, gravity=False, cn=CN, ct=0.0, one_sided=False, wind=None, aero=True, damping=None, V=None, tri=None):
    if V is None:
        V, tri = sheet()

    def body(c):
        c.set_shell(tri, H, YM, PR, RHO)
        if aero:
            c.set_aero([tri], cn, ct, one_sided)
            if wind is not None:
                c.aero_set_wind(wind, RHO_A)
    c = step_context(gpu_lib, V, body, solver, None, YM, RHO, DT, gravity=gravity)
    if damping is not None:
        c.set_damping(damping)
    c.set_rel_tol(REL_TOL)
    c.precompute()
    return c


def decay(r, a, drive=0.0, dt=DT):
    """backward Euler of r' = drive - a r |r| for r >= 0: the root of dt a r^2 + r - (r_k + dt drive) = 0"""
    return (-1.0 + np.sqrt(1.0 + 4.0 * dt * a * (r + dt * drive))) / (2.0 * dt * a)


def unstrained(X, V, e):
    return np.all(np.abs(np.linalg.norm(X[EDGES[:, 0]] - X[EDGES[:, 1]], axis=1) - np.linalg.norm(V[EDGES[:, 0]] - V[EDGES[:, 1]], axis=1)) <= 2 * e)


@pytest.mark.parametrize("solver", SOLVERS)
def test_horizontal_sheet_falls_to_its_terminal_speed(gpu_lib, solver):
    """Still air, gravity.  With the downward speed s: m (s_(k+1) - s_k) / dt = m g - (rho_a A_i / 2) Cn s_(k+1)^2, i.e. dt a s^2 + s - (s_k + dt g) = 0.
    Every node follows it for 20 steps within iterate_bound, the membrane stays unstrained within twice that (two end points), the speed rises towards
    sqrt(g / a) from below and the last step's is at least 0.9 of it (checked on the recursion itself).  Without the drag the sheet falls with s = g t: by
    the 20th step 1.96 m / s against a terminal speed of 0.61 m / s."""
    V, tri = sheet()
    a = RHO_A * CN / (2 * RHO * H)
    sT = np.sqrt(G / a)
    s, ref = 0.0, []
    for k in range(20):
        s = decay(s, a, G)
        ref.append(s)
    assert all(x < y for x, y in zip(ref, ref[1:])) and 0.9 * sT <= ref[-1] < sT  # the parameters: 20 steps reach nine tenths of the terminal speed
    c = sheet_context(gpu_lib, solver, gravity=True)
    prev, drop = V.copy(), 0.0
    for k in range(1, 21):
        assert c.solve_timestep(100) < 100
        X = c.state()["V"]
        drop += DT * ref[k - 1]
        e = iterate_bound(REL_TOL, V, DT, k)
        speed = (prev[:, 1] - X[:, 1]) / DT
        prev = X
        print(f"solver {solver} step {k}: speed {speed.min():.9f} .. {speed.max():.9f} (recursion {ref[k - 1]:.9f}, terminal {sT:.6f}), worst offset {np.abs(X - (V - [0, drop, 0])).max():.3g} (bound {e:.3g})")
        assert np.all(np.abs(X - (V - [0.0, drop, 0.0])) <= e)
        assert unstrained(X, V, e)
        assert np.all(np.abs(speed - ref[k - 1]) <= 2 * e / DT) and np.all(speed < sT)
    assert drop > 1e3 * e and G * 20 * DT - ref[-1] > 1e3 * 2 * e / DT  # far from free fall


@pytest.mark.parametrize("solver", SOLVERS)
def test_sheet_in_a_wind(gpu_lib, solver):
    """No gravity.  Head-on (w along the normal): with r = W - v, v_(k+1) = v_k + dt a r_(k+1)^2, i.e. dt a r^2 + r - r_k = 0.  Oblique (w = (Wx, Wy, 0)): the
    normal and the tangential component follow that recursion on their own, with Cn and Ct -- the normal force depends on u_n alone, the tangential on u_t
    alone, and the lagged normal of a translating sheet never changes.  Edge-on with ct 0: no force at all, the sheet stays where it is to the bit."""
    V, tri = sheet()
    for wind, ct in (((0.0, 2.0, 0.0), 0.0), ((1.5, -2.0, 0.0), 0.5)):
        an, at = RHO_A * CN / (2 * RHO * H), RHO_A * ct / (2 * RHO * H)
        c = sheet_context(gpu_lib, solver, cn=CN, ct=ct, wind=wind)
        rn, rt, pos = abs(wind[1]), abs(wind[0]), np.zeros(3)
        for k in range(1, 11):
            assert c.solve_timestep(100) < 100
            rn, rt = decay(rn, an), (decay(rt, at) if ct > 0 else rt)
            vel = np.array([np.sign(wind[0]) * (abs(wind[0]) - rt) if ct > 0 else 0.0, np.sign(wind[1]) * (abs(wind[1]) - rn), 0.0])
            pos += DT * vel
            X = c.state()["V"]
            e = iterate_bound(REL_TOL, V, DT, k)
            print(f"solver {solver} wind {wind} ct {ct:g} step {k}: velocity of the recursion {vel}, worst offset {np.abs(X - (V + pos)).max():.3g} (bound {e:.3g})")
            assert np.all(np.abs(X - (V + pos)) <= e) and unstrained(X, V, e)
        assert np.abs(pos).max() > 1e3 * e
    c = sheet_context(gpu_lib, solver, cn=CN, ct=0.0, wind=(3.0, 0.0, -2.0))  # edge-on: in the sheet's plane
    for k in range(3):
        assert c.solve_timestep(100) < 100
        assert np.array_equal(c.state()["V"], V)
    F, lag, tot = c.aero_state()
    assert np.all(F == 0.0) and np.all(tot[:4] == 0.0) and np.all(np.abs(lag[:, 1]) == 1.0) and np.all(lag[:, [0, 2]] == 0.0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_one_sided_cloth_cube_in_a_wind_takes_the_momentum_the_air_gives(gpu_lib, solver):
    """The closed cloth cube of test_gpu_chamber_step.py (8 nodes, 12 outward triangles), one-sided, ct 0, in a wind, no gravity.  The elastic forces sum to
    zero, so at the end of a step the Newton residual r = M (x - xTilde) + dt^2 (grad W + grad D), summed over the nodes, is dt M (v_(k+1) - v_k) summed
    minus dt^2 F, F the total force of aero_state at the accepted state: |sum m (v_(k+1) - v_k) - dt F| <= |sum r| / dt <= sqrt(3 n) |H|_2 delta / dt with H
    the Newton matrix and delta = iterate_bound of ONE step (2 tol: the distance of the accepted iterate from the step's minimiser).  The dissipated power
    is not negative, and only triangles whose u_n is positive carry a force."""
    V, tri = cm.CUBE_X * 0.1 + [0.3, 0.2, 0.1], cm.CUBE_TRI.copy()
    wind = np.array([4.0, 1.0, -0.5])
    c = sheet_context(gpu_lib, solver, cn=CN, ct=0.0, one_sided=True, wind=wind, V=V, tri=tri)
    m = c.features()["mass"]
    delta = iterate_bound(REL_TOL, V, DT, 0)
    prev, vprev, moved = V.copy(), np.zeros(V.shape), 0.0
    for k in range(1, 9):
        assert c.solve_timestep(100) < 100
        X = c.state()["V"]
        v = (X - prev) / DT
        F, lag, tot = c.aero_state()
        c.assemble_newton(DT * DT, True)
        ia, ja = c.get_pattern()
        A = np.zeros((len(ia) - 1, len(ia) - 1))
        A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
        Hn = np.linalg.norm(A + np.triu(A, 1).T, 2)
        dP = (m[:, None] * (v - vprev)).sum(axis=0)
        bound = np.sqrt(3 * len(V)) * Hn * delta / DT
        # the lagged records are those of the step's start: u of every triangle from them, on the host
        u = (X[tri].mean(axis=1) - lag[:, 4:7]) / DT - wind
        un = np.einsum("ta,ta->t", u, lag[:, :3])
        print(f"solver {solver} step {k}: momentum gained {dP}, dt F {DT * tot[:3]}, defect {np.abs(dP - DT * tot[:3]).max():.3g} (bound {bound:.3g}), power {tot[3]:.6g}, "
              f"{int((un > 0).sum())} of 12 triangles face the wind")
        assert np.all(np.abs(dP - DT * tot[:3]) <= bound)
        assert tot[3] >= 0.0
        margin = 1e-9 * np.abs(u).max()
        assert np.all(F[un < -margin] == 0.0) and np.all(np.abs(F[un > margin]).max(axis=1) > 0.0) and (un > margin).any() and (un < -margin).any()
        assert abs(tot[4] - lag[np.abs(F).max(axis=1) > 0, 3].sum()) <= 64 * am.U * tot[4]
        moved = max(moved, np.abs(dP).max())
        prev, vprev = X, v
    assert moved > 1e3 * bound  # the wind really pushed the cube


def test_lagged_records_follow_the_step_start_and_nothing_else(gpu_lib):
    """After begin_timestep the records are those of the positions the step starts from (mpmath, within the bound test_aero_mp.py derives for the plan's
    record, doubled for the kernel's contracted products); set_positions leaves them where they are, to the bit."""
    V, tri = sheet()
    c = sheet_context(gpu_lib, 0, gravity=True)
    assert np.array_equal(c.aero_state(with_force=False)[1], am.rest_records(V, tri))  # until the first step: the plan's rest records
    x0 = V + 0.01 * np.random.default_rng(5).standard_normal(V.shape)
    c.set_positions(x0)
    assert np.array_equal(c.aero_state(with_force=False)[1], am.rest_records(V, tri))  # set_positions does not move them
    c.begin_timestep()
    lag = c.aero_state(with_force=False)[1]
    for t, rec in zip(tri, lag):
        X = [x0[i] for i in t]
        n, A, cen = am.record_mp(*X)
        e1, e2 = np.linalg.norm(X[1] - X[0]), np.linalg.norm(X[2] - X[0])
        rel = 16 * am.U * (e1 * e2 / (2 * float(A))) * (1 + np.abs(np.array(X)).max() / min(e1, e2))
        assert all(abs(float(n[a]) - rec[a]) <= rel for a in range(3)) and abs(float(A) - rec[3]) <= rel * float(A)
        assert np.array_equal(rec[4:7], am.rest_record(*X)[4:7]) and rec[7] == 0.0  # the centroid: sums and one division, to the bit
    c.set_positions(V)
    assert np.array_equal(c.aero_state(with_force=False)[1], lag)


def test_wind_changed_between_steps_acts_in_the_next_step(gpu_lib):
    """two steps in still air without gravity: at rest to the bit.  Then a head-on wind is set: nothing has moved yet, and the next steps follow the
    recursion of test_sheet_in_a_wind from rest."""
    V, tri = sheet()
    c = sheet_context(gpu_lib, 0)
    for _ in range(2):
        assert c.solve_timestep(100) < 100
        assert np.array_equal(c.state()["V"], V)
    c.aero_set_wind((0.0, -3.0, 0.0), RHO_A)
    assert np.array_equal(c.state()["V"], V)
    a, r, pos = RHO_A * CN / (2 * RHO * H), 3.0, 0.0
    for k in range(1, 4):
        assert c.solve_timestep(100) < 100
        r = decay(r, a)
        pos -= DT * (3.0 - r)
        e = iterate_bound(REL_TOL, V, DT, k)
        assert np.all(np.abs(c.state()["V"] - (V + [0.0, pos, 0.0])) <= e)
    assert abs(pos) > 1e3 * e


@pytest.mark.parametrize("one_triangle", (True, False))
def test_damping_matrix_is_built_without_the_air_drag(gpu_lib, one_triangle):
    """The lagged damping matrix D = (damping / dt) x (stiffness Hessians at the lagged positions) is what ipcgpu_assemble_newton adds while damping is on:
    D = A(damping on) - A(damping off) at one state.  precompute() builds D at the start positions IN A WIND: unmasked, D would carry (damping / dt) x the
    drag Hessian at u = -w, which aero_hessian_add reproduces and which is asserted to be far above anything else here.  The wind is then switched off: at
    the start positions in still air u = 0, the drag kernels write nothing, and the contexts with and without surfaces run the same arithmetic on A -- so
    their differences D agree TO THE BIT if and only if the matrix precompute() built is the same.  To the bit on one shell triangle (every entry
    receives one addend per kernel: no atomic sum depends on an order); on the sheet, whose entries receive up to six addends from the shell kernels in
    any order, to 64 u of the largest entry (the tolerance of test_gpu_chamber_step.py's damping test, for its reason)."""
    V, tri = sheet()
    if one_triangle:
        V, tri = V[[0, 3, 4]].copy(), np.array([[0, 1, 2]], dtype=np.int32)
    damping, D = 0.1, []  # (at the rest positions: the lagged centroids are the current ones to the bit, and the membrane's rest stiffness is not zero)
    for aero in (True, False):
        def body(c):
            c.set_shell(tri, H, YM, PR, RHO)
            if aero:
                c.set_aero([tri], CN, 0.4, False)
                c.aero_set_wind((1.0, 3.0, -2.0), RHO_A)
        c = step_context(gpu_lib, V, body, 0, None, YM, RHO, DT, gravity=False)
        c.set_damping(damping)
        c.set_rel_tol(REL_TOL)
        c.precompute()
        if aero:
            c.set_zero()
            c.aero_hessian_add(damping / DT, True)
            unmasked = np.abs(c.get_a()).max()
            c.aero_set_wind((0.0, 0.0, 0.0), RHO_A)
        c.assemble_newton(DT * DT, True)
        on = c.get_a()
        c.set_damping(0.0)
        c.assemble_newton(DT * DT, True)
        off = c.get_a()
        D.append(on - off)
        amax = np.abs(on).max()
    tol = 0.0 if one_triangle else 64 * cm.U * amax
    print(f"damping matrix with surfaces against none: {np.abs(D[0] - D[1]).max():.3g} (tolerance {tol:.3g}); largest entry {np.abs(D[1]).max():.3g}; unmasked drag would add up to {unmasked:.3g}")
    assert np.abs(D[1]).max() > 0 and unmasked > 1e6 * 64 * cm.U * amax
    assert np.abs(D[0] - D[1]).max() <= tol


def test_error_paths(gpu_lib):
    V, tri = sheet()
    E = gpu_lib.IpcGpuError
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_aero([tri])
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.aero_set_wind((1.0, 0.0, 0.0))  # without a surface: nothing, and no error
    assert c.aero_energy() == 0.0 and c.aero_get()["n"] == 0 and np.all(c.aero_get()["wind"] == 0.0)
    c.set_shell(tri, H, YM, PR, RHO)
    c.set_aero([tri])
    assert c.aero_get()["cn"][0] == 1.28 and c.aero_get()["ct"][0] == 0.0 and not c.aero_get()["oneSided"][0] and c.aero_get()["density"] == 1.225
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -3.*opt_init"):
        c.aero_energy()  # before opt_init: no dt yet
    with pytest.raises(E, match="ipcgpu error -3"):
        c.aero_gradient_add(1.0, True)
    for bad in (((np.nan, 0.0, 0.0), 1.2), ((0.0, 0.0, 0.0), 0.0), ((0.0, 0.0, 0.0), -1.0), ((0.0, np.inf, 0.0), 1.2)):
        with pytest.raises(E, match="ipcgpu error -1"):
            c.aero_set_wind(*bad)
    c.opt_init(DT, False)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.system_report()
    with pytest.raises(E, match="ipcgpu error -3"):
        c.set_aero([tri])  # after opt_init
    with pytest.raises(E, match="ipcgpu error -3"):
        c.set_aero([])  # removing them after opt_init, too
    bad = {"out of range": ([np.where(tri == 8, 9, tri)], 1.0, 0.0), "repeats a node": ([np.vstack([tri[:-1], [[1, 1, 5]]])], 1.0, 0.0),
           "listed twice": ([np.vstack([tri, tri[2:3, [1, 2, 0]]])], 1.0, 0.0), "listed twice, flipped in another surface": ([tri, tri[:1, ::-1]], 1.0, 0.0),
           "zero rest area": ([np.vstack([tri, [[0, 1, 2]]])], 1.0, 0.0), "negative coefficient": ([tri], -1.0, 0.0), "not finite": ([tri], 1.0, np.nan)}
    for word, args in bad.items():
        c = gpu_lib.Context(0)
        c.set_mesh(V, NO_T)
        with pytest.raises(E, match="ipcgpu error -1.*surface [01].*" + word.split(",")[0]):
            c.set_aero(*args)
        assert c.aero_get()["n"] == 0
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_aero([tri[:4], tri[4:]], [1.0, 2.0], 0.1, [False, True])
    c.aero_set_wind((1.0, 2.0, 3.0), 1.0)
    c.set_aero([tri])  # a second call replaces the surfaces; wind and density stay
    assert c.aero_get()["n"] == 1 and np.array_equal(c.aero_get()["wind"], [1.0, 2.0, 3.0]) and c.aero_get()["density"] == 1.0
    c.set_mesh(V, NO_T)  # a new mesh drops them
    assert c.aero_get()["n"] == 0 and c.aero_get()["nTri"] == 0 and np.all(c.aero_get()["wind"] == 0.0)


def test_pattern_built_before_set_aero_is_rebuilt(gpu_lib):
    V, tri = sheet()
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shell(tri[:2], H, YM, PR, RHO)
    c.set_pattern()
    n0 = len(c.get_pattern()[1])
    c.set_aero([tri])
    assert len(c.get_pattern()[1]) > n0
    c.opt_init(DT, False)
    c.aero_set_wind((1.0, 2.0, 3.0))
    c.aero_hessian_add(1.0, True)  # every block is there (IPCGPU_ERR_STATE otherwise)


def test_no_surface_leaves_a_block_and_cloth_scene_bit_identical(gpu_lib):
    """A block and a one-triangle cloth (a single shell element: no atomic sum depends on an order), five steps under gravity.  Three contexts: no call;
    set_aero with nSurf == 0; surfaces set, replaced, then removed.  Pattern, gradient, matrix values, masses and the positions after every step agree to
    the bit, and every query of a context without surfaces returns empty results."""
    from ipc_amd import scene
    Vb, Tb = scene.make_bar(3, 2, 2, size=(1.5, 1.0, 1.0))
    nb = len(Vb)
    V = np.vstack([Vb, [[0.0, 3.0, 0.0], [0.3, 3.0, 0.0], [0.0, 3.0, 0.3]]])
    tri = np.array([[nb, nb + 1, nb + 2]])
    skin = scene.surface_tris(Tb)
    x = V + 0.01 * np.random.default_rng(3).standard_normal(V.shape)
    out = []
    for mode in range(3):
        c = gpu_lib.Context(0)
        c.set_mesh(V, Tb)
        c.set_shell(tri, 1e-3, 1e5, 0.3, 1000.0)
        m0 = c.features()["mass"]
        if mode == 1:
            c.set_aero([])
        if mode == 2:
            c.set_aero([skin, tri], 1.28, 0.1, [True, False])
            c.aero_set_wind((1.0, 0.0, 0.0))
            assert c.aero_get()["n"] == 2 and np.array_equal(c.features()["mass"], m0)
            c.set_aero([tri])
            assert c.aero_get()["n"] == 1 and c.aero_get()["nTri"] == 1
            c.set_aero([])
        assert np.array_equal(c.features()["mass"], m0)
        c.set_positions(x)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(np.vstack([scene.surface_tris(Tb), tri]).astype(np.int32))
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        a = c.get_a()
        steps = []
        for _ in range(5):
            assert c.solve_timestep(100) < 100
            steps.append(c.state()["V"])
        out.append((g, a, np.array(steps), c.get_pattern()[0], c.get_pattern()[1], m0))
        assert c.aero_get()["n"] == 0 and c.aero_energy() == 0.0 and c.aero_energy_per_elem().shape == (0,)
        assert np.array_equal(c.aero_gradient_add(1.0, True), np.zeros(3 * len(V))) and c.aero_state()[0].shape == (0, 3)
        c.aero_hessian_add(1.0, True)
    for p, q, r in zip(*out):
        assert np.array_equal(p, q) and np.array_equal(p, r)
