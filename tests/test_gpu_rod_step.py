"""Elastic rods in the time stepper and the building blocks: free fall, the hanging equilibrium, a cantilever, dropping onto a block and a plane with
contact, a nearly folded node, the patch assembly beside a shell and tetrahedra, the error paths, and that a context without a rod is left alone.  Small
meshes; the multifrontal and the iterative solver."""
import numpy as np
import pytest

import rod_mp as rmp
from codim_common import five_tet_cube, step_context
from ipc_amd import scene

pytestmark = pytest.mark.gpu

G = 9.80665
SOLVERS = (0, 2)
R, YM, RHO = 2e-3, 1e7, 1000.0
NO_T = np.zeros((0, 4), dtype=np.int32)
NO_SF = np.zeros((0, 3), dtype=np.int32)


def rod_context(gpu_lib, V, seg, solver=0, bend=1.0, T=None, dt=0.01, gravity=True, held=None, x0=None, r=R, E=YM):
    return step_context(gpu_lib, V, lambda c: c.set_rod(seg, r, E, RHO, bend_scale=bend), solver, T, YM, RHO, dt, gravity, held, x0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_free_fall_follows_the_discrete_recursion(gpu_lib, solver):
    """No contact, no constraint: backward Euler gives v += dt g, y += dt v for every node; a rigid translation leaves the rod energy at zero.  Bound: the
    project's iterate tolerance, 1e-9 of the fall distance.  Rod energy: a position error of 1e-9 x 1.5e-3 over a spacing of 0.1 is a strain
    of ~1e-11, squared in the energy: far below 1e-16 of the energy's magnitude sum (rod_mp scale), which is the bound asserted."""
    V, seg = rmp.chain(6, origin=(0.0, 1.0, 0.0))
    c = rod_context(gpu_lib, V, seg, solver)
    c.set_surface(NO_SF, seg)
    c.set_rel_tol(1e-8)
    c.precompute()
    case = rmp._case("fall", V, V, seg, r=R, YM=YM)
    scaleE = float(rmp.chain_reference(rmp.NP, case, magnitudes=True)[0])
    dt, v, fall = 0.01, 0.0, 0.0
    for step in range(5):
        assert c.solve_timestep(50) < 50
        v += dt * G
        fall += dt * v
        X = c.state()["V"]
        print(f"solver {solver} step {step}: fall {fall:.6g}, worst deviation {np.abs(X - (V - [0, fall, 0])).max():.3g}, rod energy {c.rod_energy():.3g}")
        assert np.all(np.abs(X - (V - [0.0, fall, 0.0])) <= 1e-9 * fall)
        assert 0.0 <= c.rod_energy() <= 1e-16 * scaleE


@pytest.mark.parametrize("solver", SOLVERS)
def test_pinned_rod_stays_at_its_hanging_equilibrium(gpu_lib, solver):
    """Nodes 0 .. n down a vertical line, node 0 held, placed at l_i = L (1 + T_i / (E A)) with T_i = g x (the mass below segment i) (pinned in mpmath by
    test_rod_mp.py): the minimiser of every backward-Euler step is this state itself.  Bound: the stepper stops when the Newton step is shorter than
    tol = relTol x (bounding-box diagonal) x dt, so an iterate lies within delta = 2 tol of its step's minimiser (the step that was not taken, doubled for the
    projected Hessian); the error enters the next step's xTilde = 2 x_k - x_(k-1), an undamped recursion e_k = 2 e_(k-1) - e_(k-2) + delta whose solution
    is delta k (k + 1) / 2: after k steps at most delta (k + 1)^2.  Plus the rounding of the placement itself, 64 u of the rod's length."""
    n, L, r, E = 6, 0.1, 2e-3, 1e6
    A = np.pi * r * r
    mass = RHO * A * L / 2 * np.array([1.0] + [2.0] * (n - 1) + [1.0])
    T = np.array([G * mass[i + 1:].sum() for i in range(n)])
    V, seg = rmp.chain(n + 1, spacing=L, axis=(0.0, -1.0, 0.0), origin=(0.0, 1.0, 0.0))
    x = V.copy()
    x[1:, 1] = 1.0 - np.cumsum(L * (1 + T / (E * A)))
    relTol, dt = 1e-9, 0.01
    c = rod_context(gpu_lib, V, seg, solver, held=[0], x0=x, r=r, E=E, dt=dt)
    c.set_surface(NO_SF, seg)
    c.set_rel_tol(relTol)
    c.precompute()
    assert np.allclose(c.rod_get()["mass"], mass, rtol=1e-13, atol=0)
    delta = 2 * relTol * np.linalg.norm(V.max(0) - V.min(0)) * dt
    for k in range(1, 4):
        assert c.solve_timestep(50) < 50
        dev = np.abs(c.state()["V"] - x).max()
        print(f"solver {solver} step {k}: deviation from the closed-form equilibrium {dev:.3g} (bound {delta * (k + 1) ** 2 + 64 * rmp.U * n * L:.3g})")
        assert dev <= delta * (k + 1) ** 2 + 64 * rmp.U * n * L


def _cantilever(gpu_lib, solver, bend, steps=20, dt=0.01):
    """A rod 0.5 long, r = 0.01, E = 1e8, clamped over its first TWO nodes (one held node is a hinge), L = 0.45 free: E I = E pi r^4 / 4 = 0.785, q = rho A g
    = 3.08 N/m, static tip deflection q L^4 / (8 E I) = 0.020, first period 2 pi / (3.516 sqrt(E I / (rho A L^4))) = 0.23 s: after 20 steps of 0.01 s it is
    near its first maximum (measured 0.0231; backward Euler damps the swing towards the static value); ten times the bending stiffness gives a tenth of the
    deflection (measured 0.0025)."""
    V, seg = rmp.chain(11, spacing=0.05, origin=(0.0, 1.0, 0.0))
    held = [0, 1]
    c = rod_context(gpu_lib, V, seg, solver, bend=bend, held=held, r=0.01, E=1e8, dt=dt)
    c.set_surface(NO_SF, seg)
    c.set_rel_tol(1e-4)
    c.precompute()
    lowest = 0.0
    for step in range(steps):
        c.begin_timestep()
        E = c.state()["E"]
        for it in range(100):
            if c.newton_iter():
                break
            E1 = c.state()["E"]
            assert np.isfinite(E1) and E1 <= E, (step, it, E, E1)  # the line search never accepts an increase
            E = E1
        else:
            raise AssertionError("no convergence in 100 iterations")
        c.end_timestep()
        X = c.state()["V"]
        assert np.all(np.isfinite(X)) and np.all(X[held] == V[held])
        lowest = max(lowest, V[-1, 1] - X[-1, 1])
    return V, X, lowest


@pytest.mark.parametrize("solver", SOLVERS)
def test_cantilever_sags_less_with_more_bending_stiffness_and_hangs_without(gpu_lib, solver):
    V, X1, _ = _cantilever(gpu_lib, solver, 1.0)
    _, X10, _ = _cantilever(gpu_lib, solver, 10.0)
    d1, d10 = V[-1, 1] - X1[-1, 1], V[-1, 1] - X10[-1, 1]
    # bend 0: a chain of pendulums 0.45 long about the second held node; a rigid rod of that length released level reaches the vertical after 0.33 s
    # (1.18 x a quarter of 2 pi sqrt(2 L / (3 g))): within 0.6 s the tip has been at least 0.6 of the free length below the clamp (measured: 0.448, it hangs)
    _, X0, low0 = _cantilever(gpu_lib, solver, 0.0, steps=30, dt=0.02)
    print(f"solver {solver}: tip deflection bend 1: {d1:.6g}, bend 10: {d10:.6g}; bend 0: lowest tip {low0:.4g} below the clamp")
    assert 0.0 < d10 < d1 < 0.1
    assert low0 >= 0.6 * 0.45


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("friction", (0.0, 0.3))
def test_rod_dropped_across_a_block_and_a_plane_ends_without_intersection(gpu_lib, solver, friction):
    """A rod 0.5 long 0.01 above a held block 0.2 x 0.04 x 0.2 (top at 0.045) over the plane y = 0, self-contact on: the block catches its middle, the
    overhanging ends droop towards the plane.  Every step ends without intersection and above the plane; the block has stopped the middle."""
    P, T = five_tet_cube(np.array([0.2, 0.04, 0.2]), np.array([0.15, 0.005, -0.35]))
    Vr, seg = rmp.chain(11, spacing=0.05, origin=(0.0, 0.055, -0.27))
    V = np.vstack([P, Vr])
    seg = seg + len(P)
    c = rod_context(gpu_lib, V, seg, solver, T=T, held=np.arange(len(P)))
    c.set_components([len(P), len(V)], [len(T), len(T)])
    c.set_surface(scene.surface_tris(T), seg)
    c.enable_self_collision(1e-3)
    plane = c.add_half_space((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1e-3)
    if friction > 0:
        c.set_friction(friction, 1, 1e-3)
        c.set_half_space_friction(plane, friction)
    c.precompute()
    touched = 0
    for step in range(20):
        assert c.solve_timestep(200) < 200
        X = c.state()["V"]
        assert np.all(np.isfinite(X)) and not c.is_intersected() and X[:, 1].min() > 0.0
        st = c.contact_state()
        touched += st["nActive"] + st["nPara"] > 0
    mid = X[len(P) + 5, 1]
    print(f"solver {solver} friction {friction}: middle node {mid:.4f}, lowest rod node {X[len(P):, 1].min():.4f}, steps with mesh constraints {touched}")
    assert touched >= 3 and 0.045 < mid < 0.055  # the rod has fallen onto the block, and the block holds it


def test_nearly_folded_node_takes_a_step_with_finite_energies(gpu_lib):
    """A node folded to 170 degrees (d = |e0||e1| (1 + cos 170) = 0.015 |e0||e1|), straight at rest, no gravity: the bending energy pushes it open.  Every
    energy the line search accepts is finite and no higher than the one before; the fold has opened at the end of the step."""
    X = rmp.elbow(0)
    x = rmp.elbow(170, 0.1, 0.16)
    c = rod_context(gpu_lib, X, [[0, 1], [1, 2]], gravity=False, x0=x, r=0.01, E=1e6)
    c.set_surface(NO_SF, np.array([[0, 1], [1, 2]]))
    c.precompute()
    k0 = np.sqrt(rmp.curvature(rmp.NP, x.tolist())[0])
    c.begin_timestep()
    E = c.state()["E"]
    assert np.isfinite(E) and np.isfinite(c.rod_energy())
    for it in range(200):
        if c.newton_iter():
            break
        E1 = c.state()["E"]
        assert np.isfinite(E1) and E1 <= E, (it, E, E1)
        E = E1
    else:
        raise AssertionError("no convergence in 200 iterations")
    c.end_timestep()
    Xn = c.state()["V"]
    k1 = np.sqrt(rmp.curvature(rmp.NP, Xn.tolist())[0])
    print(f"|kb| {k0:.4g} -> {k1:.4g} in {it} iterations")
    assert np.all(np.isfinite(Xn)) and k1 < k0


def test_rod_beside_a_shell_and_tetrahedra_goes_through_the_patch_assembly(gpu_lib):
    """The Newton assembly of a five-tet block, a small cloth and a rod equals the sum of the entry points that build it term by term: mass diagonal +
    tet-parallel elastic Hessian + shell Hessian + rod Hessian, and the same for the gradient (different summation orders: 64 u of the largest entry)."""
    import shell_mp as smp
    P, T = five_tet_cube(0.2, np.array([0.0, -1.0, 0.0]))
    Vg, tri = smp.grid(5, spacing=0.05)
    Vr, seg = rmp.chain(40, spacing=0.02, origin=(0.0, 0.5, 0.0))
    V = np.vstack([P, Vg + [0.0, 0.0, 1.0], Vr])
    tri, seg = tri + len(P), seg + len(P) + len(Vg)
    x = V + 1e-3 * np.random.default_rng(5).standard_normal(V.shape)
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=YM, PR=0.4, density=RHO)
    c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
    c.set_rod(seg, R, YM, RHO)
    c.set_positions(x)
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_xtilde(x)
    coef = 1e-4
    g = c.assemble_newton(coef, True)
    a = c.get_a()
    ia = c.get_pattern()[0]
    gsum = c.rod_gradient_add(coef, True, c.shell_gradient_add(coef, True, c.elastic_gradient(coef, True)))
    c.set_zero()
    c.elastic_hessian_add(coef, True)
    c.shell_hessian_add(coef, True)
    rodOnly = c.get_a()
    c.rod_hessian_add(coef, True)
    b = c.get_a()
    assert np.abs(b - rodOnly).max() > 0.0  # the rod adds something
    m = np.repeat(c.features()["mass"], 3)
    b[ia[:-1]] += m  # every upper-CSR row starts with its diagonal
    assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 64 * rmp.U * np.abs(b).max()
    assert np.abs(g - gsum).max() <= 64 * rmp.U * np.abs(gsum).max()
    c2 = gpu_lib.Context(0)
    c2.set_mesh(V, T)
    c2.set_rod(seg, R, YM, RHO)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*belongs to a rod"):  # the converse of set_rod's own check
        c2.set_shell(np.array([[seg[0, 0], tri[0, 0], tri[0, 1]]]), 1e-3, 1e5, 0.3, RHO)


def test_error_paths(gpu_lib):
    V, seg = rmp.chain(4)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shard(0, 2)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_rod(seg, R, YM, RHO)
    c = rod_context(gpu_lib, V, seg)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.system_report()
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3"):
        c.set_rod(seg, R, YM, RHO)  # after opt_init
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    for r, E, rho, word in ((0.0, YM, RHO, "radius > 0"), (-R, YM, RHO, "radius > 0"), (R, 0.0, RHO, "E > 0"), (R, YM, -1.0, "rho > 0")):
        c = gpu_lib.Context(0)
        c.set_mesh(V, NO_T)
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*" + word):
            c.set_rod(seg, r, E, rho)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1"):
        c.set_rod(seg, R, YM, RHO, bend_scale=-1.0)
    P, T = five_tet_cube(0.2, np.array([0.0, -1.0, 0.0]))
    c = gpu_lib.Context(0)
    c.set_mesh(np.vstack([P, V]), T)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*belongs to a tetrahedron"):
        c.set_rod(np.array([[0, 8], [8, 9]]), R, YM, RHO)
    Vt = np.vstack([V, [[0.0, 1.0, 0.0]]])
    c = gpu_lib.Context(0)
    c.set_mesh(Vt, NO_T)
    c.set_shell(np.array([[0, 1, 4]]), 1e-3, 1e5, 0.3, RHO)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*belongs to a shell triangle"):
        c.set_rod(seg, R, YM, RHO)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*is repeated"):
        c.set_rod(np.array([[2, 3], [3, 2]]), R, YM, RHO)


def test_replacing_and_removing_a_rod_puts_the_masses_back(gpu_lib):
    V, seg = rmp.chain(6)
    codim = np.full(len(V), 0.125)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_codim_nodes(np.arange(len(V)), codim)
    lumped = lambda s, r: np.bincount(s.ravel(), minlength=len(V)) * RHO * np.pi * r * r * 0.1 / 2
    c.set_rod(seg, R, YM, RHO)
    assert np.allclose(c.features()["mass"], lumped(seg, R), rtol=1e-13, atol=0)
    part = seg[:2]  # replaced by a shorter, thicker one: the nodes it leaves out get their earlier masses back
    c.set_rod(part, 2 * R, YM, RHO)
    inPart = np.bincount(part.ravel(), minlength=len(V)) > 0
    assert not inPart.all() and c.rod_get()["nSeg"] == 2 and c.rod_get()["nBend"] == 1
    assert np.allclose(c.features()["mass"], np.where(inPart, lumped(part, 2 * R), codim), rtol=1e-13, atol=0)
    c.set_rod(np.zeros((0, 2), dtype=np.int32), R, YM, RHO)
    assert c.rod_get()["nSeg"] == 0 and c.rod_get()["nBend"] == 0 and np.array_equal(c.features()["mass"], codim)
    c.set_rod(seg, R, YM, RHO)
    c.set_mesh(V, NO_T)  # a new mesh drops the rod
    assert c.rod_get()["nSeg"] == 0


def test_pattern_built_before_set_rod_is_rebuilt(gpu_lib):
    V, seg = rmp.chain(5)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_surface(NO_SF, seg)
    c.set_pattern()  # the segments only: the outer pairs (a, c) of the bending triples are missing
    n0 = len(c.get_pattern()[1])
    c.set_rod(seg, R, YM, RHO)
    assert len(c.get_pattern()[1]) > n0
    c.opt_init(0.01, False)
    c.set_positions(V + 0.01 * np.random.default_rng(1).standard_normal(V.shape))
    c.rod_hessian_add(1.0, True)  # every block is there (IPCGPU_ERR_STATE otherwise)


def test_set_rod_with_no_segment_leaves_a_tet_and_shell_scene_bit_identical(gpu_lib):
    """Two contexts on a bar beside a one-triangle shell (one triangle, no hinge: every matrix entry receives one shell addend per kernel, so the atomic sums
    do not depend on an order), one of which calls set_rod with nSeg == 0: gradient, matrix values and the positions after a step agree to the bit."""
    Vb, Tb = scene.make_bar(3, 2, 2, size=(1.5, 1.0, 1.0))
    V = np.vstack([Vb, [[0.0, 3.0, 0.0], [0.3, 3.0, 0.0], [0.0, 3.0, 0.3]]])
    tri = np.array([[len(Vb), len(Vb) + 1, len(Vb) + 2]])
    x = V + 0.01 * np.random.default_rng(3).standard_normal(V.shape)
    out = []
    for with_call in (False, True):
        c = gpu_lib.Context(0)
        c.set_mesh(V, Tb)
        c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
        if with_call:
            c.set_rod(np.zeros((0, 2), dtype=np.int32), R, YM, RHO)
        c.set_positions(x)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(np.vstack([scene.surface_tris(Tb), tri]).astype(np.int32))
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        a = c.get_a()
        assert c.solve_timestep(100) < 100
        out.append((g, a, c.state()["V"], c.get_pattern()[0]))
        assert c.rod_get()["nSeg"] == 0 and c.rod_energy() == 0.0
        assert c.rod_energy_per_elem()[0].shape == (0,) and np.array_equal(c.rod_gradient_add(1.0, True), np.zeros(3 * len(V)))
    for p, q in zip(*out):
        assert np.array_equal(p, q)
