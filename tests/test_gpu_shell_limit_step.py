"""The shells' strain limit in the time stepper: a hanging strip with and without it, a limit that is never reached, a drop onto a block and a plane with
contact and friction, a scripted pull that has to be shortened, an over-stretched start, the error paths, removal and replacement, and the patch assembly
beside tetrahedra and a rod.  Meshes of at most about 100 nodes."""
import numpy as np
import pytest

import rod_mp as rmp
import shell_limit_mp as lmp
import shell_mp as smp
from codim_common import five_tet_cube, step_context
from ipc_amd import scene

pytestmark = pytest.mark.gpu

H, PR = 1e-3, 0.3
NO_T = np.zeros((0, 4), dtype=np.int32)
ONE_V = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.0, -0.3]])
ONE_TRI = np.array([[0, 1, 2]], dtype=np.int32)


def context(gpu_lib, V, tri, E, rho=1000.0, limit=None, onset=None, stiff=None, T=None, dt=0.01, gravity=True, held=None, x0=None, solver=0):
    def set_body(c):
        c.set_shell(tri, H, E, PR, rho)
        if limit is not None:
            c.set_shell_strain_limit(limit, onset, stiff)
    return step_context(gpu_lib, V, set_body, solver, T, 1e7, 1000.0, dt, gravity, held, x0)


def hanging_strip():
    """3 x 9 nodes in the plane z = 0, 0.2 wide, 0.8 long, hanging down from its top row"""
    V, tri = smp.grid(3, 9)
    return np.column_stack([V[:, 0], 1.0 - V[:, 1], np.zeros(len(V))]), tri, np.arange(3)


def steps_checked(c, n, limited, max_iter=300, monotone=True):
    """n time steps, iteration by iteration: every accepted energy is finite and no higher than the one before (monotone=False: finite only -- while the
    augmented-Lagrangian solve of an unfinished Dirichlet move runs, the stepper changes the penalty weight and the multipliers between two iterations, and
    with them the function the energies belong to); with a limit, the largest stretch stays below it after every Newton iteration.  Returns the largest
    sigma1 / limit seen (0 without a limit)."""
    worst = 0.0
    for step in range(n):
        c.begin_timestep()
        E = c.state()["E"]
        assert np.isfinite(E)
        if limited:
            worst = max(worst, c.shell_stretch()[1])
            assert worst < 1.0
        for it in range(max_iter):
            if c.newton_iter():
                break
            E1 = c.state()["E"]
            assert np.isfinite(E1) and (E1 <= E or not monotone), (step, it, E, E1)
            E = E1
            if limited:
                worst = max(worst, c.shell_stretch()[1])
                assert worst < 1.0, (step, it, worst)
        else:
            raise AssertionError(f"no convergence in {max_iter} iterations (step {step})")
        c.end_timestep()
        assert np.all(np.isfinite(c.state()["V"]))
    return worst


def test_hanging_strip_stretches_past_1_3_without_the_limit_and_stays_below_1_1_with_it(gpu_lib):
    """E = 5e3: the top row carries rho g L = 7.8 kPa; St. Venant-Kirchhoff in uniaxial tension gives sigma (sigma^2 - 1) = 2 rho g L / E = 3.1, a static
    stretch of 1.7 at the top, reached (and overshot) after a quarter of the first longitudinal period 4 L / sqrt(E / rho) = 1.4 s: 30 steps of 0.02 s.  The
    same run with `limit 1.1 onset 1.0`: the barrier is infinite at 1.1, so the strip ends between 1.0 and 1.1, and no iterate ever reaches the limit.  Measured: 1.713 without the limit;
    1.020 with it (k b' balances the 1.57 E of weight at y = 0.2 of the range), the largest sigma1 / limit over all iterates 0.931."""
    V, tri, held = hanging_strip()
    out = {}
    for limit in (None, 1.1):
        c = context(gpu_lib, V, tri, 5e3, limit=limit, onset=None if limit is None else 1.0, dt=0.02, held=held)
        c.set_surface(tri)
        c.set_rel_tol(1e-4)
        c.precompute()
        worst = steps_checked(c, 30, limit is not None)
        sigma, ratio = c.shell_stretch()
        out[limit] = sigma[:, 0].max()
        print(f"limit {limit}: largest stretch at the end {sigma[:, 0].max():.4f}, largest sigma1 / limit over the run {worst:.4f}, at the end {ratio:.4f}, "
              f"lowest node {c.state()['V'][:, 1].min():.4f}")
        if limit is None:
            assert ratio == 0.0
        else:
            assert ratio == sigma[:, 0].max() / 1.1
    assert out[None] > 1.3
    assert 1.0 < out[1.1] < 1.1


def test_limit_never_reached_leaves_the_run_bit_identical(gpu_lib):
    """One triangle (one lane per kernel, no hinge: every sum has one shell addend, so nothing depends on the order of the atomics), released from a stretch
    of 1.2 under gravity; with the limit at 10 (onset 9) the barrier adds exact zeros and writes nothing: the positions after 5 steps agree to the bit."""
    out = []
    for limit in (None, 10.0):
        c = context(gpu_lib, ONE_V, ONE_TRI, 1e5, limit=limit, onset=None if limit is None else 9.0, x0=ONE_V * 1.2)
        c.set_surface(ONE_TRI)
        c.precompute()
        for _ in range(5):
            assert c.solve_timestep(100) < 100
        out.append(c.state()["V"])
        if limit:
            assert c.shell_limit_energy() == 0.0 and 0.0 < c.shell_stretch()[1] < 0.2
    assert np.array_equal(out[0], out[1]) and np.abs(out[0] - ONE_V * 1.2).max() > 1e-3


def test_strip_dropped_onto_a_block_and_a_plane_stays_feasible(gpu_lib):
    """The 3 x 9 strip, soft (E = 2e4), 0.01 above a held block 0.2 x 0.04 x 0.2 over the plane y = 0, contact and friction on: the block catches its middle,
    the ends hang over and pull.  Every step ends feasible (sigma1 < limit everywhere), without intersection, above the plane and finite."""
    P, T = five_tet_cube(np.array([0.2, 0.04, 0.2]), np.array([0.3, 0.005, -0.2]))
    Vg, tri = smp.grid(9, 3)
    Vs = np.column_stack([Vg[:, 0], np.full(len(Vg), 0.055), -Vg[:, 1]])  # x 0 .. 0.8, z 0 .. -0.2: the block under its middle
    V = np.vstack([P, Vs])
    tri = tri + len(P)
    c = context(gpu_lib, V, tri, 2e4, limit=1.1, onset=1.0, T=T, held=np.arange(len(P)))
    c.set_components([len(P), len(V)], [len(T), len(T)])
    c.set_surface(np.vstack([scene.surface_tris(T), tri]).astype(np.int32))
    c.enable_self_collision(1e-3)
    plane = c.add_half_space((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1e-3)
    c.set_friction(0.3, 1, 1e-3)
    c.set_half_space_friction(plane, 0.3)
    c.precompute()
    touched, worst = 0, 0.0
    for step in range(18):
        assert c.solve_timestep(300) < 300
        X = c.state()["V"]
        sigma, ratio = c.shell_stretch()
        worst = max(worst, ratio)
        assert np.all(np.isfinite(X)) and ratio < 1.0 and not c.is_intersected() and X[:, 1].min() > 0.0
        st = c.contact_state()
        touched += st["nActive"] + st["nPara"] + st["nHalfSpace"] > 0
    print(f"largest sigma1 / limit {worst:.4f}, steps with constraints {touched}, lowest strip node {X[len(P):, 1].min():.4f}")
    assert touched >= 3


def test_scripted_pull_is_shortened_and_completed(gpu_lib):
    """A 5 x 2 strip (0.4 x 0.1), light (rho = 10: inertia m / dt^2 is a hundredth of E h, the steps are quasi-static), no gravity; the left column held, the two
    nodes of the right column scripted outwards by 0.015 per step.  Moved alone, they stretch the last column of triangles to 1.15 -- over the limit 1.1 --
    while the state the step ends in is a uniform 1.0375 (then 1.075): the scripted move is shortened, the penalty solve takes the nodes the rest of the way."""
    V, tri = smp.grid(5, 2)
    left, right = np.flatnonzero(V[:, 0] == 0.0), np.flatnonzero(V[:, 0] == V[:, 0].max())
    assert len(left) == 2 and len(right) == 2
    dt, d = 0.02, 0.015
    moved = V.copy()
    moved[right, 0] += d
    alone = lmp.singular_values(lmp.NP, {"X": V, "x": moved, "tri": tri})
    assert max(s[0] for s in alone) > 1.1 and (V[right[0], 0] + 2 * d) / V[right[0], 0] < 1.1  # one unshortened move crosses the limit, the target does not
    c = context(gpu_lib, V, tri, 1e5, rho=10.0, limit=1.1, onset=1.0, dt=dt, gravity=False, held=left)
    c.add_dirichlet(right, lin_vel=(d / dt, 0.0, 0.0))
    c.set_surface(tri)
    c.precompute()
    for step in (1, 2):
        worst = steps_checked(c, 1, True, monotone=False)
        X = c.state()["V"]
        sigma, ratio = c.shell_stretch()
        print(f"step {step}: scripted nodes at {X[right, 0]}, target {V[right[0], 0] + step * d}, largest sigma1 / limit over the step {worst:.4f}, "
              f"stretch at the end {sigma[:, 0].min():.4f} .. {sigma[:, 0].max():.4f}")
        assert np.all(np.abs(X[right] - (V[right] + [step * d, 0.0, 0.0])) <= 2e-3 * d)  # the stepper's own completion tolerance: 1e-3 of the move
        assert np.all(X[left] == V[left]) and ratio < 1.0
    assert sigma[:, 0].max() > 1.05


def test_over_stretched_start_is_refused_and_changes_nothing(gpu_lib):
    x0 = ONE_V * [1.3, 1.0, 1.0]
    c = context(gpu_lib, ONE_V, ONE_TRI, 1e5, limit=1.2, onset=1.0, x0=x0)
    c.set_surface(ONE_TRI)
    c.precompute()
    assert c.shell_stretch()[1] >= 1.0 and c.shell_limit_energy() == np.inf
    for call in (lambda: c.solve_timestep(10), c.begin_timestep):
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3: 1 shell triangle has a principal stretch at or over the strain limit"):
            call()
        assert np.array_equal(c.state()["V"], x0)
    # positions written between two steps are looked at once, too
    c = context(gpu_lib, ONE_V, ONE_TRI, 1e5, limit=1.2, onset=1.0)
    c.set_surface(ONE_TRI)
    c.precompute()
    assert c.solve_timestep(50) < 50
    c.set_positions(x0)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3: 1 shell triangle"):
        c.solve_timestep(10)
    assert np.array_equal(c.state()["V"], x0)


def test_error_paths(gpu_lib):
    c = gpu_lib.Context(0)
    c.set_mesh(ONE_V, NO_T)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*no shell"):
        c.set_shell_strain_limit(1.2)
    assert c.shell_stretch()[1] == 0.0 and c.shell_stretch()[0].shape == (0, 2)
    c.set_shell(ONE_TRI, H, 1e5, PR, 1000.0)
    for limit, onset, stiff, word in ((1.0, None, None, "not above its onset"), (1.2, 1.2, None, "not above its onset"), (1.2, 1.5, None, "not above its onset"),
                                      (1.2, 0.9, None, "onset below 1"), (1.2, None, 0.0, "stiff > 0"), (1.2, None, -1.0, "stiff > 0"), (-1.2, None, None, "negative"),
                                      (np.nan, None, None, "not finite"), (np.inf, None, None, "not finite"), (1.2, np.nan, None, "not finite"),
                                      (1.2, None, np.inf, "not finite")):
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*" + word):
            c.set_shell_strain_limit(limit, onset, stiff)
        assert c.shell_stretch()[1] == 0.0  # a refused call sets nothing
    c.set_shell_strain_limit(1.2)
    assert c.shell_stretch()[1] == pytest.approx(1.0 / 1.2, rel=1e-15)


def test_removing_the_limit_and_replacing_the_shell(gpu_lib):
    """A limit set and removed again (zeros, then None) leaves the run bit-identical to a context that never had one (one triangle: no atomic order);
    ipcgpu_set_shell drops the limit."""
    out = []
    for how in ("never", "zeros", "none"):
        c = gpu_lib.Context(0)
        c.set_mesh(ONE_V, NO_T)
        c.set_shell(ONE_TRI, H, 1e5, PR, 1000.0)
        if how != "never":
            c.set_shell_strain_limit(1.25, 1.0, 2.0)
            assert c.shell_stretch()[1] == pytest.approx(0.8, rel=1e-15)
            c.set_shell_strain_limit(np.zeros(1) if how == "zeros" else None)
            assert c.shell_stretch()[1] == 0.0
        c.set_positions(ONE_V * 1.2)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(ONE_TRI)
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        for _ in range(3):
            assert c.solve_timestep(100) < 100
        assert c.shell_limit_energy() == 0.0 and not c.shell_limit_gradient_add().any() and not c.shell_limit_energy_per_elem().any()
        out.append((g, c.state()["V"]))
    for g, X in out[1:]:
        assert np.array_equal(g, out[0][0]) and np.array_equal(X, out[0][1])
    c = gpu_lib.Context(0)
    c.set_mesh(ONE_V, NO_T)
    c.set_shell(ONE_TRI, H, 1e5, PR, 1000.0)
    c.set_shell_strain_limit(1.25)
    c.set_shell(ONE_TRI, 2 * H, 1e5, PR, 1000.0)
    assert c.shell_stretch()[1] == 0.0
    c.set_shell_strain_limit(1.25)
    c.set_mesh(ONE_V, NO_T)  # a new mesh drops the shell and its limit
    assert c.shell_stretch()[0].shape == (0, 2)


def test_limited_cloth_beside_tetrahedra_and_a_rod_goes_through_the_patch_assembly(gpu_lib):
    """The Newton assembly of a five-tet block, a cloth stretched into the barrier's range and a rod equals the sum of the entry points that build it term by
    term: mass diagonal + tet-parallel elastic Hessian + membrane and bending (taken with the limit removed) + the limit term + rod Hessian, and the same
    for the gradient (different summation orders: 64 u of the largest entry, as the rod's test)."""
    P, T = five_tet_cube(0.2, np.array([0.0, -1.0, 0.0]))
    Vg, tri = smp.grid(5, spacing=0.05)
    Vr, seg = rmp.chain(40, spacing=0.02, origin=(0.0, 0.5, 0.0))
    V = np.vstack([P, Vg + [0.0, 0.0, 1.0], Vr])
    tri, seg = tri + len(P), seg + len(P) + len(Vg)
    x = V + 1e-4 * np.random.default_rng(5).standard_normal(V.shape)  # (0.3 % of the cloth's spacing: stretches 1.06 +- 0.01)
    x[len(P):len(P) + len(Vg), 0] *= 1.06
    limit = np.where(np.arange(len(tri)) % 3 == 0, 0.0, 1.1)  # a third of the triangles unlimited
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=1e7, PR=0.4, density=1000.0)
    c.set_shell(tri, H, 1e5, PR, 1000.0)
    c.set_shell_strain_limit(limit, 1.0, 1.5)
    c.set_rod(seg, 2e-3, 1e7, 1000.0)
    c.set_positions(x)
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_xtilde(x)
    assert 0.9 < c.shell_stretch()[1] < 1.0
    coef = 1e-4
    g = c.assemble_newton(coef, True)
    a = c.get_a()
    ia = c.get_pattern()[0]
    c.set_shell_strain_limit(None)
    gsum = c.rod_gradient_add(coef, True, c.shell_gradient_add(coef, True, c.elastic_gradient(coef, True)))
    c.set_zero()
    c.elastic_hessian_add(coef, True)
    c.shell_hessian_add(coef, True)
    c.rod_hessian_add(coef, True)
    c.set_shell_strain_limit(limit, 1.0, 1.5)
    noLimit = c.get_a()
    gl = c.shell_limit_gradient_add(coef, True)
    c.shell_limit_hessian_add(coef, True)
    b = c.get_a()
    assert np.abs(b - noLimit).max() > 1e-3 * np.abs(noLimit).max() and np.abs(gl).max() > 1e-3 * np.abs(gsum).max()  # the limit adds something that counts
    gsum = gsum + gl
    b[ia[:-1]] += np.repeat(c.features()["mass"], 3)  # every upper-CSR row starts with its diagonal
    print(f"matrix {np.abs(a - b).max() / np.abs(b).max() / lmp.U:.3g} u, gradient {np.abs(g - gsum).max() / np.abs(gsum).max() / lmp.U:.3g} u of the largest entry")
    assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 64 * lmp.U * np.abs(b).max()
    assert np.abs(g - gsum).max() <= 64 * lmp.U * np.abs(gsum).max()
