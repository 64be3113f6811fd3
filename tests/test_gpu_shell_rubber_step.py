"""The shells' rubber membrane in the time stepper: free fall, the patch test, a balloon under constant pressure (the discrete virial identity) and under the
gas law (the limit point, which the StVK membrane does not have), the guards against a degenerate rubber triangle, the error paths, removal, and rubber
with a strain limit.  Meshes of at most 642 nodes."""
import numpy as np
import pytest

import shell_mp as smp
import shell_rubber_mp as rmp
from chamber_gas_mp import icosphere
from codim_common import step_context

pytestmark = pytest.mark.gpu

NO_T = np.zeros((0, 4), dtype=np.int32)
G = 9.80665
# dyadic coordinates: the scripted move of the guard test lands exactly on a collinear state
ONE_V = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, -0.25]])
ONE_TRI = np.array([[0, 1, 2]], dtype=np.int32)


def iterate_bound(relTol, V, dt, k):
    """as tests/test_gpu_attach_step.py: an iterate lies within 2 relTol x (bounding-box diagonal) x dt of its step's minimiser, (k + 1)^2 of that after k steps"""
    return 2 * relTol * np.linalg.norm(V.max(0) - V.min(0)) * dt * (k + 1) ** 2


def context(gpu_lib, V, tri, E, h=1e-3, rho=1000.0, model=1, alpha=0.0, bend=1.0, limit=None, chambers=None, dt=0.01, gravity=True, held=None, x0=None, solver=0):
    def set_body(c):
        c.set_shell(tri, h, E, 0.3, rho, bend_scale=bend)
        if model is not None:
            c.set_shell_membrane(model, alpha)
        if limit is not None:
            c.set_shell_strain_limit(limit, 1.0, 1.0)
        if chambers is not None:
            c.set_chambers([tri], [chambers])
    return step_context(gpu_lib, V, set_body, solver, None, 1e7, 1000.0, dt, gravity, held, x0)


def test_free_fall_follows_the_discrete_recursion(gpu_lib):
    """No contact, no constraint: backward Euler gives v += dt g, y += dt v for every node (bound: 1e-9 of the fall distance, as test_gpu_shell_step.py).  A
    rigid translation leaves F at the identity: the rubber energy k1 ((tr + 1 / J) - 3) + k2 ((tr / J + J) - 3) is then a few roundings of 3, bounded here by
    16 u of its magnitude sum (the restatement's `scale`: every term by its magnitude)."""
    V, tri = smp.grid(4)
    V = V + [0.0, 1.0, 0.0]
    c = context(gpu_lib, V, tri, 1e5, alpha=0.25)
    c.set_surface(tri)
    c.set_rel_tol(1e-8)
    c.precompute()
    nt = len(tri)
    case = {"X": V, "x": V, "tri": tri, "h": np.full(nt, 1e-3), "YM": np.full(nt, 1e5), "alpha": np.full(nt, 0.25), "model": np.ones(nt, dtype=np.int32)}
    scaleE = float(rmp.patch_reference(rmp.NP, case, magnitudes=True)[0])
    dt, v, fall = 0.01, 0.0, 0.0
    for step in range(5):
        assert c.solve_timestep(50) < 50
        v += dt * G
        fall += dt * v
        X = c.state()["V"]
        print(f"step {step}: fall {fall:.6g}, worst deviation {np.abs(X - (V - [0, fall, 0])).max():.3g}, rubber energy {c.shell_rubber_energy():.3g} (scale {scaleE:.3g})")
        assert np.all(np.abs(X - (V - [0.0, fall, 0.0])) <= 1e-9 * fall)
        assert abs(c.shell_rubber_energy()) <= 16 * rmp.U * scaleE


def test_patch_test_affine_biaxial_stretch(gpu_lib):
    """A 5 x 5 sheet, every boundary node Dirichlet at the affine stretch (1.5, 1.2), the interior perturbed in and out of the plane.  The affine state is the
    discrete equilibrium (constant stress, interior forces cancel); the sheet is light (rho 10, dt 1: inertia m / dt^2 = 1e-7 against mu h = 33, so each step
    is static to 3e-9 of what is left of the perturbation).  After 3 steps the interior lies within e = iterate_bound of the affine positions, and the rubber
    energy equals h A psi(1.5, 1.2) to first order in the strain error 2 e / spacing: (dpsi/dl1 + dpsi/dl2) / psi = 4.5 at (1.5, 1.2), so 8 x that strain."""
    V, tri = smp.grid(5)
    rng = np.random.default_rng(3)
    affine = V * [1.5, 1.2, 1.0]
    boundary = np.flatnonzero((V[:, 0] == 0) | (V[:, 1] == 0) | (V[:, 0] == V[:, 0].max()) | (V[:, 1] == V[:, 1].max()))
    interior = np.setdiff1d(np.arange(len(V)), boundary)
    assert len(interior) == 9
    x0 = affine.copy()
    x0[interior] += 0.01 * rng.standard_normal((9, 3))
    relTol, dt, steps, h, E, alpha = 1e-8, 1.0, 3, 1e-3, 1e5, 0.1
    c = context(gpu_lib, V, tri, E, h=h, rho=10.0, alpha=alpha, dt=dt, gravity=False, held=boundary, x0=x0)
    c.set_surface(tri)
    c.set_rel_tol(relTol)
    c.precompute()
    for _ in range(steps):
        assert c.solve_timestep(100) < 100
    X = c.state()["V"]
    e = iterate_bound(relTol, affine, dt, steps)
    area = 0.4 * 0.4
    want = h * area * float(rmp.psi_principal(1.5, 1.2, E / 3, alpha))
    got = c.shell_rubber_energy()
    strain = 2 * e / 0.1
    print(f"worst deviation from the affine state {np.abs(X - affine).max():.3g} (bound {e:.3g}); energy {got:.12g}, closed form {want:.12g}, "
          f"relative error {abs(got - want) / want:.3g} (bound {8 * strain:.3g})")
    assert np.all(X[boundary] == affine[boundary])
    assert np.all(np.abs(X - affine) <= e)
    assert abs(got - want) <= 8 * strain * want
    assert np.abs(c.shell_thickness() / h - 1 / 1.8).max() <= 4 * strain  # every triangle thinned by 1 / (1.5 x 1.2)


def inflate(gpu_lib, level, steps=8):
    """the all-rubber unit icosphere, `bend 0`, one chamber at p = 0.4 x 2 mu h / R, stepped to rest (dt 1: backward Euler damps the breathing mode,
    w = sqrt(E / rho) / R = 17 rad / s, by (w dt)^-2 per step) with stiffness damping on but for the last two steps; returns the context and the last three position sets"""
    V, tri = icosphere(level)
    E, h, rho = 3e5, 0.01, 1000.0
    mu = E / 3
    p = 0.4 * 2 * mu * h / 1.0
    c = context(gpu_lib, V, tri, E, h=h, rho=rho, alpha=0.0, bend=0.0, chambers=p, dt=1.0, gravity=False)
    c.set_surface(tri)
    c.set_damping(0.1)
    c.set_rel_tol(1e-8)
    c.precompute()
    hist = [V.copy()]
    its = []
    for k in range(steps):
        if k == steps - 2:
            c.set_damping(0.0)  # the last two steps without it: the residual of the state they end in is that of W - p V and the inertia alone
        its.append(c.solve_timestep(300))
        assert its[-1] < 300
        hist.append(c.state()["V"].copy())
    return c, hist[-3:], dict(mu=mu, h=h, p=p, rho=rho, tri=tri, V=V, its=its)


def radius_root(q):
    a, b = 1.0, 7.0 ** (1.0 / 6.0)  # lambda^-1 - lambda^-7 rises from 0 to its maximum 0.62 on this interval
    f = lambda l: 1 / l - l ** -7 - q
    for _ in range(200):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if f(mid) < 0 else (a, mid)
    return 0.5 * (a + b)


@pytest.fixture(scope="module")
def balloons(gpu_lib):
    return {level: inflate(gpu_lib, level) for level in (2, 3)}


def test_balloon_at_constant_pressure_meets_the_discrete_virial_identity(balloons):
    """At a discrete equilibrium sum_v x_v . (grad W - p grad V) = 0.  Scaling x -> s x scales both stretches of every triangle by s and V by s^3, so
    x . grad W = d/ds W(s x) = sum_t h A_t mu (s1^2 + s2^2 - 2 (s1 s2)^-2) (neo-Hookean, alpha = 0) and x . grad V = 3 V:  the two sides below.  The stretches
    come from ipcgpu_shell_stretch and V from ipcgpu_chamber_state, neither from the gradient kernel under test.  The state is not exactly an equilibrium:
    with the residual r = grad W - p grad V the two sides differ by x . r, |x . r| <= |x| |r|, x taken from the centroid (forces and grad V sum to zero);
    r = (g - M (x - xTilde)) / dt^2 with g the stepper's residual gradient (ipcgpu_opt_get_state) and xTilde = 2 x_n-1 - x_n-2 (backward Euler), plus 64 u
    of the sum of the magnitudes for the rounding of the two sums."""
    c, (x2, x1, x0), m = balloons[2]
    sigma, _ = c.shell_stretch()
    area = c.shell_get()["area"]
    lhs_terms = m["h"] * area * m["mu"] * (sigma[:, 0] ** 2 + sigma[:, 1] ** 2 - 2 * (sigma[:, 0] * sigma[:, 1]) ** -2.0)
    vol = c.chamber_state()[0][0]
    lhs, rhs = lhs_terms.sum(), 3 * m["p"] * vol
    st = c.state()
    mass = np.repeat(c.shell_get()["mass"], 3)
    dt = 1.0
    inertia = mass * (x0 - 2 * x1 + x2).ravel()
    r = (np.abs(st["gradient"]) + np.abs(inertia)) / dt ** 2
    xc = x0 - x0.mean(axis=0)
    tol = np.linalg.norm(xc) * np.linalg.norm(r) + 64 * rmp.U * (np.abs(lhs_terms).sum() + abs(rhs))
    print(f"virial: sum h A mu (s1^2 + s2^2 - 2 / (s1 s2)^2) = {lhs:.12g}, 3 p V = {rhs:.12g}, difference {abs(lhs - rhs):.3g} (tolerance {tol:.3g}; "
          f"|g| {np.linalg.norm(st['gradient']):.3g}, |inertia| {np.linalg.norm(inertia):.3g}); Newton iterations per step {m['its']}")
    assert lhs > 0 and abs(lhs - rhs) <= tol
    assert tol <= 1e-4 * rhs  # the run did come to rest: the identity is tested, not the tolerance


def test_balloon_radius_converges_to_the_membrane_solution(balloons):
    """p R / (2 mu h) = lambda^-1 - lambda^-7 for the neo-Hookean spherical membrane.  The faceted sphere deviates (its area and volume are below the
    sphere's); no bound for that error is at hand, so the test asserts only that level 3 is closer than level 2.  Measured: DESIGN.md."""
    lam = radius_root(0.4)
    dev = {}
    for level, (c, (x2, x1, x0), m) in balloons.items():
        ratio = np.linalg.norm(x0 - x0.mean(axis=0), axis=1).mean() / np.linalg.norm(m["V"], axis=1).mean()
        dev[level] = abs(ratio - lam)
        print(f"level {level}: mean radius ratio {ratio:.6f}, membrane solution {lam:.6f}, deviation {dev[level]:.3g}, Newton iterations per step {m['its']}")
    assert dev[3] < dev[2]
    assert dev[2] < 0.05  # (the balloon did inflate to the neighbourhood of the solution, 1.10: not a comparison of two wrong states)


def gas_sequence(gpu_lib, model):
    """the level-2 sphere as an ideal-gas chamber (isothermal, ambient 1e5 against 2 mu h / R = 2e3: nearly volume control, which is stable past the limit
    point), fillVolume raised so that the radius stretch goes 1 -> 2 in 12 quasi-static steps of two time steps each; returns the gauge pressures"""
    V, tri = icosphere(2)
    E, h = 3e5, 0.01
    c = context(gpu_lib, V, tri, E, h=h, alpha=0.0, bend=0.0, model=model, chambers=0.0, dt=1.0, gravity=False)
    c.set_surface(tri)
    c.set_damping(0.1)
    c.set_rel_tol(1e-6)
    v0 = c.chamber_get()["restVolume"][0]
    c.chamber_set_gas(True, ambient=1e5, gamma=1.0, fill_volume=v0)
    c.precompute()
    gauge, lam = [], []
    for k in range(1, 13):
        c.chamber_set_gas(True, ambient=1e5, gamma=1.0, fill_volume=v0 * (1 + k / 12.0) ** 3)
        for _ in range(2):
            assert c.solve_timestep(300) < 300
        vol, g, _ = c.chamber_gas_state()
        gauge.append(g[0])
        lam.append((vol[0] / v0) ** (1.0 / 3.0))
    return np.array(gauge), np.array(lam)


def test_limit_point_rubber_pressure_rises_then_falls_stvk_rises_throughout(gpu_lib):
    rub, lam = gas_sequence(gpu_lib, 1)
    stvk, lam0 = gas_sequence(gpu_lib, None)
    unit = 2 * 1e5 * 0.01
    print("stretch      " + " ".join(f"{v:7.3f}" for v in lam))
    print("rubber gauge " + " ".join(f"{v / unit:7.4f}" for v in rub) + "  (in 2 mu h / R)")
    print("StVK gauge   " + " ".join(f"{v / unit:7.4f}" for v in stvk))
    k = int(np.argmax(rub))
    assert 0 < k < len(rub) - 1 and np.all(np.diff(rub[:k + 1]) > 0) and np.all(np.diff(rub[k:]) < 0)  # rises, then falls
    assert 1.2 < lam[k] < 1.6 and lam[-1] > 1.9  # the maximum near 7^(1/6) = 1.383; the run goes on to a stretch of 2
    assert 0.5 < rub[k] / unit < 0.7  # the membrane solution's maximum is 0.62
    assert np.all(np.diff(stvk) > 0) and stvk[-1] > 5 * rub[-1]  # the cloth law has no limit point


def test_scripted_move_that_would_flatten_a_triangle_is_shortened(gpu_lib):
    """One light free triangle (rho 10), no gravity, its third node scripted by 0.25 in one step -- alone, that puts it exactly on the first node (dyadic
    coordinates: det C = 0, energy +infinity).  The scripted move is shortened (the state after begin_timestep is feasible, the node short of its target),
    and the solve then takes the node the rest of the way while the free nodes give way: the triangle ends translated, never degenerate."""
    dt, d = 0.25, 0.25
    c = context(gpu_lib, ONE_V, ONE_TRI, 1e5, rho=10.0, alpha=0.1, dt=dt, gravity=False)
    c.add_dirichlet(np.array([2], dtype=np.int32), lin_vel=(0.0, 0.0, d / dt))
    c.set_surface(ONE_TRI)
    c.precompute()
    c.begin_timestep()
    st = c.state()
    print(f"after the scripted move: node 2 at z = {st['V'][2, 2]}, energy {st['E']:.6g}, rubber energy {c.shell_rubber_energy():.6g}")
    assert np.isfinite(st["E"]) and np.isfinite(c.shell_rubber_energy())
    assert -0.25 < st["V"][2, 2] < 0.0  # moved, but not all the way
    for it in range(300):
        done = c.newton_iter()
        assert np.isfinite(c.state()["E"]) and np.isfinite(c.shell_rubber_energy())
        if done:
            break
    else:
        raise AssertionError("no convergence in 300 iterations")
    c.end_timestep()
    X = c.state()["V"]
    sigma, _ = c.shell_stretch()
    print(f"at the end of the step: node 2 at {X[2]}, stretches {sigma[0]}")
    assert np.all(np.abs(X[2] - [0.0, 0.0, 0.0]) <= 2e-3 * d)  # the stepper's own completion tolerance: 1e-3 of the move
    assert sigma[0, 1] > 0.5


def test_step_from_a_collinear_rubber_triangle_is_refused_and_changes_nothing(gpu_lib):
    x0 = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.125, 0.0, 0.0]])
    c = context(gpu_lib, ONE_V, ONE_TRI, 1e5, x0=x0)
    c.set_surface(ONE_TRI)
    c.precompute()
    assert c.shell_rubber_energy() == np.inf
    for call in (lambda: c.solve_timestep(10), c.begin_timestep):
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3: 1 rubber triangle is degenerate"):
            call()
        assert np.array_equal(c.state()["V"], x0)
    # positions written between two steps are looked at once, too
    c = context(gpu_lib, ONE_V, ONE_TRI, 1e5)
    c.set_surface(ONE_TRI)
    c.precompute()
    assert c.solve_timestep(50) < 50
    c.set_positions(x0)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3: 1 rubber triangle"):
        c.solve_timestep(10)
    assert np.array_equal(c.state()["V"], x0)


def test_error_paths(gpu_lib):
    c = gpu_lib.Context(0)
    c.set_mesh(ONE_V, NO_T)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*no shell"):
        c.set_shell_membrane(1)
    c.set_shell(ONE_TRI, 1e-3, 1e5, 0.3, 1000.0)
    assert c.shell_thickness()[0] == 1e-3
    for model, alpha, word in ((2, None, "model other than 0"), (-1, None, "model other than 0"), (1, 1.0, "alpha outside"), (1, -0.1, "alpha outside"),
                               (1, 1.5, "alpha outside"), (1, np.nan, "not finite"), (1, np.inf, "not finite")):
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*" + word):
            c.set_shell_membrane(model, alpha)
        assert not c.shell_membrane_get()[0].any()  # a refused call sets nothing
    c.set_shell_membrane(0, np.nan)  # alpha of a StVK triangle is not read
    c.set_shell_membrane(1, 0.5)
    m, a = c.shell_membrane_get()
    assert m.tolist() == [1] and a.tolist() == [0.5]
    c.opt_init(0.01, False)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*positive"):
        c.shell_rubber_energy(-1.0)
    c.set_positions(ONE_V * 2.0)
    assert c.shell_thickness()[0] == pytest.approx(0.25e-3, rel=1e-14)


def test_removal_and_all_zero_models_leave_the_run_bit_identical(gpu_lib):
    """A membrane model set and removed again (zeros, then None), and one that was all zero from the start, leave the run bit-identical to a context that never
    made the call (one triangle: no atomic order); ipcgpu_set_shell drops the term."""
    out = []
    for how in ("never", "all zero", "zeros", "none"):
        c = gpu_lib.Context(0)
        c.set_mesh(ONE_V, NO_T)
        c.set_shell(ONE_TRI, 1e-3, 1e5, 0.3, 1000.0)
        if how == "all zero":
            c.set_shell_membrane(np.zeros(1, dtype=np.int32), 0.3)
        elif how != "never":
            c.set_shell_membrane(1, 0.3)
            assert c.shell_membrane_get()[0].tolist() == [1]
            c.set_shell_membrane(np.zeros(1, dtype=np.int32) if how == "zeros" else None)
        assert c.shell_membrane_get()[0].tolist() == [0] and c.shell_membrane_get()[1].tolist() == [0.0]
        c.set_positions(ONE_V * 1.2)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(ONE_TRI)
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        E = c.shell_energy()
        for _ in range(3):
            assert c.solve_timestep(100) < 100
        assert c.shell_rubber_energy() == 0.0 and not c.shell_rubber_gradient_add().any() and not c.shell_rubber_energy_per_elem().any()
        out.append((g, E, c.state()["V"]))
    assert out[0][1] > 0.0  # the StVK membrane is back
    for g, E, X in out[1:]:
        assert np.array_equal(g, out[0][0]) and E == out[0][1] and np.array_equal(X, out[0][2])
    c = gpu_lib.Context(0)
    c.set_mesh(ONE_V, NO_T)
    c.set_shell(ONE_TRI, 1e-3, 1e5, 0.3, 1000.0)
    c.set_shell_membrane(1)
    c.set_shell(ONE_TRI, 2e-3, 1e5, 0.3, 1000.0)
    assert c.shell_membrane_get()[0].tolist() == [0]
    c.set_positions(ONE_V * 1.2)
    c.opt_init(0.01, False)
    assert c.shell_rubber_energy() == 0.0 and c.shell_energy_per_elem()[0][0] > 0.0  # StVK again, with its constants
    c.set_shell_membrane(1)
    c.set_mesh(ONE_V, NO_T)  # a new mesh drops the shell and its membrane model
    assert c.shell_membrane_get()[0].shape == (0,)


def test_rubber_with_a_strain_limit_on_the_same_triangles(gpu_lib):
    """The hanging 3 x 9 strip of test_gpu_shell_limit_step.py, soft (E = 5e3: without a limit the top row stretches far past 1.1), all rubber, `limit 1.1`:
    every accepted iterate is finite and below the limit, and the strip ends stretched between 1.0 and 1.1"""
    Vg, tri = smp.grid(3, 9)
    V = np.column_stack([Vg[:, 0], 1.0 - Vg[:, 1], np.zeros(len(Vg))])
    c = context(gpu_lib, V, tri, 5e3, alpha=0.1, limit=1.1, dt=0.02, held=np.arange(3))
    c.set_surface(tri)
    c.set_rel_tol(1e-4)
    c.precompute()
    worst = 0.0
    for step in range(15):
        c.begin_timestep()
        for it in range(300):
            done = c.newton_iter()
            E, ratio = c.state()["E"], c.shell_stretch()[1]
            worst = max(worst, ratio)
            assert np.isfinite(E) and ratio < 1.0, (step, it, E, ratio)
            if done:
                break
        else:
            raise AssertionError(f"no convergence (step {step})")
        c.end_timestep()
    sigma, ratio = c.shell_stretch()
    print(f"largest stretch at the end {sigma[:, 0].max():.4f}, largest sigma1 / limit over the run {worst:.4f}; limit energy {c.shell_limit_energy():.3g}, "
          f"rubber energy {c.shell_rubber_energy():.3g}")
    assert 1.0 < sigma[:, 0].max() < 1.1 and c.shell_limit_energy() > 0.0 and c.shell_rubber_energy() > 0.0
    assert c.shell_thickness().min() < 1e-3  # stretched rubber thins
