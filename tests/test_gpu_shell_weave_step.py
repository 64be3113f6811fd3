"""The shells' woven cloth in the time stepper: the patch test with the warp along either axis, the soft bias, a cantilever that drapes by its yarn direction, the
run that a removed weave leaves bit-identical, what drops the term, the pairings that are refused and the argument errors.  Meshes of at most 52 nodes."""
import numpy as np
import pytest
from mpmath import mpf

import shell_mp as smp
import shell_weave_mp as wmp
from codim_common import step_context

pytestmark = pytest.mark.gpu

NO_T = np.zeros((0, 4), dtype=np.int32)
ONE_V = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, -0.25]])
ONE_TRI = np.array([[0, 1, 2]], dtype=np.int32)
FAB = dict(E1=1e5, E2=5e4, G12=2e3, nu12=0.25)


def context(gpu_lib, V, tri, d, fab=FAB, h=1e-3, E=1e5, rho=10.0, bend=0.0, bend_warp=None, bend_weft=None, dt=1.0, gravity=False, held=None, x0=None, weave=True):
    def set_body(c):
        c.set_shell(tri, h, E, 0.3, rho, bend_scale=bend)
        if weave:
            c.set_shell_weave(1, d, fab["E1"], fab["E2"], fab["G12"], fab["nu12"], bend_warp, bend_weft)
    c = step_context(gpu_lib, V, set_body, 0, None, 1e7, 1000.0, dt, gravity, held, x0)
    c.set_surface(tri)
    return c


def settle(c, steps, max_iter=200):
    for _ in range(steps):
        assert c.solve_timestep(max_iter) < max_iter


REL_TOL = 1e-8
PATCH_F = np.array([[1.05, 0.02, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])  # 5 % stretch along x, 2 % shear


def patch_run(gpu_lib, d):
    V, tri = smp.grid(7)  # 6 x 6 quads, 49 nodes, spacing 0.1
    affine = V @ PATCH_F.T
    boundary = np.flatnonzero((V[:, 0] == 0) | (V[:, 1] == 0) | (V[:, 0] == V[:, 0].max()) | (V[:, 1] == V[:, 1].max()))
    interior = np.setdiff1d(np.arange(len(V)), boundary)
    assert len(interior) == 25
    x0 = affine.copy()
    x0[interior] += 0.01 * 0.1 * np.random.default_rng(5).standard_normal((25, 3))  # 1 % of the edge length, in and out of the plane
    c = context(gpu_lib, V, tri, d, held=boundary, x0=x0)
    c.set_rel_tol(REL_TOL)
    c.precompute()
    settle(c, 3)
    return c, V, affine, boundary


def patch_psi(swap):
    """psi(G) of the patch in mpmath: G = (F^T F - I) / 2 with the warp along x, or (swap) along y -- which is the law with E1 and E2 swapped (and nu12 with
    nu21, so that C12 stays what it is) at the same G"""
    F = [[mpf("1.05"), mpf("0.02")], [mpf(0), mpf(1)]]
    G = [[(sum(F[k][i] * F[k][j] for k in range(2)) - (1 if i == j else 0)) / 2 for j in range(2)] for i in range(2)]
    E1, E2, G12, nu12 = (mpf(FAB[k]) for k in ("E1", "E2", "G12", "nu12"))
    along_y = wmp.psi(G[1][1], G[0][0], -G[0][1], wmp.moduli(E1, E2, G12, nu12))
    if swap:
        swapped = wmp.psi(G[0][0], G[1][1], G[0][1], wmp.moduli(E2, E1, G12, nu12 * E2 / E1))
        assert abs(along_y - swapped) <= mpf(10) ** -40 * swapped
        return float(along_y)
    return float(wmp.psi(G[0][0], G[1][1], G[0][1], wmp.moduli(E1, E2, G12, nu12)))


def test_patch_test_affine_stretch_and_shear_with_the_warp_along_either_axis(gpu_lib):
    """A 6 x 6-quad sheet (49 nodes, spacing 0.1), every boundary node Dirichlet on the affine map x = F X (5 % stretch along x, 2 % shear), the interior displaced
    by a seeded 1 % of the edge length.  The affine state is the discrete equilibrium (one fabric, one direction: constant stress, the interior forces cancel).
    Three static steps (dt = 1, rho 10, no gravity: the inertia m / dt^2 = 1e-7 per node stands against C22 h = 50).
    Allowed position error: the stepper stops when the largest entry of its Newton step falls below relTol x bounding-box diagonal x dt = 1e-8 x 0.849 x 1
    = 8.5e-9.  A step of that size leaves a force of at most the largest stiffness C11 h times it, which the softest direction, min(C22, G12) h = G12 h, turns
    into a position error of C11 / G12 = 51.6 times the step; times 10 for the crudeness of that conversion: e = 4.4e-6 (0.44 % of the initial displacement).
    Allowed energy error, first order in e: |delta G| <= |F| |delta F| with |delta F| <= 2 e / spacing and |F| <= 1.07, so |delta psi| <= (|s_ww| + |s_ff| + 2
    |s_wf|) 1.07 (2 e / 0.1); the stresses from the same restatement.  (The energy is stationary at the equilibrium, so this is generous.)
    Turning the direction by 90 degrees gives the law with E1 and E2 swapped (nu12 and nu21 with them) at the same G."""
    C = [float(v) for v in wmp.moduli(*(FAB[k] for k in ("E1", "E2", "G12", "nu12")))]
    h, area = 1e-3, 0.36
    energies = {}
    for name, d, swap in (("warp along x", (1.0, 0.0, 0.0), False), ("warp along y", (0.0, 1.0, 0.0), True)):
        c, V, affine, boundary = patch_run(gpu_lib, d)
        X = c.state()["V"]
        e = 10 * (C[0] / min(C[2], C[3])) * REL_TOL * np.linalg.norm(V.max(0) - V.min(0)) * 1.0
        psi = patch_psi(swap)
        want = h * area * psi
        G = 0.5 * (PATCH_F[:2, :2].T @ PATCH_F[:2, :2] - np.eye(2))
        Eww, Eff, Ewf = (G[1, 1], G[0, 0], G[0, 1]) if swap else (G[0, 0], G[1, 1], G[0, 1])
        stress = abs(C[0] * Eww + C[1] * Eff) + abs(C[1] * Eww + C[2] * Eff) + 2 * abs(2 * C[3] * Ewf)
        tolE = h * area * stress * 1.07 * (2 * e / 0.1)
        got = c.shell_energy()
        energies[name] = got
        print(f"{name}: worst deviation from the affine state {np.abs(X - affine).max():.3g} (bound {e:.3g}); energy {got:.12g}, h A psi(G) {want:.12g}, "
              f"error {abs(got - want):.3g} (bound {tolE:.3g})")
        assert abs(e - 4.4e-6) < 1e-7
        held = np.abs(X[boundary] - affine[boundary]).max()
        print(f"  largest movement of a held node {held:.3g}")
        assert held <= 16 * wmp.U  # (a fixed Dirichlet node is carried through the scripted rigid motion with zero velocity: a rounding of its coordinate per step)
        assert np.all(np.abs(X - affine) <= e)
        assert abs(got - want) <= tolE and tolE < 0.01 * want
        assert got == c.shell_weave_energy() and not c.shell_energy_per_elem()[0].any()  # the woven term is the whole membrane energy
        st = c.shell_weave_state()
        assert np.all(np.abs(st[:, 0] - Eww) <= 1.07 * 2 * e / 0.1) and np.all(np.abs(st[:, 1] - Eff) <= 1.07 * 2 * e / 0.1)
    assert energies["warp along x"] > 1.5 * energies["warp along y"]  # E1 = 2 E2: the pull along the warp costs more


def test_pull_on_the_bias_is_soft(gpu_lib):
    """A 12 x 3-quad strip (52 nodes) pulled 5 % between two clamped ends, E1 = E2, G12 = E1 / 100, nu12 = 0.  Uniaxial closed forms: E1 along the yarns,
    1 / E_45 = (2 / E1 + 1 / G12) / 4 = 1 / (3.9e-2 E1) on the bias: they differ by 25 x; the clamped ends stiffen the bias pull, the middle of the strip stays
    free.  An ordering, not a figure: the converged energy with the warp at 45 degrees is below half of that with the warp along the pull."""
    V, tri = smp.grid(13, 4)
    ends = np.flatnonzero((V[:, 0] == 0) | (V[:, 0] == V[:, 0].max()))
    fab = dict(E1=1e5, E2=1e5, G12=1e3, nu12=0.0)
    E = {}
    for name, d in (("along", (1.0, 0.0, 0.0)), ("bias", (1.0, 1.0, 0.0))):
        c = context(gpu_lib, V, tri, d, fab=fab, held=ends, x0=V * [1.05, 1.0, 1.0])
        c.set_rel_tol(REL_TOL)
        c.precompute()
        settle(c, 4)
        E[name] = c.shell_weave_energy()
        st = c.shell_weave_state()
        print(f"warp {name}: energy {E[name]:.6g}, largest shear angle {np.degrees(np.abs(st[:, 2]).max()):.3g} degrees")
    assert 0.0 < E["bias"] < 0.5 * E["along"]


def test_cantilever_cut_along_the_warp_droops_less(gpu_lib):
    """A 8 x 2-quad strip (27 nodes, 0.4 x 0.1) along x, its first two node columns held, under gravity, isotropic membrane moduli (so the cut changes the bending
    alone), `bendwarp 10 bendweft 1`.  The hinges that carry the droop lie across the strip: cut along the warp they curve the warp yarns (factor 10), cut
    along the weft the weft yarns (factor 1) -- the first droops strictly less at the tip."""
    Vg, tri = smp.grid(9, 3, spacing=0.05)
    V = np.column_stack([Vg[:, 0], np.zeros(len(Vg)), Vg[:, 1]])  # horizontal: gravity acts along -y
    held = np.flatnonzero(Vg[:, 0] <= 0.05 + 1e-12)
    tip = np.flatnonzero(Vg[:, 0] == Vg[:, 0].max())
    E, nu = 4e8, 0.3
    fab = dict(E1=E, E2=E, G12=E / (2 * (1 + nu)), nu12=nu)
    droop = {}
    for name, d in (("warp", (1.0, 0.0, 0.0)), ("weft", (0.0, 0.0, 1.0))):
        c = context(gpu_lib, V, tri, d, fab=fab, h=2e-3, E=E, rho=1000.0, bend=1.0, bend_warp=10.0, bend_weft=1.0, gravity=True, held=held)
        c.set_rel_tol(1e-6)
        c.precompute()
        settle(c, 5, 300)
        droop[name] = -c.state()["V"][tip, 1].mean()
        f = c.shell_weave_get()["hingeFactor"]
        print(f"cut along the {name}: tip droop {droop[name]:.4g} of 0.4; hinge factors {f.min():.3g} .. {f.max():.3g}")
    assert 0.0 < droop["warp"] < droop["weft"]
    assert droop["weft"] > 3 * droop["warp"]  # a factor 10 in the stiffness: nothing marginal is compared


def test_adding_and_removing_the_weave_leaves_the_run_bit_identical(gpu_lib):
    """A weave set and removed again (zeros, then None), and an all-zero selector from the start, leave a 5-step run bit-identical to a context that never made the
    call (one triangle: no atomic order).  On a bent pair of triangles the hinge constants come back bit for bit, too."""
    out = []
    for how in ("never", "all zero", "zeros", "none"):
        c = gpu_lib.Context(0)
        c.set_mesh(ONE_V, NO_T)
        c.set_shell(ONE_TRI, 1e-3, 1e5, 0.3, 1000.0)
        if how == "all zero":
            c.set_shell_weave(np.zeros(1, dtype=np.int32), (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)
        elif how != "never":
            c.set_shell_weave(1, (1.0, 0.0, 0.0), 1e5, 5e4, 2e3, 0.2, 3.0, 2.0)
            assert c.shell_weave_get()["woven"].tolist() == [1]
            c.set_shell_weave(np.zeros(1, dtype=np.int32) if how == "zeros" else None)
        w = c.shell_weave_get()
        assert w["woven"].tolist() == [0] and not w["a"].any() and not w["const4"].any()
        c.set_positions(ONE_V * 1.2)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(ONE_TRI)
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        E = c.shell_energy()
        for _ in range(5):
            assert c.solve_timestep(100) < 100
        assert c.shell_weave_energy() == 0.0 and not c.shell_weave_gradient_add().any() and not c.shell_weave_energy_per_elem().any() and not c.shell_weave_state().any()
        out.append((g, E, c.state()["V"]))
    assert out[0][1] > 0.0  # the StVK membrane is back
    for g, E, X in out[1:]:
        assert np.array_equal(g, out[0][0]) and E == out[0][1] and np.array_equal(X, out[0][2])
    # the hinge: factors on, then off again, between steps and after opt_init
    x = smp.hinge_nodes(40)
    c = gpu_lib.Context(0)
    c.set_mesh(smp.hinge_nodes(0), NO_T)
    c.set_shell(smp.HINGE_TRI, 1e-3, 1e5, 0.3, 1000.0, bend_scale=0.7)
    c.opt_init(0.01, False)
    c.set_positions(x)
    tri0, hinge0 = c.shell_energy_per_elem()
    plan0 = c.shell_get()
    c.set_shell_weave([1, 0], (1.0, 0.0, 0.0), 1e5, 5e4, 2e3, 0.2, 5.0, 3.0)
    f = c.shell_weave_get()["hingeFactor"]
    assert f.tolist() == [(3.0 + 1.0) / 2]  # the edge runs along the warp of the one woven triangle: bendWeft there, 1 for the other
    tri1, hinge1 = c.shell_energy_per_elem()
    assert hinge0[0] > 0 and abs(hinge1[0] - 2.0 * hinge0[0]) <= 4 * wmp.U * hinge1[0] and tri1[0] == 0.0 and tri1[1] == tri0[1]
    assert all(np.array_equal(c.shell_get()[k], plan0[k]) for k in ("hingeWeight", "restAngle", "area", "mass"))  # ipcgpu_shell_get: the plan's values, as before
    c.set_shell_weave([1, 0], (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)  # default factors: row 1 is the plan's again
    assert np.array_equal(c.shell_energy_per_elem()[1], hinge0)
    c.set_shell_weave([1, 0], (1.0, 0.0, 0.0), 1e5, 5e4, 2e3, 0.2, 5.0, 3.0)
    c.set_shell_weave(None)
    tri2, hinge2 = c.shell_energy_per_elem()
    assert np.array_equal(tri2, tri0) and np.array_equal(hinge2, hinge0) and np.all(c.shell_weave_get()["hingeFactor"] == 1.0)


def test_set_shell_and_set_mesh_drop_the_weave(gpu_lib):
    c = gpu_lib.Context(0)
    c.set_mesh(ONE_V, NO_T)
    c.set_shell(ONE_TRI, 1e-3, 1e5, 0.3, 1000.0)
    c.set_shell_weave(1, (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)
    assert c.shell_thickness()[0] == 1e-3  # the rest thickness on a woven triangle
    c.set_shell(ONE_TRI, 2e-3, 1e5, 0.3, 1000.0)
    assert c.shell_weave_get()["woven"].tolist() == [0]
    c.set_positions(ONE_V * 1.2)
    c.opt_init(0.01, False)
    assert c.shell_weave_energy() == 0.0 and c.shell_energy_per_elem()[0][0] > 0.0  # StVK again, with its constants
    c.set_shell_weave(1, (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)  # allowed after opt_init
    assert c.shell_weave_energy() > 0.0 and c.shell_energy_per_elem()[0][0] == 0.0 and c.shell_energy() == c.shell_weave_energy()
    c.set_shell_strain_limit(1.5)  # a strain limit composes unchanged
    assert c.shell_limit_energy() > 0.0 and abs(c.shell_energy() - (c.shell_weave_energy() + c.shell_limit_energy())) <= 4 * wmp.U * c.shell_energy()
    c.set_mesh(ONE_V, NO_T)  # a new mesh drops the shell and its weave
    assert c.shell_weave_get()["woven"].shape == (0,)
    assert c.shell_weave_energy_per_elem().shape == (0,) and c.shell_weave_state().shape == (0, 6)  # without a shell: nothing, and no error


def test_a_woven_triangle_is_neither_rubber_nor_plastic_both_ways_round(gpu_lib):
    V, tri = smp.hinge_nodes(0), np.array(smp.HINGE_TRI, dtype=np.int32)
    weave = lambda c, sel: c.set_shell_weave(sel, (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)

    def fresh():
        c = gpu_lib.Context(0)
        c.set_mesh(V, NO_T)
        c.set_shell(tri, 1e-3, 1e5, 0.3, 1000.0)
        return c
    c = fresh()
    c.set_shell_membrane([0, 1])
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4.*shell_set_weave: triangle 1 carries the rubber membrane"):
        weave(c, [1, 1])
    assert not c.shell_weave_get()["woven"].any()  # a refused call sets nothing
    weave(c, [1, 0])  # side by side is fine
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4.*shell_set_membrane: rubber on a woven triangle \\(triangle 0\\)"):
        c.set_shell_membrane([1, 1])
    assert c.shell_membrane_get()[0].tolist() == [0, 1] and c.shell_weave_get()["woven"].tolist() == [1, 0]
    c = fresh()
    c.shell_set_plasticity((1, 2), 0.01)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4.*shell_set_weave: triangle 1 is plastic"):
        weave(c, [0, 1])
    weave(c, [1, 0])
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4.*shell_set_plasticity: triangle 0 is woven"):
        c.shell_set_plasticity((0, 2), 0.01)
    assert c.shell_weave_get()["woven"].tolist() == [1, 0]
    c.shell_set_plasticity((0, 2), np.inf, np.inf)  # switching the flow off is no flow


def test_argument_errors_name_the_triangle(gpu_lib):
    V, tri = smp.hinge_nodes(0), np.array(smp.HINGE_TRI, dtype=np.int32)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*no shell"):
        c.set_shell_weave(1, (1.0, 0.0, 0.0), 1e5, 5e4, 2e3)
    assert c.shell_weave_energy_per_elem().shape == (0,)
    c.set_shell(tri, 1e-3, 1e5, 0.3, 1000.0)
    ok = dict(woven=[1, 1], direction=(1.0, 0.0, 0.0), E1=1e5, E2=5e4, G12=2e3, nu12=0.2, bend_warp=1.0, bend_weft=1.0)
    two = lambda v, base: [base, v]
    for key, v, word in (("woven", [1, 2], "selector other than 0 or 1"), ("woven", [1, -1], "selector other than 0 or 1"), ("E1", two(np.nan, 1e5), "not finite"),
                         ("nu12", two(np.inf, 0.2), "not finite"), ("E1", two(0.0, 1e5), "not positive"), ("E2", two(-1.0, 5e4), "not positive"),
                         ("G12", two(0.0, 2e3), "not positive"), ("nu12", two(1.5, 0.2), "nu12\\^2 >= E1 / E2"), ("bend_warp", two(0.0, 1.0), "bend factor"),
                         ("bend_weft", two(-1.0, 1.0), "bend factor"), ("direction", [(1.0, 0.0, 0.0), (0.0, 0.0, 0.0)], "zero length"),
                         ("direction", [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)], "normal to the triangle")):
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*triangle 1 .*" + word):
            c.set_shell_weave(**dict(ok, **{key: v}))
        assert not c.shell_weave_get()["woven"].any()  # a refused call sets nothing
    c.set_shell_weave(**dict(ok, woven=[1, 0], E1=two(np.nan, 1e5)))  # a value of a triangle that is not woven is not read
    assert c.shell_weave_get()["woven"].tolist() == [1, 0]
