"""Elastic shells in the time stepper and the building blocks: free fall, a patch test, a clamped strip, draping over a plane and a block with contact, the
error paths, and that a context without a shell is left alone.  Small meshes; the multifrontal and the iterative solver."""
import numpy as np
import pytest

import shell_mp as smp
from codim_common import five_tet_cube, step_context
from ipc_amd import scene

pytestmark = pytest.mark.gpu

G = 9.80665
SOLVERS = (0, 2)
H, YM, PR, RHO = 1e-3, 1e5, 0.3, 1000.0


def cloth(n, m=None, spacing=0.1, y=0.0, origin=(0.0, 0.0)):
    """n x m nodes in the plane y = const (normal +y), as smp.grid numbers them"""
    V, tri = smp.grid(n, m, spacing)
    return np.column_stack([V[:, 0] + origin[0], np.full(len(V), y), -V[:, 1] + origin[1]]), tri


def shell_context(gpu_lib, V, tri, solver=0, bend=1.0, T=None, dt=0.01, gravity=True, held=None, x0=None, h=H, E=YM):
    return step_context(gpu_lib, V, lambda c: c.set_shell(tri, h, E, PR, RHO, bend_scale=bend), solver, T, YM, RHO, dt, gravity, held, x0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_free_fall_follows_the_discrete_recursion(gpu_lib, solver):
    """No contact, no constraint: backward Euler gives v += dt g, y += dt v for every node; a rigid translation leaves the shell energy at zero.  Bound: the
    project's iterate tolerance, 1e-9 of the fall distance.  Shell energy: a position error of 1e-9 x 1.5e-3 over a spacing of 0.1 is a strain
    of ~1e-11, squared in the energy: far below 1e-16 of the energy's magnitude sum (shell_mp scale), which is the bound asserted."""
    V, tri = cloth(4, y=1.0)
    c = shell_context(gpu_lib, V, tri, solver)
    c.set_surface(tri)
    c.set_rel_tol(1e-8)
    c.precompute()
    case = {"X": V, "x": V, "tri": tri, "h": np.full(len(tri), H), "YM": np.full(len(tri), YM), "PR": np.full(len(tri), PR), "bendScale": 1.0}
    scaleE = float(smp.patch_reference(smp.NP, case, magnitudes=True)[0])
    dt, v, fall = 0.01, 0.0, 0.0
    for step in range(5):
        assert c.solve_timestep(50) < 50
        v += dt * G
        fall += dt * v
        X = c.state()["V"]
        print(f"solver {solver} step {step}: fall {fall:.6g}, worst deviation {np.abs(X - (V - [0, fall, 0])).max():.3g}, shell energy {c.shell_energy():.3g}")
        assert np.all(np.abs(X - (V - [0.0, fall, 0.0])) <= 1e-9 * fall)
        assert 0.0 <= c.shell_energy() <= 1e-16 * scaleE


def test_patch_test_uniform_biaxial_stretch(gpu_lib):
    """x = s X on a flat cloth, xTilde = x: the interior rows of ipcgpu_gradient vanish, the boundary rows are the mpmath values (tolerance: shell_mp)"""
    V, tri = cloth(4)
    x = V * 1.1
    c = shell_context(gpu_lib, V, tri, gravity=False, x0=x)
    c.set_pattern()
    c.set_xtilde(x)
    coef = 0.01 ** 2
    case = {"X": V, "x": x, "tri": tri, "h": np.full(len(tri), H), "YM": np.full(len(tri), YM), "PR": np.full(len(tri), PR), "bendScale": 1.0,
            "dbc": np.zeros(len(V), dtype=np.int32)}
    case.update(smp.evaluate(case))
    ref, tol = smp.expected(case, "g", coef, True)
    interior = np.array([5, 6, 9, 10])
    rows = lambda a, ids: a.reshape(-1, 3)[ids]
    for g, name in ((c.gradient(coef, True), "gradient"), (c.assemble_newton(coef, True), "assemble_newton")):
        print(name, "worst err / tol", np.max(np.abs(g - ref) / tol), "interior", np.abs(rows(g, interior)).max(), "boundary", np.abs(ref).max())
        assert np.all(np.abs(g - ref) <= tol)
        assert np.all(np.abs(rows(g, interior)) <= rows(tol, interior) + np.abs(rows(ref, interior)))
    assert np.abs(ref).max() > 1e6 * tol.max()  # the boundary carries a real force


def _strip(gpu_lib, solver, bend):
    """A plate strip 0.1 wide, 0.02 thick, E = 1e8, clamped over its first TWO node columns (one held column is a pinned edge: no hinge crosses a boundary
    edge, and the strip would swing about it like a rigid door), 0.6 free: as a cantilever (E I = E h^3 w / 12 = 6.7, 2 kg/m, q = 19.6 N/m) its static tip
    deflection is q L^4 / (8 E I) = 0.048 and its first period 0.35 s, so after 20 steps of 0.01 s it is just past its first maximum (about twice the static
    value); ten times the bending stiffness gives 0.0048 and a period of 0.11 s: at most about 0.01 at any time.  Measured: 0.0201 and 0.0023 (backward Euler damps the swing
    towards the static values; the hinge model on this coarse mesh is stiffer than the beam).  (The default cloth of this file, h = 1e-3 and E = 1e5, has a static
    deflection of many strip lengths: within 0.2 s both strips are in free fall about the clamp and the bending stiffness shows only in the seventh digit.)"""
    V, tri = cloth(8, 2)
    held = np.flatnonzero(V[:, 0] <= 0.1 + 1e-12)
    c = shell_context(gpu_lib, V, tri, solver, bend=bend, held=held, h=0.02, E=1e8)
    c.set_surface(tri)
    c.set_rel_tol(1e-4)
    c.precompute()
    for step in range(20):
        c.begin_timestep()
        E = c.state()["E"]
        for it in range(100):
            if c.newton_iter():
                break
            E1 = c.state()["E"]
            assert E1 <= E, (step, it, E, E1)  # the line search never accepts an increase
            E = E1
        else:
            raise AssertionError("no convergence in 100 iterations")
        c.end_timestep()
        X = c.state()["V"]
        assert np.all(np.isfinite(X)) and np.all(X[held] == V[held])
    return V, c.state()["V"]


@pytest.mark.parametrize("solver", SOLVERS)
def test_clamped_strip_sags_less_with_more_bending_stiffness(gpu_lib, solver):
    V, X1 = _strip(gpu_lib, solver, 1.0)
    _, X10 = _strip(gpu_lib, solver, 10.0)
    tip = np.flatnonzero(V[:, 0] == V[:, 0].max())
    d1, d10 = (V[tip, 1] - X1[tip, 1]).mean(), (V[tip, 1] - X10[tip, 1]).mean()
    print(f"solver {solver}: tip deflection bend 1: {d1:.6g}, bend 10: {d10:.6g}")
    assert 0.0 < d10 < d1


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("friction", (0.0, 0.3))
def test_cloth_drapes_over_a_block_and_a_plane_without_intersection(gpu_lib, solver, friction):
    """A 0.5 x 0.5 cloth 0.055 above the plane y = 0, over a held block 0.2 x 0.04 x 0.2 whose top is at 0.045.  Free fall covers g dt^2 n (n + 1) / 2 = 0.065
    in 11 steps, so in 18 steps the middle of the cloth lies on the block and its rim has reached the plane: both kinds of constraint are active at the end
    (asserted: half-space constraints in the stepper's sets, a half-space row and a block row in the contact report, a node within the barrier's reach of
    the plane)."""
    P, T = five_tet_cube(np.array([0.2, 0.04, 0.2]), np.array([0.15, 0.005, -0.35]))
    Vc, tri = cloth(6, y=0.055, origin=(0.0, 0.0))
    V = np.vstack([P, Vc])
    tri = tri + len(P)
    SF = np.vstack([scene.surface_tris(T), tri]).astype(np.int32)
    c = shell_context(gpu_lib, V, tri, solver, T=T, held=np.arange(len(P)))
    c.set_components([len(P), len(V)], [len(T), len(T)])
    c.set_surface(SF)
    c.enable_self_collision(1e-3)
    plane = c.add_half_space((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1e-3)
    if friction > 0:
        c.set_friction(friction, 1, 1e-3)
        c.set_half_space_friction(plane, friction)
    c.precompute()
    onPlane = 0
    for step in range(18):
        assert c.solve_timestep(200) < 200
        X = c.state()["V"]
        assert np.all(np.isfinite(X)) and not c.is_intersected() and X[:, 1].min() > 0.0
        onPlane += c.contact_state()["nHalfSpace"] > 0
    rep, st, reach = c.contact_report(), c.contact_state(), np.sqrt(c.state()["dHat"])
    low = X[len(P):, 1].min()
    assert onPlane >= 3  # plane constraints were active at the end of several steps, not in one bounce
    print(f"solver {solver} friction {friction}: lowest cloth node {low:.3g} (barrier reach {reach:.3g}), highest {X[len(P):, 1].max():.4f}, "
          f"half-space constraints {st['nHalfSpace']}, mesh constraints {st['nActive'] + st['nPara']}, report rows {[(int(a), int(b)) for a, b in zip(rep['a'], rep['b'])]}")
    assert 0.0 < low < reach and st["nHalfSpace"] > 0  # the rim rests on the plane, inside the barrier
    assert X[len(P):, 1].max() > 0.045  # ... and the block holds the middle up
    assert st["nActive"] + st["nPara"] > 0
    assert np.any(rep["b"] < 0) and np.any(rep["b"] >= 0)  # a half-space row and a row between components


def test_error_paths(gpu_lib):
    V, tri = cloth(3)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32))
    c.set_shard(0, 2)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_shell(tri, H, YM, PR, RHO)
    c = shell_context(gpu_lib, V, tri)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.system_report()
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3"):
        c.set_shell(tri, H, YM, PR, RHO)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32))
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*same direction"):
        c.set_shell(np.array([[0, 1, 4], [0, 1, 3]]), H, YM, PR, RHO)


def test_scene_material_reaches_the_masses_once(gpu_lib, tmp_path):
    """A shell shape with its own `material`, through scene_script.apply on a real context: the nodal masses are rho h A / 3 summed over the triangles --
    the shape's density, once (ipcgpu_set_component_material would scale them by rho / density a second time)."""
    from ipc_amd import scene_script as ss
    V, tri = smp.grid(4)
    (tmp_path / "cloth.obj").write_text("".join(f"v {a} {b} {c}\n" for a, b, c in V) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in tri))
    cfg = ss.SceneConfig.parse("shapes input 1\ncloth.obj 0 1 0  0 0 0  1 1 1 material 900 1e6 0.3 shell 0.002\ndensity 500\nstiffness 2e5 0.35\n", str(tmp_path))
    sc = ss.assemble(cfg, lambda p: None)
    c = gpu_lib.Context(0)
    ss.apply(sc, c)
    want = np.zeros(len(V))
    np.add.at(want, tri.ravel(), np.repeat(900.0 * 0.002 * 0.5 * 0.1 * 0.1 / 3, 3 * len(tri)))
    for got in (c.shell_get()["mass"], c.features()["mass"]):
        assert np.allclose(got, want, rtol=1e-13, atol=0)


def test_pattern_built_before_set_shell_is_rebuilt(gpu_lib):
    V, tri = cloth(3)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32))
    c.set_surface(tri)
    c.set_pattern()  # triangle edges only: the opposite pairs of the hinges are missing
    n0 = len(c.get_pattern()[1])
    c.set_shell(tri, H, YM, PR, RHO)
    assert len(c.get_pattern()[1]) > n0
    c.opt_init(0.01, False)
    c.set_positions(V + 0.01 * np.random.default_rng(1).standard_normal(V.shape))
    c.shell_hessian_add(1.0, True)  # every block is there (IPCGPU_ERR_STATE otherwise)


def test_replacing_and_removing_a_shell_puts_the_masses_back(gpu_lib):
    V, tri = cloth(4)
    area = 0.5 * 0.1 * 0.1
    codim = np.full(len(V), 0.125)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32))
    c.set_codim_nodes(np.arange(len(V)), codim)
    lumped = lambda t, h: np.bincount(t.ravel(), minlength=len(V)) * RHO * h * area / 3
    c.set_shell(tri, H, YM, PR, RHO)
    assert np.allclose(c.features()["mass"], lumped(tri, H), rtol=1e-13, atol=0)
    part = tri[:6]  # replaced by a smaller, thicker one: the nodes it leaves out get their area masses back
    c.set_shell(part, 2 * H, YM, PR, RHO)
    inPart = np.bincount(part.ravel(), minlength=len(V)) > 0
    assert not inPart.all() and c.shell_get()["nTri"] == 6
    assert np.allclose(c.features()["mass"], np.where(inPart, lumped(part, 2 * H), codim), rtol=1e-13, atol=0)
    c.set_shell(np.zeros((0, 3), dtype=np.int32), H, YM, PR, RHO)
    assert c.shell_get()["nTri"] == 0 and c.shell_get()["nHinge"] == 0 and np.array_equal(c.features()["mass"], codim)


def test_large_cloth_beside_tetrahedra_goes_through_the_patch_assembly(gpu_lib):
    """4 356 shell nodes beside a five-tet block: the patch plan owns the cloth's rows too (mass diagonal, inertia), and nodes without elements must not
    pile up in one patch (3 doubles of LDS per owned node: one patch of all of them asks for more LDS than a workgroup has).  The Newton assembly equals
    the sum of the entry points that build it term by term: mass diagonal + tet-parallel elastic Hessian + shell Hessian, and the same for the gradient
    (different summation orders: 64 u of the largest entry)."""
    P, T = five_tet_cube(0.2, np.array([0.0, -1.0, 0.0]))
    Vc, tri = cloth(66, spacing=0.01, y=0.5)
    V = np.vstack([P, Vc])
    tri = tri + len(P)
    rng = np.random.default_rng(5)
    x = V + 1e-4 * rng.standard_normal(V.shape)
    c = shell_context(gpu_lib, V, tri, T=T, gravity=False, x0=x)
    c.set_pattern()
    c.set_xtilde(x)
    coef = 1e-4
    g = c.assemble_newton(coef, True)
    a = c.get_a()
    ia = c.get_pattern()[0]
    gsum = c.shell_gradient_add(coef, True, c.elastic_gradient(coef, True))
    c.set_zero()
    c.elastic_hessian_add(coef, True)
    c.shell_hessian_add(coef, True)
    b = c.get_a()
    m = np.repeat(c.features()["mass"], 3)
    b[ia[:-1]] += m  # every upper-CSR row starts with its diagonal
    assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 64 * smp.U * np.abs(b).max()
    assert np.abs(g - gsum).max() <= 64 * smp.U * np.abs(gsum).max()


def test_no_shell_no_side_effect(gpu_lib):
    Vb, Tb = scene.make_bar(3, 2, 2, size=(1.5, 1.0, 1.0))
    c = gpu_lib.Context(0)
    c.set_mesh(Vb, Tb)
    c.opt_init(0.01, True)
    c.set_pattern()
    rng = np.random.default_rng(3)
    c.set_positions(Vb + 0.01 * rng.standard_normal(Vb.shape))
    g0 = c.assemble_newton(1e-4, True)
    a0, ia0 = c.get_a(), c.get_pattern()[0]
    c.set_shell(np.zeros((0, 3), dtype=np.int32), H, YM, PR, RHO)
    g1 = c.assemble_newton(1e-4, True)
    assert np.array_equal(g0, g1) and np.array_equal(a0, c.get_a()) and np.array_equal(ia0, c.get_pattern()[0])
    assert c.shell_get()["nTri"] == 0 and c.shell_energy() == 0.0
