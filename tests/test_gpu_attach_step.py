"""Attachments in the time stepper and the building blocks: a free spring between two blocks, a block hanging by a tether, two sewn cloth strips, a cloth
corner tied to a scripted collider, a rod end on a tetrahedral face, the error paths, and that a context without attachments is left alone.  Small meshes;
the multifrontal and the iterative solver where cheap."""
import numpy as np
import pytest

import rod_mp as rmp
import shell_mp as smp
from codim_common import NO_T, five_tet_cube, step_context

pytestmark = pytest.mark.gpu

G = 9.80665
SOLVERS = (0, 2)
RHO = 1000.0
NO_SF = np.zeros((0, 3), dtype=np.int32)
# Young's modulus of the blocks in the tests that assert to the iterate tolerance: stiff enough that the loads here (at most 150 N on a 0.1 m block) strain
# them by 1e-5, so the eigenvalue projection of the tetrahedral Hessians changes next to nothing and Newton's method keeps its fast convergence down to a
# relative tolerance of 1e-9 (with E = 1e6 the projected Hessians of the loaded elements make it linear, 0.78 per iteration: 100 iterations do not reach it)
STIFF = 1e9
# LINE_SEARCH_FLOOR: the line search compares incremental potentials in fp64, so it cannot see a decrease below u E; a Newton step p with p^T H p / 2 under
# that is rejected however often it is halved, and the stepper never gets under |p| ~ sqrt(2 u E / lambda).  Measured on the rod scene below (E = 1.2e-3 at
# dt = 0.05, the block's gravity potential): a stall at |p| = 3e-9; on the two free blocks at 2e-10.  The relative tolerances of these two tests (1e-6:
# |p| < 2e-8 and 4e-9) stay above that floor; the bounds asserted are derived from the tolerance that is set, whatever it is.


def iterate_bound(relTol, V, dt, k):
    """The stepper stops when the Newton step is shorter than tol = relTol x (bounding-box diagonal) x dt, so an iterate lies within delta = 2 tol of its
    step's minimiser; the error enters the next step's xTilde = 2 x_k - x_(k-1), an undamped recursion whose solution after k steps is at most
    delta (k + 1)^2 (the derivation of test_gpu_rod_step.py's hanging rod)."""
    return 2 * relTol * np.linalg.norm(V.max(0) - V.min(0)) * dt * (k + 1) ** 2


@pytest.mark.parametrize("solver", SOLVERS)
def test_free_spring_exerts_no_net_force_and_no_net_torque(gpu_lib, solver):
    """Two free blocks joined by one pre-stretched tether between two corner nodes (off the line of the centres: the blocks turn as well), no gravity, at
    rest: the spring force is internal (1.5 N on blocks of 1 kg: a stiff block turned by a large angle within one step would cost Newton's method
    hundreds of iterations).  With backward Euler v_k = (x_k - x_(k-1)) / dt, and the exact discrete trajectory obeys
    M (v_(k+1) - v_k) = -dt grad W(x_(k+1)).  W is invariant under translation and rotation (test_attach_mp.py), so sum grad W = 0 and
    sum x x grad W = 0: the total linear momentum P stays at its initial zero, and the angular momentum L = sum m x x v obeys
    L_(k+1) - L_k = dt sum m v_(k+1) x v_k exactly (backward Euler itself does not conserve L: this term is the integrator's, and it is there without any
    attachment; a net torque of the spring would add to it).  Both are asserted.  Bound: every x_k lies within e_k = delta (k + 1)^2 of the exact discrete
    trajectory (iterate_bound), so a velocity is off by 2 e_k / dt: |P| <= 2 M e_k / dt; a term m x x v by m (2 |x| e_k / dt + e_k |v|), two L's and the
    product term give 4 M e_k R / dt + 6 M e_k vmax, R the largest distance of a node from the origin and vmax the largest nodal speed of the run."""
    Pa, T = five_tet_cube(0.1, np.array([0.0, 0.0, 0.0]))
    Pb, _ = five_tet_cube(0.1, np.array([0.25, 0.05, 0.02]))
    V = np.vstack([Pa, Pb])
    TT = np.vstack([T, T + 8]).astype(np.int32)
    relTol, dt, steps = 1e-6, 0.01, 10  # (LINE_SEARCH_FLOOR)
    c = step_context(gpu_lib, V, lambda c: c.set_attachments([6], [8 + 0], 20.0, 0.1), solver, TT, STIFF, RHO, dt, gravity=False)
    c.set_rel_tol(relTol)
    c.precompute()
    m = c.features()["mass"]
    l0, f0 = c.attach_state()
    assert l0[0] > 0.1 and f0[0] > 0  # pre-stretched
    prev, vmax, moved, Lprev, vprev = V.copy(), 0.0, 0.0, np.zeros(3), np.zeros(V.shape)
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
        moved = max(moved, np.abs(m[:8, None] * v[:8]).sum())
        torque = Lm - Lprev - dt * (m[:, None] * np.cross(v, vprev)).sum(axis=0)
        Lprev, vprev = Lm, v
        print(f"solver {solver} step {k}: |P| {np.linalg.norm(Pm):.3g} (bound {bP:.3g}), |L| {np.linalg.norm(Lm):.3g}, defect of the angular momentum balance "
              f"{np.linalg.norm(torque):.3g} (bound {bL:.3g}), one block's momentum {moved:.3g}")
        assert np.linalg.norm(Pm) <= bP and np.linalg.norm(torque) <= bL
    assert moved > 1e2 * bP  # the spring really moved the blocks: the zero is a cancellation, not rest
    assert c.attach_state()[0][0] < l0[0]


@pytest.mark.parametrize("solver", SOLVERS)
def test_block_hanging_by_a_tether_settles_at_m_g_over_k(gpu_lib, solver):
    """A block hangs by one tether from a node of a held block above it; the tether ends on the middle of the hanging block's top face (the midpoint of a
    face diagonal, an edge point), above its centre of mass.  At rest the tether carries the whole weight: l - L = m g / k, whatever the block's own
    elastic sag.  Backward Euler with dt = 1 damps every mode by 1 / sqrt(1 + w^2 dt^2) per step (w >= sqrt(k / m) = 31: at least 1e-15 over ten steps;
    the start is the rigid equilibrium, off by the block's sag only), so what remains is the iterate tolerance, bounded as in iterate_bound."""
    k, L, size = 1000.0, 0.05, 0.1
    Ph, T = five_tet_cube(size, np.array([0.0, 0.3, 0.0]))
    Pc, _ = five_tet_cube(size, np.array([0.0, 0.0, 0.0]))
    mass = RHO * size ** 3
    ext = mass * G / k
    top = np.array([0.5 * size, size, 0.5 * size])  # the middle of the top face = the midpoint of the nodes 2 and 7 of five_tet_cube
    assert np.allclose(0.5 * (Pc[2] + Pc[7]), top)
    Ph = Ph - Ph[0] + top + [0.0, L + ext, 0.0]  # node 0 of the held block straight above, at the equilibrium distance
    V = np.vstack([Ph, Pc])
    TT = np.vstack([T, T + 8]).astype(np.int32)
    relTol, dt, steps = 1e-9, 1.0, 10
    c = step_context(gpu_lib, V, lambda c: c.set_attachments([[0, -1]], [[8 + 2, 8 + 7]], k, L, [[1.0, 0.0]], [[0.5, 0.5]]), solver, TT, STIFF, RHO, dt,
                     held=np.arange(8))
    c.set_rel_tol(relTol)
    c.precompute()
    assert abs(c.features()["mass"][8:].sum() - mass) <= 1e-12 * mass
    assert abs(c.attach_get()["restDist"][0] - (L + ext)) <= 1e-15
    prev = V
    for step in range(1, steps + 1):
        assert c.solve_timestep(100) < 100
        X = c.state()["V"]
        l, f = c.attach_state()
        drift = np.abs(X - prev).max()
        prev = X
    bound = iterate_bound(relTol, V, dt, steps) + 1e-12
    print(f"solver {solver}: extension {l[0] - L:.9g}, m g / k {ext:.9g}, difference {abs(l[0] - L - ext):.3g} (bound {bound:.3g}), last step moved {drift:.3g}")
    assert abs((l[0] - L) - ext) <= bound and abs(f[0] - mass * G) <= k * bound
    assert drift <= 2 * bound  # velocities have vanished
    assert np.all(X[:8] == V[:8])


def strips():
    """two 6 x 3-node strips in the plane y = 1, B behind A along x with a gap of 0.02; the seam: A's last column and B's first"""
    Va, tri = smp.grid(6, 3, 0.1)
    to3 = lambda P, x0: np.column_stack([P[:, 0] + x0, np.full(len(P), 1.0), P[:, 1]])
    V = np.vstack([to3(Va, 0.0), to3(Va, 0.52)])
    seamA = np.array([5, 11, 17])
    seamB = 18 + np.array([0, 6, 12])
    return V, np.vstack([tri, tri + 18]).astype(np.int32), seamA, seamB


def test_sewn_strips_hang_together_with_short_stitches(gpu_lib):
    """Strip A held along its far edge, strip B sewn to A's free edge by three zero-length stitches, the contact between the two strips masked by contact
    groups (a zero-length stitch would otherwise settle at a gap below dHat with the barrier active).  Backward Euler with dt = 0.5 for 16 steps damps the
    swing (period about 1.5 s: a factor 1 / sqrt(1 + w^2 dt^2) = 0.43 per step, 1e-6 in all).  At rest the stitches carry B's weight between them: no
    stitch is longer than (B's weight) / k, the bound with one stitch carrying everything; a residual swing of 1e-6 of the drop adds 1e-6 to the force."""
    V, tri, seamA, seamB = strips()
    k = 1000.0
    held = np.array([0, 6, 12])
    c = step_context(gpu_lib, V, lambda c: (c.set_shell(tri, 1e-3, 1e5, 0.3, RHO), c.set_attachments(seamA, seamB, k)), 0, None, 1e5, RHO, 0.5, held=held)
    c.set_components([18, 36], [0, 0])
    c.set_contact_groups([0, 1], [[1, 0], [0, 1]])
    c.set_surface(tri)
    c.enable_self_collision(1e-3)
    c.set_rel_tol(1e-6)
    c.precompute()
    assert np.allclose(c.attach_get()["restDist"], 0.02, rtol=0, atol=1e-15)  # pre-stretched by the gap
    weightB = c.features()["mass"][18:].sum() * G
    for step in range(16):
        assert c.solve_timestep(300) < 300
        X = c.state()["V"]
        assert np.all(np.isfinite(X)) and not c.is_intersected()
    l, f = c.attach_state()
    print(f"stitch lengths {l}, forces {f} (sum {f.sum():.6g}), B's weight {weightB:.6g}, bound {weightB / k:.3g}; mean height A {X[:18, 1].mean():.4f}, B {X[18:, 1].mean():.4f}")
    assert np.all(l <= weightB / k * (1 + 1e-3))
    assert abs(f.sum() - weightB) <= 0.05 * weightB  # ... and together they do carry it (the stitches are nearly parallel at rest)
    assert X[18:, 1].mean() < X[:18, 1].mean() and X[18:, 1].max() < 1.0
    assert np.all(X[held] == V[held])


def test_cloth_corner_follows_a_scripted_collider(gpu_lib):
    """A 3 x 3 cloth whose corner is tied (L = 0) to a node of a block that moves as a scripted Dirichlet body: the corner follows it, the attachment's force
    stays finite, and the rows of the collider's node in the attachment gradient are dropped (projected Dirichlet node) while the cloth's are not."""
    P, T = five_tet_cube(0.1, np.array([0.0, 0.0, 0.0]))
    Vc, tri = smp.grid(3, 3, 0.05)
    Vc = np.column_stack([Vc[:, 0] + 0.12, np.full(len(Vc), 0.1), Vc[:, 1]])
    V = np.vstack([P, Vc])
    tri = tri + 8
    k, dt, vel = 500.0, 0.01, np.array([0.0, 0.5, 0.0])
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=1e7, PR=0.4, density=RHO)
    c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
    c.set_attachments([2], [8], k)  # block node 2 = (0.1, 0.1, 0), cloth corner 8 = (0.12, 0.1, 0)
    c.opt_init(dt, True)
    c.set_time_integration("BE")
    c.add_dirichlet(np.arange(8, dtype=np.int32), lin_vel=vel)
    c.set_rel_tol(1e-6)
    c.precompute()
    steps = 20
    for step in range(steps):
        assert c.solve_timestep(100) < 100
        l, f = c.attach_state()
        assert np.all(np.isfinite(l)) and np.all(np.isfinite(f))
    X = c.state()["V"]
    travelled = vel * dt * steps
    assert np.allclose(X[:8], V[:8] + travelled, rtol=0, atol=1e-12)  # the collider went where its script sent it
    weight = c.features()["mass"][8:].sum() * G
    print(f"collider moved {travelled[1]:.3g}, corner moved {X[8, 1] - V[8, 1]:.4g}, stitch length {l[0]:.3g}, force {f[0]:.3g}, cloth weight {weight:.3g}")
    assert X[8, 1] - V[8, 1] > 0.8 * travelled[1]  # the corner follows ...
    assert X[9:, 1].min() < X[8, 1]  # ... and the rest of the cloth hangs from it
    g = c.attach_gradient_add(1.0, True).reshape(-1, 3)
    assert np.all(g[2] == 0.0) and np.linalg.norm(g[8]) > 0.0 and abs(np.linalg.norm(g[8]) - f[0]) <= 1e-12 * abs(f[0])


def test_rod_end_on_a_tetrahedral_face_settles_within_force_over_k(gpu_lib):
    """A rod hangs by its first node from a barycentric point of a side face of a block held at its bottom nodes (L = 0: a 4-node stencil whose pattern
    blocks and Hessian go through the patch assembly beside the tetrahedra).  At rest the stitch carries the rod's weight W: its length is W / k, within
    the iterate tolerance (iterate_bound; the rod starts with its end on the point, hanging straight down along the face -- there is no contact in this
    scene --, at rest up to its own stretch and the stitch's, and backward Euler with dt = 0.05 over 12 steps damps that vertical motion, w = sqrt(k / m)
    = 230, by 1 / 11 per step)."""
    size, k, dt, steps, relTol = 0.2, 100.0, 0.05, 12, 1e-6  # (LINE_SEARCH_FLOOR; dt: the block's gravity potential scales with dt^2)
    P, T = five_tet_cube(size, np.array([0.0, 0.0, 0.0]))
    face, w = np.array([2, 6, 1]), np.array([0.25, 0.25, 0.5])  # on the face x = size
    point = w @ P[face]
    assert abs(point[0] - size) <= 1e-15
    Vr, seg = rmp.chain(4, spacing=0.05, axis=(0.0, -1.0, 0.0), origin=point)
    V = np.vstack([P, Vr])
    seg = seg + 8
    R = 2e-3
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=STIFF, PR=0.4, density=RHO)
    c.set_rod(seg, R, 1e7, RHO)
    c.set_attachments([[8, -1, -1]], [face.tolist()], k, 0.0, [[1.0, 0.0, 0.0]], [w.tolist()])
    c.opt_init(dt, True)
    c.set_time_integration("BE")
    c.add_dirichlet(np.flatnonzero(P[:, 1] == 0.0).astype(np.int32))
    c.set_rel_tol(relTol)
    c.precompute()
    assert c.attach_get()["count"].tolist() == [4]
    W = c.rod_get()["mass"].sum() * G
    for step in range(steps):
        assert c.solve_timestep(200) < 200
    X = c.state()["V"]
    l, f = c.attach_state()
    gap = np.linalg.norm(X[8] - w @ X[face])
    bound = iterate_bound(relTol, V, dt, steps) + 1e-6 * W / k
    print(f"stitch length {l[0]:.6g} (point to rod end {gap:.6g}), W / k {W / k:.6g}, difference {abs(l[0] - W / k):.3g} (bound {bound:.3g})")
    assert abs(gap - l[0]) <= 1e-15 and abs(l[0] - W / k) <= bound


def test_error_paths(gpu_lib):
    V, seg = rmp.chain(4)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_shard(0, 2)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_attachments([0], [1], 10.0)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_rod(seg, 2e-3, 1e7, RHO)
    c.set_attachments([0], [3], 10.0, 0.1)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*set_pattern"):
        c.attach_hessian_add(1.0, True)  # no pattern yet
    c.opt_init(0.01, False)
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -4"):
        c.system_report()
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3"):
        c.set_attachments([0], [2], 10.0)  # after opt_init
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3"):
        c.set_attachments(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 10.0)  # removing them after opt_init, too
    bad = {"out of range": ([0], [4], 10.0, 0.0, None, None), "has no node": ([[-1, -1]], [[0, -1]], 10.0, 0.0, [[0.0, 0.0]], [[1.0, 0.0]]),
           "negative weight": ([[0, 1]], [[2, -1]], 10.0, 0.0, [[1.5, -0.5]], [[1.0, 0.0]]),
           "not finite": ([[0, 1]], [[2, -1]], 10.0, 0.0, [[np.nan, 0.5]], [[1.0, 0.0]]),
           "do not sum to 1": ([[0, 1]], [[2, -1]], 10.0, 0.0, [[0.5, 0.4]], [[1.0, 0.0]]), "k > 0": ([0], [1], 0.0, 0.0, None, None),
           "L >= 0": ([0], [1], 10.0, -1.0, None, None), "same point": ([[0, 1]], [[1, 0]], 10.0, 0.0, [[0.5, 0.5]], [[0.5, 0.5]])}
    for word, args in bad.items():
        c = gpu_lib.Context(0)
        c.set_mesh(V, NO_T)
        with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -1.*" + word):
            c.set_attachments(*args)
        assert c.attach_get()["n"] == 0


def test_pattern_built_before_set_attachments_is_rebuilt(gpu_lib):
    """(so IPCGPU_ERR_STATE from ipcgpu_attach_hessian_add for a missing block cannot be reached through the API: the call that adds the pairs rebuilds a
    pattern that exists)"""
    V, seg = rmp.chain(5)
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T)
    c.set_rod(seg, 2e-3, 1e7, RHO)
    c.set_pattern()
    n0 = len(c.get_pattern()[1])
    c.set_attachments([0], [4], 10.0)
    assert len(c.get_pattern()[1]) > n0
    c.opt_init(0.01, False)
    c.set_positions(V + 0.01 * np.random.default_rng(1).standard_normal(V.shape))
    c.attach_hessian_add(1.0, True)  # every block is there (IPCGPU_ERR_STATE otherwise)


def test_no_attachment_leaves_a_cube_cloth_and_rod_scene_bit_identical(gpu_lib):
    """A block, a one-triangle cloth and a one-segment rod (single elements: every entry receives one addend per kernel, so no atomic sum depends on an
    order).  Three contexts: no call; set_attachments with n == 0; a set, replaced by another, then removed.  Pattern, gradient, matrix values, masses and
    the positions after a step agree to the bit."""
    from ipc_amd import scene
    Vb, Tb = scene.make_bar(3, 2, 2, size=(1.5, 1.0, 1.0))
    nb = len(Vb)
    V = np.vstack([Vb, [[0.0, 3.0, 0.0], [0.3, 3.0, 0.0], [0.0, 3.0, 0.3]], [[2.0, 3.0, 0.0], [2.0, 2.8, 0.0]]])
    tri, seg = np.array([[nb, nb + 1, nb + 2]]), np.array([[nb + 3, nb + 4]])
    x = V + 0.01 * np.random.default_rng(3).standard_normal(V.shape)
    none = np.zeros(0, dtype=np.int32)
    out = []
    for mode in range(3):
        c = gpu_lib.Context(0)
        c.set_mesh(V, Tb)
        c.set_shell(tri, 1e-3, 1e5, 0.3, RHO)
        c.set_rod(seg, 2e-3, 1e7, RHO)
        m0 = c.features()["mass"]
        if mode == 1:
            c.set_attachments(none, none, 1.0)
        if mode == 2:
            c.set_attachments([0, nb], [nb + 3, 5], 50.0, [0.0, 0.1])
            assert c.attach_get()["n"] == 2 and np.array_equal(c.features()["mass"], m0)
            c.set_attachments([[1, 2, 3]], [[nb + 1, -1, -1]], 70.0, 0.0, [[0.25, 0.25, 0.5]], [[1.0, 0.0, 0.0]])
            assert c.attach_get()["n"] == 1 and c.attach_get()["count"].tolist() == [4]
            c.set_attachments(none, none, 1.0)
        assert np.array_equal(c.features()["mass"], m0)
        c.set_positions(x)
        c.opt_init(0.01, True)
        c.set_time_integration("BE")
        c.set_surface(np.vstack([scene.surface_tris(Tb), tri]).astype(np.int32), seg)
        c.precompute()
        g = c.assemble_newton(1e-4, True)
        a = c.get_a()
        assert c.solve_timestep(100) < 100
        out.append((g, a, c.state()["V"], c.get_pattern()[0], c.get_pattern()[1], m0))
        assert c.attach_get()["n"] == 0 and c.attach_energy() == 0.0 and c.attach_energy_per_elem().shape == (0,)
        assert np.array_equal(c.attach_gradient_add(1.0, True), np.zeros(3 * len(V))) and c.attach_state()[0].shape == (0,)
        c.attach_hessian_add(1.0, True)
    for p, q, r in zip(*out):
        assert np.array_equal(p, q) and np.array_equal(p, r)
