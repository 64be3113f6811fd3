"""Round colliders in the time stepper: a five-tet cube (or a 5 x 5 shell sheet) against a sphere, a hollow sphere, a capsule and a moving sphere; a few
dozen nodes and a few dozen steps each.  The colliders see the surface VERTICES only (one distance evaluation per vertex), so a cube rests on a sphere
with its four bottom corners.

Force balance.  With backward Euler the stepper's gradient of the incremental potential, summed over the nodes of a free body, is
  sum g = sum M (x - 2 x_n + x_n-1) - dt^2 m grav + (barrier + friction gradient of the collider),
the elastic forces summing to zero.  With F the state query's barrier plus friction force on the body (minus those gradients, in the same units),
  |F - (-dt^2 m grav)| <= |sum g| + |sum M (x - 2 x_n + x_n-1)|
holds at every step, and at rest the right side is small against dt^2 m |grav|: both are asserted."""
import numpy as np
import pytest

import codim_common as cc
from ipc_amd import scene
from ipc_amd.lib import IpcGpuError

pytestmark = pytest.mark.gpu

DT, GRAV = 0.01, 9.80665
SIZE = 0.1


def cube_context(gpu_lib, lo, solver=0, iterative=None):
    V, T = cc.five_tet_cube(SIZE, np.asarray(lo, dtype=np.float64))
    c = gpu_lib.Context(0, solver=solver)
    if iterative:
        c.set_iterative(*iterative)
    c.set_mesh(V, T, YM=1e6, PR=0.4, density=1000.0)
    c.opt_init(DT, True)
    c.set_time_integration("BE")
    c.set_surface(scene.surface_tris(T))
    return c, V, T


def run(c, steps, each=None, probe=None):
    """`steps` time steps as ipcgpu_opt_solve_timestep takes them; probe() is called inside the last one, before it ends: x^t and the friction lag
    are then still those the step's own gradient was evaluated with"""
    hist = [c.state()["V"].copy()]
    for k in range(steps):
        if each:
            each(k)
        c.begin_timestep()
        it = 0
        while True:
            while it < 200 and not c.newton_iter():
                it += 1
            if it >= 200 or not c.next_subproblem():
                break
        assert it < 200
        if probe and k == steps - 1:
            probe()
        c.end_timestep()
        hist.append(c.state()["V"].copy())
    return hist


class Balance:
    """|F - dt^2 m g e_y| per component, its bound from the residual and the inertia, and dt^2 m g; taken inside the last step"""

    def __init__(self, c, idx):
        self.c, self.idx = c, idx

    def __call__(self):
        self.st, self.rs = self.c.state(), self.c.round_state(self.idx)

    def figures(self, hist):
        mass = np.asarray(self.c.features()["mass"])
        x0, x1, x2 = hist[-1], hist[-2], hist[-3]
        inertia = (mass[:, None] * (x0 - 2 * x1 + x2)).sum(axis=0)
        g = self.st["gradient"].reshape(-1, 3).sum(axis=0)
        want = np.array([0.0, DT * DT * mass.sum() * GRAV, 0.0])
        F = self.rs["force"] + self.rs["friction"]
        bound = np.abs(g) + np.abs(inertia) + 64 * 2.0 ** -53 * (np.abs(F) + want[1])
        return np.abs(F - want), bound, want[1], self.rs


SPHERE = dict(centre=np.array([0.05, -0.5, 0.05]), R=0.45)


def drop_on_sphere(gpu_lib, solver=0, iterative=None, mu=0.5, shift=0.0, steps=40):
    """the cube 2e-3 above where its corners would touch the sphere below it; shift: the cube's offset in x"""
    corner = np.sqrt(SPHERE["R"] ** 2 - 2 * (SIZE / 2) ** 2) + SPHERE["centre"][1]
    c, V, T = cube_context(gpu_lib, [shift, corner + 2e-3, 0.0], solver, iterative)
    idx = c.add_sphere_collider(SPHERE["centre"], SPHERE["R"], False, 1e-3)
    if mu > 0:
        c.set_round_collider_friction(idx, mu)
    c.precompute()
    mins, bal = [], Balance(c, idx)
    hist = run(c, steps, lambda k: mins.append(c.round_state(idx)["min_s"]), bal)
    mins.append(c.round_state(idx)["min_s"])
    return c, idx, hist, mins, bal


def free_fall(gpu_lib, steps, collider):
    c, V, T = cube_context(gpu_lib, [0.0, 0.0, 0.0])
    if collider:
        c.add_sphere_collider([0.0, -50.0, 0.0], 1.0, False, 1e-3)
    c.precompute()
    return c, run(c, steps)


def test_a_far_collider_changes_no_bit_of_a_falling_cube(gpu_lib):
    c0, h0 = free_fall(gpu_lib, 5, False)
    c1, h1 = free_fall(gpu_lib, 5, True)
    assert c1.round_state(0)["n"] == 0
    for a, b in zip(h0, h1):
        assert np.array_equal(a, b)
    assert h0[-1][:, 1].max() < h0[0][:, 1].max() - 0.01
    c0.close()
    c1.close()


def test_a_context_runs_as_before_after_a_collider_was_added_and_the_context_reset(gpu_lib):
    c0, h0 = free_fall(gpu_lib, 4, False)
    c1, _ = free_fall(gpu_lib, 2, True)
    V, T = cc.five_tet_cube(SIZE, np.zeros(3))
    c1.set_mesh(V, T, YM=1e6, PR=0.4, density=1000.0)  # the reset: clears the colliders where it clears the planes
    c1.opt_init(DT, True)
    c1.set_time_integration("BE")
    c1.set_surface(scene.surface_tris(T))
    with pytest.raises(IpcGpuError, match="index out of range"):
        c1.round_state(0)
    c1.precompute()
    h1 = run(c1, 4)
    for a, b in zip(h0, h1):
        assert np.array_equal(a, b)
    c0.close()
    c1.close()


@pytest.fixture(scope="module")
def rested(gpu_lib):
    return drop_on_sphere(gpu_lib)


def test_cube_dropped_on_a_sphere_with_friction_comes_to_rest_in_balance(rested):
    c, idx, hist, mins, bal = rested
    assert min(mins) > 0.0
    move = np.abs(hist[-1] - hist[-2]).max()
    err, bound, mg, rs = bal.figures(hist)
    print(f"cube on sphere: last step moves {move:.3g}; |F - dt^2 m g| = {err}, bound {bound}, dt^2 m g = {mg:.6g}, set {rs['n']}, min s {rs['min_s']:.3g}")
    assert rs["n"] == 4 and move <= 1e-6  # at rest on its four bottom corners
    assert np.all(err <= bound)
    assert bound.max() <= 1e-2 * mg  # the run did come to rest: the balance is tested, not the bound


def test_cube_dropped_off_centre_without_friction_slides_off(gpu_lib):
    c, idx, hist, mins, _ = drop_on_sphere(gpu_lib, mu=0.0, shift=0.12, steps=60)
    assert min(mins) > 0.0
    centre = hist[-1].mean(axis=0)
    print(f"off-centre drop: the cube's centre ends at {centre}")
    assert centre[0] > hist[0].mean(axis=0)[0] and centre[1] < SPHERE["centre"][1]
    c.close()


def test_cube_inside_a_hollow_sphere_settles_at_the_bottom(gpu_lib):
    R, ctr = 0.3, np.array([0.05, 0.3, 0.05])
    bottom = ctr[1] - np.sqrt((R - 2e-3) ** 2 - 2 * (SIZE / 2) ** 2)  # the corners 2e-3 inside the sphere
    c, V, T = cube_context(gpu_lib, [0.0, bottom, 0.0])
    idx = c.add_sphere_collider(ctr, R, True, 1e-3)
    c.set_round_collider_friction(idx, 0.5)
    c.precompute()
    rmax, bal = [], Balance(c, idx)
    hist = run(c, 40, lambda k: rmax.append(np.linalg.norm(c.state()["V"] - ctr, axis=1).max()), bal)
    rmax.append(np.linalg.norm(hist[-1] - ctr, axis=1).max())
    err, bound, mg, rs = bal.figures(hist)
    print(f"cube in bowl: max r / R = {max(rmax) / R:.6f}; |F - dt^2 m g| = {err}, bound {bound}, dt^2 m g = {mg:.6g}, set {rs['n']}")
    assert max(rmax) < R and rs["min_s"] > 0.0
    assert np.abs(hist[-1] - hist[-2]).max() <= 1e-6 and rs["n"] == 4
    assert np.all(err <= bound) and bound.max() <= 1e-2 * mg
    c.close()


def sheet(n=5, h=0.05, y=0.0):
    X = np.array([[h * (i - (n - 1) / 2), y, h * (j - (n - 1) / 2)] for i in range(n) for j in range(n)])
    tri = np.array([t for i in range(n - 1) for j in range(n - 1) for t in ((n * i + j, n * i + n + j, n * i + n + 1 + j), (n * i + j, n * i + n + 1 + j, n * i + 1 + j))],
                   dtype=np.int32)
    return X, tri


def test_a_sheet_drapes_over_a_capsule_bar(gpu_lib):
    X, tri = sheet(y=0.0)
    Rb, axisY = 0.02, -0.0205
    # (dt = 0.04: the two halves swing under the bar like pendulums, period 0.6 s; backward Euler at this step damps that within the run)
    c = cc.step_context(gpu_lib, X, lambda c: c.set_shell(tri, 5e-4, 1e5, 0.3, 500.0), dt=0.04)
    c.set_surface(tri)
    idx = c.add_round_collider([0.0, axisY, -0.5], [0.0, axisY, 0.5], Rb, False, 1e-3)
    c.set_round_collider_friction(idx, 0.5)
    c.precompute()
    mins = []
    hist = run(c, 50, lambda k: mins.append(c.round_state(idx)["min_s"]))
    mins.append(c.round_state(idx)["min_s"])
    x = hist[-1]
    left, right = x[:5], x[-5:]  # the rows at x = -0.1 and x = +0.1
    print(f"sheet over bar: min s {min(mins):.3g}; outer rows end at y = {left[:, 1].mean():.4f} / {right[:, 1].mean():.4f} (axis {axisY})")
    assert min(mins) > 0.0
    assert np.all(left[:, 1] < axisY) and np.all(right[:, 1] < axisY) and left[:, 0].mean() < 0.0 < right[:, 0].mean()
    assert x[10:15, 1].mean() > axisY + Rb  # the middle row still lies on the bar
    c.close()


def test_a_moving_sphere_pushes_a_held_sheet(gpu_lib):
    X, tri = sheet(y=0.0)
    held = np.r_[0:5, 20:25]
    c = cc.step_context(gpu_lib, X, lambda c: c.set_shell(tri, 5e-4, 1e5, 0.3, 500.0), dt=DT, gravity=False, held=held)
    c.set_surface(tri)
    R = 0.03
    idx = c.add_sphere_collider([0.0, -R - 5e-3, 0.0], R, False, 1e-3)
    c.precompute()
    v, fr, mins, carry = np.array([0.0, 0.5, 0.0]), [], [], np.zeros(3)
    for k in range(20):
        delta = v * DT + carry  # what the last move left over is carried into this one
        left = c.round_move(idx, delta, 0.5)
        carry = left * delta
        fr.append(1.0 - left)
        assert not c.round_state(idx)["min_s"] <= 0.0
        run(c, 1)
        mins.append(c.round_state(idx)["min_s"])
    x = c.state()["V"]
    print(f"moving sphere: fractions {min(fr):.3g} .. {max(fr):.3g}, min s {min(mins):.3g}, the sheet's centre at y = {x[12, 1]:.4f}, the sphere's top at {c.round_get(idx)['p0'][1] + R:.4f}")
    assert all(0.0 < f <= 1.0 for f in fr) and min(fr) < 1.0  # the sheet did cut a move short
    assert min(mins) > 0.0
    # displaced along the motion by more than the barrier's reach (dHat^(1/2) = 2.8e-4): pushed, not merely left alone.  (A move takes half the gap
    # at most, and the sheet only retreats inside dHat, so the sphere creeps: that is the rule of HipHalfSpace::move as well.)
    assert x[12, 1] > 1e-3 and x[12, 1] > c.round_get(idx)["p0"][1] + R and np.all(x[held, 1] == 0.0)
    c.close()


def test_guards(gpu_lib):
    c, V, T = cube_context(gpu_lib, [0.0, 0.0, 0.0])
    with pytest.raises(IpcGpuError, match="intersecting start"):
        c.add_sphere_collider([0.05, 0.05, 0.05], 0.2, False, 1e-3)
    with pytest.raises(IpcGpuError, match="intersecting start"):
        c.add_sphere_collider([0.05, 0.05, 0.05], 0.05, True, 1e-3)  # a hollow sphere the cube sticks out of
    with pytest.raises(IpcGpuError, match="radius must be positive"):
        c.add_sphere_collider([0.0, -1.0, 0.0], 0.0, False, 1e-3)
    with pytest.raises(IpcGpuError, match="radius must be positive"):
        c.add_sphere_collider([0.0, -1.0, 0.0], -0.5, False, 1e-3)
    with pytest.raises(IpcGpuError, match="not finite"):
        c.add_sphere_collider([0.0, np.nan, 0.0], 0.5, False, 1e-3)
    with pytest.raises(IpcGpuError, match="not finite"):
        c.add_sphere_collider([0.0, -1.0, 0.0], np.inf, False, 1e-3)
    with pytest.raises(IpcGpuError, match="only a sphere"):
        c.add_round_collider([0.0, -1.0, 0.0], [1.0, -1.0, 0.0], 0.5, True, 1e-3)
    with pytest.raises(IpcGpuError, match=r"R\^2 > dHat"):
        c.add_sphere_collider([0.05, 0.05, 0.05], 0.1, True, 1.0)  # dHat = the squared bounding-box diagonal, 0.03 > R^2
    idx = c.add_sphere_collider([0.0, -1.0, 0.0], 0.5, False, 1e-3)
    assert idx == 0
    with pytest.raises(IpcGpuError, match="share one dHat"):
        c.add_sphere_collider([0.0, -3.0, 0.0], 0.5, False, 2e-3)
    with pytest.raises(IpcGpuError, match="share one dHat"):
        c.add_half_space([0.0, -5.0, 0.0], [0.0, 1.0, 0.0], 2e-3)
    with pytest.raises(IpcGpuError, match="sharded"):
        c.set_shard(0, 2)
    with pytest.raises(IpcGpuError, match="round collider"):
        c.system_report()
    # a start state moved into the collider from outside is refused when the step begins
    c.precompute()
    c.set_positions(V + np.array([0.0, -0.58, 0.0]))
    with pytest.raises(IpcGpuError, match="intersecting start"):
        c.begin_timestep()
    c.close()
    c2, V, T = cube_context(gpu_lib, [0.0, 0.0, 0.0])
    c2.set_shard(0, 2)
    with pytest.raises(IpcGpuError, match="sharded"):
        c2.add_sphere_collider([0.0, -1.0, 0.0], 0.5, False, 1e-3)
    c2.close()


def test_pcg_reaches_the_same_rest_position(gpu_lib, rested):
    """the bound of tests/test_gpu_pcg.py: ten times the difference of the two direct solvers, at least 1e-11 of the scene's size"""
    r0 = rested[2]
    c1, _, r1, _, _ = drop_on_sphere(gpu_lib, solver=1)
    c2, _, r2, _, _ = drop_on_sphere(gpu_lib, solver=2, iterative=(1e-10, 1000, 0, 8))
    diag = float(np.linalg.norm(r0[0].max(0) - r0[0].min(0)))
    d01, d02 = np.abs(r0[-1] - r1[-1]).max(), np.abs(r0[-1] - r2[-1]).max()
    bound = 10 * max(d01, 1e-12 * diag)
    print(f"cube on sphere at rest: max|x_0 - x_1| = {d01:.3e}, max|x_0 - x_2| = {d02:.3e}, bound {bound:.3e}")
    assert d02 <= bound
    c1.close()
    c2.close()
