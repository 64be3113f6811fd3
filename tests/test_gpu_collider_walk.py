"""The analytic obstacles as the stepper walks them, and the reduction their energies share, on the 6 x 6 x 6 bar (343 nodes) through the public API.

Registration order.  The stepper visits every half-space in registration order, then every round collider in registration order, whatever the order of
the add calls: the energy sums and the object index of the close-constraint list are positions in that walk.  Two contexts that differ only in the order
of the two add calls therefore take bit-identical steps.

Block edges.  An energy is the sum of one positive barrier value per set entry, taken as 256-lane workgroup sums and one pass over those: sets of 0, 1,
256 and 257 entries are the empty launch, one lane, one full workgroup and a second workgroup with one lane.  With kappa = 1 the scale is exact, so the
device sum of n positive terms differs from their exact sum by at most (n - 1) 2^-53 relative in any order; the reference is the correctly rounded sum
(math.fsum, 2^-53 more) of the one-entry energies of the same entry point, and (n - 1) 2^-52 bounds the two together for n >= 2.  One entry is exact."""
import math

import numpy as np
import pytest

from ipc_amd import scene

pytestmark = pytest.mark.gpu

DT = 0.01


def bar_context(gpu_lib):
    V, F = scene.make_bar(6, 6, 6, size=(3.0, 1.0, 1.0))
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    return c, V


def slide(gpu_lib, plane_first):
    """the bar sliding along +x under gravity on a plane and a capsule that lies in it, both with friction: two time steps"""
    c, V = bar_context(gpu_lib)
    y0 = float(V[:, 1].min()) - 2e-3

    def plane():
        c.set_half_space_friction(c.add_half_space([0.0, y0, 0.0], [0.0, 1.0, 0.0]), 0.3)

    def capsule():
        c.set_round_collider_friction(c.add_round_collider([-1.0, y0 - 0.2, 0.0], [1.0, y0 - 0.2, 0.0], 0.2), 0.4)
    for add in ((plane, capsule) if plane_first else (capsule, plane)):
        add()
    c.set_velocity(np.tile([0.5, 0.0, 0.0], (len(V), 1)))
    c.precompute()
    out = []
    for _ in range(2):
        n = c.solve_timestep(100)
        s = c.state()
        out.append((s["V"].copy(), s["E"], n, s["innerIterAmt"], c.round_state(0)["n"], c.friction_state()["n_half_space_lagged"]))
    c.close()
    return out


def test_registration_order_does_not_change_the_steps(gpu_lib):
    a, b = slide(gpu_lib, True), slide(gpu_lib, False)
    for (Va, Ea, na, ia, ra, ha), (Vb, Eb, nb, ib, rb, hb) in zip(a, b):
        assert ra > 0 and ha > 0, (ra, ha)  # both obstacles act, with friction lagged on the plane
        assert np.array_equal(Va, Vb)
        assert np.array_equal([Ea, na, ia, ra, ha], [Eb, nb, ib, rb, hb])


@pytest.mark.parametrize("kind", ["halfspace", "round"])
def test_energy_sum_at_block_edges(gpu_lib, kind):
    c, V = bar_context(gpu_lib)
    if kind == "halfspace":  # every node lies between 0.1 and 1.1 above the plane
        idx, dHat = c.add_half_space([0.0, -0.6, 0.0], [0.0, 1.0, 0.0]), 1.2 ** 2
        set_, energy = c.halfspace_set, c.halfspace_energy
    else:  # a solid sphere under the bar: gaps between 0.1 and 1.7
        idx, dHat = c.add_sphere_collider([0.0, -2.0, 0.0], 1.4), 1.8 ** 2
        set_, energy = c.round_set, c.round_energy
    order = np.random.default_rng(3).permutation(len(V)).astype(np.int32)[:257]
    one = []
    for v in order:
        set_(idx, np.array([v], dtype=np.int32))
        one.append(energy(idx, dHat, 1.0))
    assert all(e > 0.0 and math.isfinite(e) for e in one), min(one)
    for n in (0, 1, 256, 257):
        set_(idx, order[:n])
        got, want = energy(idx, dHat, 1.0), math.fsum(one[:n])
        print(f"{kind} n={n}: got {got!r} want {want!r} rel {abs(got - want) / want if want else 0.0:.3e} bound {(n - 1) * 2.0 ** -52 if n else 0.0:.3e}")
        if n == 0:
            assert got == 0.0
        else:
            assert abs(got - want) <= (n - 1) * 2.0 ** -52 * want, (n, got, want)
    c.close()
