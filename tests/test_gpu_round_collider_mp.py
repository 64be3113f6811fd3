"""The round-collider kernels through the C ABI against the mpmath restatement of round_collider_mp.py: 40 hand-placed vertices (five five-tet cubes, every
node a surface node) per shape -- solid sphere, hollow sphere, an axis-aligned and a skew capsule with vertices in the cap region, in the side region,
exactly on the end planes and on the axis extension --, gaps just below and just above dHat, one Dirichlet vertex inside dHat.  The tolerance is
round_collider_mp's M (sens + u scale) with M = 1 (the float64 restatement's worst ratio 0.842, rounded up to a power of two).

Measured on one MI355X (worst err / (sens + u scale), printed by the tests): energy 0.842, gradient 0.330, Hessian 0.838, step bound 0.206, friction
gradient 0.007 / Hessian 0.173; the float64 restatement on the same cases: 0.842 / 0.330 / 0.752 / 0.206."""
import numpy as np
import pytest
from mpmath import mpf

import codim_common as cc
import round_collider_mp as rc
from ipc_amd import scene

pytestmark = pytest.mark.gpu

NAMES = ("solid_sphere", "hollow_sphere", "capsule_aligned", "capsule_skew")
MU, EPS2 = 0.4, 1.0e-6


class Carrier:
    def __init__(self, gpu_lib, name):
        self.collider, self.P, self.dbc = rc.cases()[name]
        cubes = [cc.five_tet_cube(0.5, np.array([1.0 * k, 0.0, 0.0])) for k in range(5)]
        self.V = np.vstack([q[0] for q in cubes])
        self.T = np.vstack([q[1] + 8 * k for k, q in enumerate(cubes)]).astype(np.int32)
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.V, self.T, YM=1e5, PR=0.4, density=1000.0)
        c.set_positions(self.P)
        c.opt_init(0.01, False)
        c.set_surface(scene.surface_tris(self.T))
        c.set_dbc(np.flatnonzero(self.dbc).astype(np.int32), 1)
        self.idx = c.add_round_collider(self.collider["p0"], self.collider["p1"], self.collider["R"], self.collider["hollow"], 1e-3)
        c.set_pattern()
        self.want = [v for v in range(40) if rc.active(self.collider, self.P[v], self.dbc[v], rc.DHAT)]

    def blocks(self):
        """the upper triangle of every node's diagonal block as 3 x 3 (lower part zero), and whether anything else of the matrix is non-zero"""
        ia, ja = self.c.get_pattern()
        n = len(ia) - 1
        A = np.zeros((n, n))
        A[np.repeat(np.arange(n), np.diff(ia)), ja] = self.c.get_a()
        B = np.array([A[3 * v:3 * v + 3, 3 * v:3 * v + 3].copy() for v in range(n // 3)])
        for v in range(n // 3):
            A[3 * v:3 * v + 3, 3 * v:3 * v + 3] = 0.0
        return B, bool(np.any(A != 0.0))


@pytest.fixture(scope="module")
def carriers(gpu_lib):
    return {name: Carrier(gpu_lib, name) for name in NAMES}


def _check(got13, ref, tol, worst, bad, where):
    got13 = np.asarray(got13, dtype=np.float64)
    assert np.all(np.isfinite(got13)), where
    r = rc.ratio(got13 - ref, tol)
    for k, sl in (("E", slice(0, 1)), ("g", slice(1, 4)), ("H", slice(4, 13))):
        worst[k] = max(worst.get(k, 0.0), float(r[sl].max()))
        if not r[sl].max() <= rc.M:
            bad.append(f"{where} {k}: err / (sens + u scale) = {r[sl].max():.3g}")


def test_sets_energy_gradient_hessian_against_mpmath(carriers):
    worst, bad = {}, []
    for name, cr in carriers.items():
        c, idx = cr.c, cr.idx
        got = c.round_build(idx, rc.DHAT)
        assert got.tolist() == cr.want and 10 <= len(cr.want) < 40 and 2 not in cr.want, name  # (vertex 2: Dirichlet, inside dHat)
        refs = {v: rc.expected_vertex(cr.collider, cr.P[v], rc.DHAT, rc.KAPPA) for v in cr.want}
        E = c.round_energy(idx, rc.DHAT, rc.KAPPA)
        assert abs(E - sum(r[0][0] for r in refs.values())) <= rc.M * sum(r[1][0] for r in refs.values()), name
        g = c.round_gradient_add(idx, rc.DHAT, rc.KAPPA).reshape(-1, 3)
        c.set_zero()
        c.round_hessian_add(idx, rc.DHAT, rc.KAPPA, True)
        B, elsewhere = cr.blocks()
        assert not elsewhere
        for v in range(40):
            if v not in refs:
                assert np.all(g[v] == 0.0) and np.all(B[v] == 0.0), (name, v)
        Ev = {}
        for v in cr.want:  # the energy of one vertex: the set handed in through the ABI
            c.round_set(idx, [v])
            Ev[v] = c.round_energy(idx, rc.DHAT, rc.KAPPA)
        for v, (ref, tol) in refs.items():
            H = B[v]
            assert np.all(np.tril(H, -1) == 0.0)
            Hs = H + np.triu(H, 1).T
            _check(np.concatenate([[Ev[v]], g[v], Hs.ravel()]), ref, tol, worst, bad, f"{name} vertex {v}")
        # the projected Dirichlet rule: a set that holds the Dirichlet vertex writes its block only without projection
        c.round_set(idx, cr.want + [2])
        c.set_zero()
        c.round_hessian_add(idx, rc.DHAT, rc.KAPPA, True)
        assert np.all(cr.blocks()[0][2] == 0.0)
        c.set_zero()
        c.round_hessian_add(idx, rc.DHAT, rc.KAPPA, False)
        ref, tol = rc.expected_vertex(cr.collider, cr.P[2], rc.DHAT, rc.KAPPA)
        H = cr.blocks()[0][2]
        assert rc.ratio((H + np.triu(H, 1).T).ravel() - ref[4:], tol[4:]).max() <= rc.M and np.any(H != 0.0)
        c.round_build(idx, rc.DHAT)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {rc.M:g})")
    assert not bad, "\n".join(bad)


def test_hollow_sphere_keeps_the_curvature_term_and_solid_shapes_drop_it(carriers):
    """rank of the blocks: n n^T alone (rank 1) on a solid collider, n n^T plus the tangent plane (rank 3) inside a hollow sphere"""
    for name, cr in carriers.items():
        c = cr.c
        c.round_build(cr.idx, rc.DHAT)
        c.set_zero()
        c.round_hessian_add(cr.idx, rc.DHAT, rc.KAPPA, True)
        B = cr.blocks()[0]
        for v in cr.want:
            if not float(rc.evaluate(rc.MP, cr.collider, cr.P[v])[0]) < 0.095:  # (at the rim of dHat both coefficients vanish, the second one faster)
                continue
            H = B[v] + np.triu(B[v], 1).T
            ev = np.linalg.eigvalsh(H)
            assert ev[0] >= -1e-9 * ev[-1]
            assert int(np.sum(ev > 1e-9 * ev[-1])) == (3 if name == "hollow_sphere" else 1), (name, v, ev)


def test_step_bounds_against_the_mpmath_root(carriers):
    worst, bad = 0.0, []
    STEP = 16.0
    for name, cr in carriers.items():
        c = cr.c
        for x, p, label in rc.rays(name):
            P = cr.P.copy()
            P[0] = x
            c.set_positions(P)
            d = np.zeros((40, 3))
            d[0] = p
            got = c.round_step_bound(cr.idx, d, 0.9, STEP)
            t, tol = rc.expected_step(cr.collider, x, p, 0.9)
            if t is None or t - rc.M * tol > STEP:
                assert got == STEP, (name, label, got)
                continue
            r = float(rc.ratio(got - t, tol))
            worst = max(worst, r)
            if not r <= rc.M:
                bad.append(f"{name} {label}: t = {got!r}, mpmath {t!r}, err / (sens + u scale) = {r:.3g}")
            assert rc.gap_along_ray_mp(cr.collider, x, p, mpf(got)) > 0, (name, label)
        labels = [q[2] for q in rc.rays(name)]
        if not cr.collider["hollow"]:
            assert "miss" in labels and "away" in labels and "graze" in labels
        c.set_positions(cr.P)
    print(f"step bounds: worst err / (sens + u scale) = {worst:.3g} (M = {rc.M:g})")
    assert not bad, "\n".join(bad)


def test_a_dirichlet_node_does_not_bound_a_step_but_bounds_a_move(gpu_lib):
    cr = Carrier(gpu_lib, "solid_sphere")  # (its own context: the collider moves)
    c, col = cr.c, cr.collider
    c.set_positions(cr.P)
    towards = np.zeros((40, 3))
    towards[2] = np.array(col["p0"]) - cr.P[2]  # vertex 2 is a Dirichlet node: straight at the centre
    assert c.round_step_bound(cr.idx, towards, 0.9, 1.0) == 1.0
    # the collider moved against vertex 2: the relative ray of every surface node counts, Dirichlet or not
    u = cr.P[2] - np.array(col["p0"])
    gap2 = float(np.linalg.norm(u)) - col["R"]
    delta = 0.5 * u / np.linalg.norm(u)
    left = c.round_move(cr.idx, delta, 0.5)
    assert 0.0 < left < 1.0
    moved = c.round_get(cr.idx)
    travelled = float(np.linalg.norm(moved["p0"] - np.array(col["p0"])))
    assert travelled <= 0.5 * gap2 * (1 + 1e-12) and np.array_equal(moved["p0"], moved["p1"])
    st = c.round_state(cr.idx, rc.DHAT, rc.KAPPA)
    assert st["min_s"] > 0.0
    assert c.round_move(cr.idx, -(1.0 - left) * delta, 0.5) == 0.0  # away again: the whole move is taken
    c.close()


def test_friction_against_the_restatement_with_the_lagged_normal(carriers):
    worst, bad = {}, []
    rng = np.random.default_rng(7)
    for name, cr in carriers.items():
        c, idx = cr.c, cr.idx
        c.set_positions(cr.P)
        c.round_build(idx, rc.DHAT)
        c.set_round_collider_friction(idx, MU)
        assert c.round_lag_update(idx, rc.DHAT, rc.KAPPA) == len(cr.want)
        for speed, label in ((3e-2, "sliding"), (2e-4, "sticking")):
            x = cr.P + speed * rng.uniform(-1, 1, size=cr.P.shape)
            c.set_positions(x)
            refs = {v: rc.expected_friction(cr.collider, cr.P[v], rc.DHAT, rc.KAPPA, x[v], cr.P[v], MU, EPS2) for v in cr.want}
            E = c.round_friction_energy(idx, cr.P, EPS2)
            assert abs(E - sum(r[0][0] for r in refs.values())) <= rc.M * sum(r[1][0] for r in refs.values()), (name, label)
            g = c.round_friction_gradient_add(idx, cr.P, EPS2).reshape(-1, 3)
            c.set_zero()
            c.round_friction_hessian_add(idx, cr.P, EPS2, True)
            B, elsewhere = cr.blocks()
            assert not elsewhere
            nSlide = 0
            for v, (ref, tol) in refs.items():
                Hs = B[v] + np.triu(B[v], 1).T
                _check(np.concatenate([[ref[0]], g[v], Hs.ravel()]), ref, tol, worst, bad, f"{name} {label} vertex {v}")  # (the energy: checked in total above)
                n = np.array([float(q) for q in rc.lag(rc.MP, cr.collider, cr.P[v], rc.DHAT, rc.KAPPA)[1]])
                vp = (x[v] - cr.P[v]) - ((x[v] - cr.P[v]) @ n) * n
                nSlide += int(vp @ vp > EPS2)
            assert nSlide == (len(refs) if label == "sliding" else 0), (name, label, nSlide)
        c.set_positions(cr.P)
    print("friction: worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {rc.M:g})")
    assert not bad, "\n".join(bad)


def test_state_sums_the_gradient_and_repeats_to_the_bit(carriers):
    for name, cr in carriers.items():
        c, idx = cr.c, cr.idx
        c.set_positions(cr.P)
        c.round_build(idx, rc.DHAT)
        a, b = c.round_state(idx, rc.DHAT, rc.KAPPA), c.round_state(idx, rc.DHAT, rc.KAPPA)
        assert a["n"] == len(cr.want)
        for k in ("force", "torque", "friction"):
            assert np.array_equal(a[k], b[k])
        assert a["min_s"] == b["min_s"]
        g = c.round_gradient_add(idx, rc.DHAT, rc.KAPPA).reshape(-1, 3)
        scale = np.abs(g).sum()
        assert np.abs(a["force"] + g.sum(axis=0)).max() <= 64 * rc.U * scale
        arm = cr.P - np.array(cr.collider["p0"])
        assert np.abs(a["torque"] + np.cross(arm, g).sum(axis=0)).max() <= 64 * rc.U * np.abs(arm).max() * scale
        want = min(float(rc.evaluate(rc.MP, cr.collider, x)[0]) for x in cr.P)
        assert abs(a["min_s"] - want) <= 8 * rc.U * (cr.collider["R"] + np.abs(arm).max())


def test_entries_are_bit_identical_between_two_calls_and_two_contexts(gpu_lib, carriers):
    cr = carriers["capsule_skew"]
    other = Carrier(gpu_lib, "capsule_skew")
    out = []
    for q in (cr, cr, other):
        c = q.c
        c.set_positions(q.P)
        assert c.round_build(q.idx, rc.DHAT).tolist() == q.want
        c.set_zero()
        c.round_hessian_add(q.idx, rc.DHAT, rc.KAPPA, True)
        out.append((c.round_energy(q.idx, rc.DHAT, rc.KAPPA), c.round_gradient_add(q.idx, rc.DHAT, rc.KAPPA), c.get_a().copy(),
                    c.round_step_bound(q.idx, np.tile([0.3, -0.2, 0.1], 40), 0.9, 1.0)))
    for o in out[1:]:
        assert o[0] == out[0][0] and np.array_equal(o[1], out[0][1]) and np.array_equal(o[2], out[0][2]) and o[3] == out[0][3]
    other.c.close()
