"""The pressure-chamber kernels through the C ABI against the mpmath cases of chamber_mp.py (tests/golden/chamber_mp_cases.npz).  Every case is a node range
and a chamber of its own in ONE carrier mesh without tetrahedra (ranges side by side), so each case's energy terms, gradient rows and dense block are its
own.  One triangle of the tetrahedron case is also a one-triangle shell, so the pattern comes from two sources (shell and chamber pairs); a single shell
triangle has one addend per matrix entry, which keeps what the shell adds free of any summation order.  The tolerance is
chamber_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_chamber_mp.py."""
import numpy as np
import pytest
from mpmath import mpf

import chamber_mp as cm
import codim_common as cc

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)
SHELL_ON = ("tetrahedron", 3)  # (case, its triangle)


class Carrier:
    def __init__(self, gpu_lib, cases, shell_on=SHELL_ON):
        self.cases = cases
        self.off = off = np.concatenate([[0], np.cumsum([len(c["x"]) for c in cases])]).astype(int)
        # (a rigid shift would change the stored inputs: the cases stay where they are, overlapping in space -- there is no contact here).  The rest
        # positions are the current ones: the rest reference point of every chamber is the one its case stores, and the shell triangle is at rest
        self.x = np.vstack([c["x"] for c in cases])
        self.dbc = np.concatenate([c["dbc"] for c in cases])
        self.tris = [np.asarray(c["tri"], dtype=np.int32) + o for c, o in zip(cases, off)]
        self.p = np.array([c["p"] for c in cases])
        self.owner = np.concatenate([np.full(len(t), i) for i, t in enumerate(self.tris)])
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.x, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
        if shell_on is not None:
            by = {cs["name"]: i for i, cs in enumerate(cases)}
            self.shell = self.tris[by[shell_on[0]]][shell_on[1]][None, :]
            c.set_shell(self.shell, 1e-3, 1e5, 0.3, 1000.0)
        c.set_chambers(self.tris, self.p)
        for typ in (1, 2):
            if np.any(self.dbc == typ):
                c.set_dbc(np.flatnonzero(self.dbc == typ), typ)
        c.opt_init(0.01, False)
        c.set_pattern()
        c.set_positions(self.x)
        c.set_xtilde(self.x)

    def dense_upper(self):
        ia, ja = self.c.get_pattern()
        A = np.zeros((len(ia) - 1, len(ia) - 1))
        A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = self.c.get_a()
        return A


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, cm.load())


def test_reference_point_is_the_stored_one(carrier):
    r = carrier.c.chamber_state()[2]
    for i, cs in enumerate(carrier.cases):
        assert np.all(np.abs(r[i] - cs["r"]) <= 4 * cm.U * np.linalg.norm(cs["r"])), cs["name"]
        assert np.array_equal(r[i], cs["r"]), cs["name"]  # (in fact to the bit: the plan sums in the order chamber_mp.ref_point restates)


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    per = c.chamber_energy_per_elem()
    assert np.all(np.isfinite(per))
    for i, cs in enumerate(cases):  # the per-triangle terms one by one: each within its case's energy tolerance
        assert np.all(np.abs(per[carrier.owner == i] - cs["perE"]) <= cm.expected(cs, "E")[1]), cs["name"]
    for coef in COEFS:
        Eall = c.chamber_energy(coef)
        Esum = sum(cm.expected(cs, "E", coef)[0] for cs in cases)
        print(f"coef {coef:g}: total energy {Eall!r}, reference {Esum!r}, tolerance {sum(cm.expected(cs, 'E', coef)[1] for cs in cases):.3g}")
        assert abs(Eall - Esum) <= sum(cm.expected(cs, "E", coef)[1] for cs in cases)
        cc.compare(cm, cases, "E", lambda i: coef * per[carrier.owner == i].sum(), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.chamber_gradient_add(coef, proj)
            c.set_zero()
            c.chamber_hessian_add(coef, proj)
            A = carrier.dense_upper()
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(cm, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(cm, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert dropped.any() and np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i, cs in enumerate(cases):
                s = slice(3 * off[i], 3 * off[i + 1])
                if cs["p"] == 0.0:  # an unpressurised chamber writes nothing at all
                    assert np.all(g[s] == 0.0) and np.all(A[s, s] == 0.0)
                A[s, s] = 0.0  # ... and nothing between the cases
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {cm.M:g})")
    assert not bad, "\n".join(bad)


def test_newton_assembly_adds_the_chambers_to_mass_inertia_and_shell(carrier):
    """ipcgpu_assemble_newton / ipcgpu_gradient / ipcgpu_incremental_potential on the same state.  The shell triangle is at rest and single (one addend
    per entry: no summation order), so what it adds is taken off with its own entry points: a matrix entry holds fl(fl(m + s) + h) -- mass or identity
    m, shell s, chamber h -- and those two roundings, at most u (|m + s| + |m + s + h|), are no part of the chamber Hessian's tolerance and are taken off
    before measuring (as test_gpu_attach_mp.py does)."""
    c, cases, off = carrier.c, carrier.cases, carrier.off
    coef = COEFS[1]
    mass = c.features()["mass"]
    for proj in (True, False):
        g = c.assemble_newton(coef, proj, with_gradient=True)
        A = carrier.dense_upper()
        g2 = c.gradient(coef, proj)
        gOther = c.shell_gradient_add(coef, proj)
        c.set_zero()
        c.shell_hessian_add(coef, proj)
        Sm = carrier.dense_upper()
        dropped = (carrier.dbc == 1) | ((carrier.dbc == 2) & proj)
        Sm += np.diag(np.repeat(np.where(dropped, 1.0, mass), 3))
        H = A - Sm
        slack = cm.U * (np.abs(Sm) + np.abs(A))
        worst, bad = {}, []
        cc.compare(cm, cases, "g", lambda i: (g - gOther)[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "assemble_newton")
        cc.compare(cm, cases, "g", lambda i: (g2 - gOther)[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "gradient")

        def block(i):
            s = slice(3 * off[i], 3 * off[i + 1])
            ref = np.triu(cm.expected(cases[i], "H", coef, proj)[0])
            err = H[s, s] - ref
            return ref + np.sign(err) * np.maximum(np.abs(err) - slack[s, s], 0.0)
        cc.compare(cm, cases, "H", block, coef, proj, worst, bad, "assemble_newton")
        assert not bad, "\n".join(bad)
    E = c.incremental_potential(coef)
    want = sum(cm.expected(cs, "E", coef)[0] for cs in cases) + c.shell_energy(coef)
    assert abs(E - want) <= sum(cm.expected(cs, "E", coef)[1] for cs in cases)  # (xTilde = x: no inertia term)


def _state_bounds(m, volMag, areaMag):
    """Bounds of chamber_state from its arithmetic, for a chamber of m triangles.  y_k = fl(x_k - r') carries u |y_k|.  The triple product is six products of
    three factors (3 u from the y, 2 u from the two multiplications) joined by five additions (at most 3 u on any path): 8 u on each term, and the six
    terms' magnitudes sum to at most |y0|_1 |y1|_1 |y2|_1 <= 3 sqrt(3) |y0| |y1| |y2|: 42 u m_t with m_t = |y0| |y1| |y2|.  The lanes stride over the range
    and a tree of 8 levels follows: no partial sum sees more than d = ceil(m / 256) + 8 additions, d u sum_t |triple_t| <= d u sum m_t; the division by 6
    adds one more rounding.  Area: an edge e = fl(y_i - y_j) carries at most 2 u S_t, S_t = |y0| + |y1| + |y2| >= |e|; the cross product of two edges
    then carries 2 (2 u S_t) S_t + 4 u S_t^2 (its own three roundings per entry, generously), the norm and the square root u S_t^2 more, and the half
    halves it: 4.5 u S_t^2 per triangle, plus d u A <= d u sum S_t^2 / 2 from the summation and one rounding of the product with 0.5.
    r' (the centroid mean of the current positions) differs from the stored r by roundings only; the factor 1.01 covers what that does to m_t and S_t."""
    d = -(-m // 256) + 8
    return 1.01 * cm.U * (42 + d + 1) * volMag / 6.0, 1.01 * cm.U * (4.5 + d / 2.0 + 1) * areaMag


def test_state_and_get_against_mpmath(carrier):
    c, cases = carrier.c, carrier.cases
    V, A, r = c.chamber_state()
    info = c.chamber_get()
    assert info["n"] == len(cases) and info["nTri"] == len(carrier.owner)
    assert np.array_equal(info["tri"], np.vstack(carrier.tris)) and np.array_equal(info["triEnd"], np.cumsum([len(t) for t in carrier.tris]))
    assert np.array_equal(info["pressure"], carrier.p)
    worst = 0.0
    for i, cs in enumerate(cases):
        tv, ta = _state_bounds(len(cs["tri"]), cs["volMag"], cs["areaMag"])
        worst = max(worst, abs(V[i] - cs["vol"]) / tv, abs(A[i] - cs["area"]) / ta)
        assert abs(V[i] - cs["vol"]) <= tv and abs(A[i] - cs["area"]) <= ta, cs["name"]
        assert abs(info["restVolume"][i] - cs["vol"]) <= tv  # (the rest positions of the carrier are the current ones)
        assert info["restVolume"][i] == cm.rest_volume(cs["x"], cs["tri"], cs["r"])  # the plan's documented order, to the bit
    print(f"worst error of volume and area over its bound: {worst:.3g}")


def test_pattern_holds_every_block_of_the_reference_matrix(carrier):
    ia, ja = carrier.c.get_pattern()
    P = np.zeros((len(ia) - 1, len(ia) - 1), dtype=bool)
    P[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = True
    for cs, o, e in zip(carrier.cases, carrier.off[:-1], carrier.off[1:]):
        full = np.array(cm.reference(cm.NP, dict(cs, p=1.0))[2], dtype=np.float64)  # (projected: the diagonal blocks are there too)
        assert np.all(P[3 * o:3 * e, 3 * o:3 * e][np.triu(np.abs(full) > 0.0)]), cs["name"]


def box_surface(na, nb, nc, size, lo, jitter, seed):
    """the closed, outward-oriented surface of a box of na x nb x nc cells: 4 (na nb + nb nc + nc na) triangles over the grid's boundary nodes"""
    idx = lambda i, j, k: (i * (nb + 1) + j) * (nc + 1) + k
    P = np.array([[i, j, k] for i in range(na + 1) for j in range(nb + 1) for k in range(nc + 1)], dtype=np.float64)
    centre = np.array([na, nb, nc]) / 2.0
    tri = []
    for axis, n in enumerate((na, nb, nc)):
        o1, o2 = [a for a in range(3) if a != axis]
        dims = (na, nb, nc)
        for side in (0, n):
            for u in range(dims[o1]):
                for v in range(dims[o2]):
                    def node(du, dv):
                        q = [0, 0, 0]
                        q[axis], q[o1], q[o2] = side, u + du, v + dv
                        return idx(*q)
                    for t in ((node(0, 0), node(1, 0), node(1, 1)), (node(0, 0), node(1, 1), node(0, 1))):
                        nrm = np.cross(P[t[1]] - P[t[0]], P[t[2]] - P[t[0]])
                        tri.append(t if nrm @ (P[list(t)].mean(axis=0) - centre) > 0 else (t[0], t[2], t[1]))
    used = np.unique(np.array(tri))
    remap = -np.ones(len(P), dtype=np.int64)
    remap[used] = np.arange(len(used))
    X = P[used] * size + np.asarray(lo) + jitter * size * (np.random.default_rng(seed).random((len(used), 3)) - 0.5)
    return X, remap[np.array(tri)].astype(np.int32)


def test_segmented_reduction_across_a_lane_boundary_and_a_tiny_chamber_behind_a_large_one(gpu_lib):
    """two chambers of 260 and 4 triangles in that order: the first strides past the 256 lanes of its workgroup, the second uses four of them"""
    X, T = box_surface(5, 5, 4, 0.05, [0.1, 0.2, 0.3], 0.2, 5)
    assert len(T) == 260
    tet = cm.TET_X * 0.2 + [0.6, 0.1, 0.1]
    cases = [{"name": "box", "x": X, "tri": T, "p": np.float64(700.0), "dbc": np.zeros(len(X), dtype=np.int32)},
             {"name": "tet", "x": tet, "tri": cm.TET_TRI, "p": np.float64(-300.0), "dbc": np.zeros(4, dtype=np.int32)}]
    for cs in cases:
        cs["r"] = cm.ref_point(cs["x"], cs["tri"])
    car = Carrier(gpu_lib, cases, shell_on=None)
    V, A, r = car.c.chamber_state()
    info = car.c.chamber_get()
    per = car.c.chamber_energy_per_elem()
    Etot = car.c.chamber_energy(1.0)
    for i, cs in enumerate(cases):
        assert np.array_equal(r[i], cs["r"])
        Vm, Am, m3, m2 = cm.volume_area(cs)
        tv, ta = _state_bounds(len(cs["tri"]), float(m3), float(m2))
        print(f"{cs['name']}: volume error {float(abs(mpf(float(V[i])) - Vm)) / tv:.3g}, area error {float(abs(mpf(float(A[i])) - Am)) / ta:.3g} of the bound")
        assert abs(mpf(float(V[i])) - Vm) <= tv and abs(mpf(float(A[i])) - Am) <= ta
        assert info["restVolume"][i] == cm.rest_volume(cs["x"], cs["tri"], cs["r"])
        # the per-triangle energies sum to -p V: each carries the 42 u m_t of the triple product (and the scaling by p / 6: 2 u more)
        assert abs(mpf(float(per[car.owner == i].sum())) + mpf(float(cs["p"])) * Vm) <= abs(cs["p"]) * cm.U * (44 + len(cs["tri"])) * float(m3) / 6.0
    assert abs(Etot - per.sum()) <= cm.U * (len(per) + 16) * np.abs(per).sum()
