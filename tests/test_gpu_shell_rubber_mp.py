"""The rubber-membrane kernels of the shells through the C ABI against the mpmath cases of shell_rubber_mp.py (tests/golden/shell_rubber_mp_cases.npz).  Every
case is one connected component of ONE carrier mesh without tetrahedra (node ranges side by side), so each case's energy terms, gradient rows and dense
block are its own; the tolerance is shell_rubber_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_shell_rubber_mp.py."""
import numpy as np
import pytest

import codim_common as cc
import shell_mp as smp
import shell_rubber_mp as rmp

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)
NO_T = np.zeros((0, 4), dtype=np.int32)


def dense_upper(c):
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A


class Carrier:
    def __init__(self, gpu_lib, cases, bend_scale=1.0):
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]).astype(int)
        # (the cases stay where they are, overlapping in space -- there is no contact here, only elasticity)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.tri = np.vstack([c["tri"] + o for c, o in zip(cases, self.off)]).astype(np.int32)
        self.triOwner = np.concatenate([np.full(len(c["tri"]), i) for i, c in enumerate(cases)])
        cat = lambda k: np.concatenate([c[k] for c in cases])
        self.dbc = cat("dbc")
        self.model, self.alpha, self.h = cat("model"), cat("alpha"), cat("h")
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, cat("h"), cat("YM"), cat("PR"), cat("rho"), bend_scale=bend_scale)
        c.set_shell_membrane(self.model, self.alpha)
        for typ in (1, 2):
            if np.any(self.dbc == typ):
                c.set_dbc(np.flatnonzero(self.dbc == typ), typ)
        c.opt_init(0.01, False)
        c.set_pattern()
        c.set_positions(self.x)
        c.set_xtilde(self.x)

    def finite_positions(self):
        """the carrier's positions with every case whose energy is +infinity put back to rest"""
        x = self.x.copy()
        for cs, o, e in zip(self.cases, self.off[:-1], self.off[1:]):
            if cs["E"] == np.inf:
                x[o:e] = cs["X"]
        return x


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, rmp.load())


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    m, a = c.shell_membrane_get()
    assert np.array_equal(m, carrier.model) and np.array_equal(a, np.where(carrier.model == 1, carrier.alpha, 0.0))
    perTri = c.shell_rubber_energy_per_elem()
    assert np.all(perTri[carrier.model == 0] == 0.0)
    assert sum(cs["E"] == np.inf for cs in cases) == 1  # the collinear case
    for coef in COEFS:
        assert c.shell_rubber_energy(coef) == np.inf  # the collinear case: +infinity, not NaN
        cc.compare(rmp, cases, "E", lambda i: coef * perTri[carrier.triOwner == i].sum(), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.shell_rubber_gradient_add(coef, proj)
            c.set_zero()
            c.shell_rubber_hessian_add(coef, proj)
            A = dense_upper(c)
            where = f"coef {coef:g} projectDBC {int(proj)}"
            # (the collinear case has tolerance 0: its gradient rows and its block stay exactly zero, and finite)
            cc.compare(rmp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(rmp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i in range(len(cases)):  # nothing between the components
                A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]] = 0.0
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {rmp.M:g})")
    assert not bad, "\n".join(bad)


def test_gradient_and_matrix_are_unchanged_by_a_collinear_triangle(carrier):
    """added to a vector and a matrix that already hold something: the entries of the collinear case come back bit for bit"""
    c, off = carrier.c, carrier.off
    i = [cs["name"] for cs in carrier.cases].index("exactly collinear, alpha 0.1")
    g0 = np.linspace(1.0, 2.0, 3 * len(carrier.X))
    g = c.shell_rubber_gradient_add(1.0, False, g0)
    assert np.array_equal(g[3 * off[i]:3 * off[i + 1]], g0[3 * off[i]:3 * off[i + 1]]) and np.all(np.isfinite(g))
    assert not np.array_equal(g, g0)
    ia, ja = c.get_pattern()
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    mine = (rows >= 3 * off[i]) & (rows < 3 * off[i + 1])  # the stored entries of the case's rows (its columns lie in the same range: a component of its own)
    a0 = np.linspace(-1.0, 3.0, len(ja))
    try:
        c.set_a(a0)
        c.shell_rubber_hessian_add(1.0, False)
        a = c.get_a()
    finally:
        c.set_zero()
    assert mine.sum() >= 45 and np.array_equal(a[mine], a0[mine]) and np.all(np.isfinite(a))
    assert not np.array_equal(a, a0)


def test_finite_total_energy_against_mpmath(carrier):
    c, cases = carrier.c, carrier.cases
    c.set_positions(carrier.finite_positions())
    try:
        for coef in COEFS:
            fin = [cs for cs in cases if cs["E"] != np.inf]
            E = c.shell_rubber_energy(coef)
            want, tol = sum(rmp.expected(cs, "E", coef)[0] for cs in fin), sum(rmp.expected(cs, "E", coef)[1] for cs in fin)
            print(f"coef {coef:g}: total {E:.17g}, mpmath {want:.17g}, err / tol {abs(E - want) / tol:.3g}")
            assert abs(E - want) <= tol
    finally:
        c.set_positions(carrier.x)


def test_thickness_is_h_over_the_area_stretch(carrier):
    c = carrier.c
    sigma, _ = c.shell_stretch()  # (pinned against mpmath by test_gpu_shell_limit_mp.py)
    with np.errstate(divide="ignore"):
        want = np.where(carrier.model == 1, carrier.h / (sigma[:, 0] * sigma[:, 1]), carrier.h)
    got = c.shell_thickness()
    assert np.array_equal(got, want)
    assert np.isinf(want).sum() == 1 and np.all(want[carrier.model == 0] == carrier.h[carrier.model == 0])
    i = [cs["name"] for cs in carrier.cases].index("biaxial stretch 2, alpha 0")
    assert abs(got[carrier.triOwner == i][0] / carrier.h[0] - 0.25) <= 64 * rmp.U  # a sheet stretched 2 x 2 goes to a quarter


def test_stvk_and_rubber_triangle_side_by_side(gpu_lib):
    """two triangles sharing an edge, one StVK and one rubber, in their plane and with `bend 0` (the hinge adds exact zeros): ipcgpu_shell_energy,
    _gradient_add and _hessian_add are the StVK restatement of the first (shell_mp) plus the rubber restatement of the second, and the rubber triangle
    carries no StVK energy"""
    case = {cs["name"]: cs for cs in rmp.load()}["StVK and rubber triangle sharing an edge"]
    car = Carrier(gpu_lib, [case], bend_scale=0.0)
    c = car.c
    nodes = case["tri"][0]
    stvk = smp.evaluate(smp._case("StVK triangle", case["X"][nodes], case["x"][nodes], [[0, 1, 2]], h=case["h"][0], YM=case["YM"][0], PR=case["PR"][0]))
    idx = np.array([3 * v + i for v in nodes for i in range(3)])
    perTri, perHinge = c.shell_energy_per_elem()
    assert perTri[1] == 0.0 and perTri[0] > 0.0 and np.all(perHinge == 0.0)
    assert abs(perTri[0] - stvk["E"]) <= smp.tolerance(stvk, "E")
    rub = c.shell_rubber_energy_per_elem()
    assert rub[0] == 0.0 and rub[1] > 0.0
    for coef in COEFS:
        E = c.shell_energy(coef)
        want, tol = coef * stvk["E"] + rmp.expected(case, "E", coef)[0], smp.tolerance(stvk, "E", coef) + rmp.expected(case, "E", coef)[1]
        print(f"coef {coef:g}: shell energy {E:.17g}, StVK + rubber restatements {want:.17g}, err / tol {abs(E - want) / tol:.3g}")
        assert abs(E - want) <= tol
        assert c.shell_rubber_energy(coef) == coef * rub[1]
        g = c.shell_gradient_add(coef, False)
        gw, gt = rmp.expected(case, "g", coef, False)
        gw[idx] += coef * stvk["g"]
        gt[idx] += smp.tolerance(stvk, "g", coef)
        assert np.all(np.abs(g - gw) <= gt)
        c.set_zero()
        c.shell_hessian_add(coef, False)
        A = dense_upper(c)
        Hw, Ht = rmp.expected(case, "H", coef, False)
        Hw[np.ix_(idx, idx)] += coef * stvk["H"]
        Ht[np.ix_(idx, idx)] += smp.tolerance(stvk, "H", coef)
        assert np.all(np.abs(A - np.triu(Hw)) <= np.triu(Ht))
    # the stepper's assembly carries the term: with it minus the rubber term alone = the StVK triangle alone
    coef = COEFS[1]
    g = c.assemble_newton(coef, True, with_gradient=True)
    a = c.get_a()
    gl = c.shell_rubber_gradient_add(coef, True)
    c.set_zero()
    c.shell_rubber_hessian_add(coef, True)
    al = c.get_a()
    c.set_zero()
    c.shell_hessian_add(coef, True)
    asl = c.get_a()
    assert np.abs(al).max() > 0 and np.abs(gl).max() > 0
    gs = c.shell_gradient_add(coef, True)
    assert np.abs(c.gradient(coef, True) - g).max() <= 64 * rmp.U * np.abs(g).max()
    # (xTilde = x: the inertia term adds the masses to the diagonal and nothing to the gradient)
    assert np.abs(g - gs).max() <= 64 * rmp.U * np.abs(gs).max()
    off = np.abs(a - asl) > 64 * rmp.U * np.abs(asl).max()
    ia, ja = c.get_pattern()
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    assert np.all(rows[off] == ja[off])  # the two assemblies differ on the diagonal only: the masses


def test_strip_with_one_rubber_triangle_more_than_a_block(gpu_lib):
    """2 x 130 nodes, 258 triangles, the first 257 rubber (256 + 1: the tail lanes of the energy kernels and of the 64-wide assemble kernel), the last StVK.  Every
    coordinate is dyadic, so each up / down triangle has bit for bit the edge vectors of the stored single triangle: the reference is those two cases assembled"""
    st = {cs["name"]: cs for cs in rmp.load()}
    up, dn = st["strip, up triangle"], st["strip, down triangle"]
    V, tri = smp.grid(130, 2, spacing=rmp.STRIP_H)
    assert len(tri) == 258 and np.array_equal(V[tri[0]], up["X"]) and np.array_equal(V[tri[1]], dn["X"])
    x = V @ rmp.STRIP_MAP.T
    model = np.ones(len(tri), dtype=np.int32)
    model[-1] = 0
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_shell(tri, up["h"][0], up["YM"][0], 0.3, 1000.0, bend_scale=1.0)
    c.set_shell_membrane(model, up["alpha"][0])
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_positions(x)
    n3 = 3 * len(V)
    coef = COEFS[1]
    Ew = Et = 0.0
    gw, gt, Hw, Ht = np.zeros(n3), np.zeros(n3), np.zeros((n3, n3)), np.zeros((n3, n3))
    for t in range(257):
        cs = dn if t % 2 else up
        idx = np.array([3 * v + i for v in tri[t] for i in range(3)])
        Ew, Et = Ew + rmp.expected(cs, "E", coef)[0], Et + rmp.expected(cs, "E", coef)[1]
        gw[idx] += rmp.expected(cs, "g", coef)[0]
        gt[idx] += rmp.expected(cs, "g", coef)[1]
        Hw[np.ix_(idx, idx)] += rmp.expected(cs, "H", coef)[0]
        Ht[np.ix_(idx, idx)] += rmp.expected(cs, "H", coef)[1]
    perTri = c.shell_rubber_energy_per_elem()
    assert perTri[-1] == 0.0 and len(set(perTri[0:257:2])) == 1 and len(set(perTri[1:257:2])) == 1 and perTri[256] > 0.0
    E = c.shell_rubber_energy(coef)
    g = c.shell_rubber_gradient_add(coef, True)
    c.set_zero()
    c.shell_rubber_hessian_add(coef, True)
    A = dense_upper(c)
    print(f"strip: energy err / tol {abs(E - Ew) / Et:.3g}, gradient {np.max(np.abs(g - gw) / gt):.3g}, "
          f"matrix {np.max(rmp.ratio(A - np.triu(Hw), np.triu(Ht))):.3g} of the tolerance")
    assert abs(E - Ew) <= Et
    assert np.all(np.abs(g - gw) <= gt)
    assert np.all(np.abs(A - np.triu(Hw)) <= np.triu(Ht))
    assert np.any(g[-3:] != 0.0)  # the last node belongs to the last rubber triangle (256) as well as to the StVK one
