"""The strain-limit kernels of the shells through the C ABI against the mpmath cases of shell_limit_mp.py (tests/golden/shell_limit_mp_cases.npz).  Every
case is one connected component of ONE carrier mesh without tetrahedra (node ranges side by side), so each case's energy terms, gradient rows and dense
block are its own; the tolerance is shell_limit_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_shell_limit_mp.py."""
import numpy as np
import pytest

import codim_common as cc
import shell_limit_mp as lmp

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)
NO_T = np.zeros((0, 4), dtype=np.int32)


class Carrier:
    def __init__(self, gpu_lib, cases, limited=True):
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]).astype(int)
        # (the cases stay where they are, overlapping in space -- there is no contact here, only elasticity)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.tri = np.vstack([c["tri"] + o for c, o in zip(cases, self.off)]).astype(np.int32)
        self.triOwner = np.concatenate([np.full(len(c["tri"]), i) for i, c in enumerate(cases)])
        cat = lambda k: np.concatenate([c[k] for c in cases])
        self.dbc = cat("dbc")
        self.limit, self.onset, self.stiff = cat("limit"), cat("onset"), cat("stiff")
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, cat("h"), cat("YM"), cat("PR"), cat("rho"), bend_scale=1.0)
        if limited:
            c.set_shell_strain_limit(self.limit, self.onset, self.stiff)
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

    def finite_positions(self):
        """the carrier's positions with every case whose energy is +infinity put back to rest"""
        x = self.x.copy()
        for cs, o, e in zip(self.cases, self.off[:-1], self.off[1:]):
            if cs["E"] == np.inf:
                x[o:e] = cs["X"]
        return x


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, lmp.load())


@pytest.fixture(scope="module")
def unlimited(gpu_lib):
    return Carrier(gpu_lib, lmp.load(), limited=False)


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    perTri = c.shell_limit_energy_per_elem()
    assert np.all(perTri[carrier.limit == 0] == 0.0)
    for coef in COEFS:
        assert c.shell_limit_energy(coef) == np.inf  # the case over its limit: +infinity, not NaN
        cc.compare(lmp, cases, "E", lambda i: coef * perTri[carrier.triOwner == i].sum(), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.shell_limit_gradient_add(coef, proj)
            c.set_zero()
            c.shell_limit_hessian_add(coef, proj)
            A = carrier.dense_upper()
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(lmp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(lmp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i in range(len(cases)):  # nothing between the components
                A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]] = 0.0
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {lmp.M:g})")
    assert not bad, "\n".join(bad)


def test_finite_total_energy_against_mpmath(carrier):
    c, cases = carrier.c, carrier.cases
    c.set_positions(carrier.finite_positions())
    try:
        for coef in COEFS:
            fin = [cs for cs in cases if cs["E"] != np.inf]
            E = c.shell_limit_energy(coef)
            want, tol = sum(lmp.expected(cs, "E", coef)[0] for cs in fin), sum(lmp.expected(cs, "E", coef)[1] for cs in fin)
            print(f"coef {coef:g}: total {E:.17g}, mpmath {want:.17g}, err / tol {abs(E - want) / tol:.3g}")
            assert abs(E - want) <= tol
    finally:
        c.set_positions(carrier.x)


def test_shell_entry_points_are_membrane_plus_bending_plus_limit(carrier, unlimited):
    """ipcgpu_shell_energy / _gradient_add / _hessian_add with a limit set against the same calls of a second context on the same mesh without a limit plus
    the limit term alone: 64 u of the largest magnitude (different summation orders of the atomics)"""
    c, c0 = carrier.c, unlimited.c
    coef = COEFS[1]
    for proj in (True, False):
        g, g0, gl = c.shell_gradient_add(coef, proj), c0.shell_gradient_add(coef, proj), c.shell_limit_gradient_add(coef, proj)
        assert np.abs(gl).max() > 0 and np.abs(g - (g0 + gl)).max() <= 64 * lmp.U * max(np.abs(g0).max(), np.abs(gl).max())
        vals = []
        for ctx, calls in ((c, ("shell_hessian_add",)), (c0, ("shell_hessian_add",)), (c, ("shell_limit_hessian_add",))):
            ctx.set_zero()
            for name in calls:
                getattr(ctx, name)(coef, proj)
            vals.append(ctx.get_a())
        a, a0, al = vals
        print(f"projectDBC {int(proj)}: gradient {np.abs(g - (g0 + gl)).max() / max(np.abs(g0).max(), np.abs(gl).max()) / lmp.U:.3g} u, "
              f"matrix {np.abs(a - (a0 + al)).max() / max(np.abs(a0).max(), np.abs(al).max()) / lmp.U:.3g} u of the largest magnitude")
        assert np.abs(al).max() > 0 and np.abs(a - (a0 + al)).max() <= 64 * lmp.U * max(np.abs(a0).max(), np.abs(al).max())
    assert c.shell_energy(coef) == np.inf and np.isfinite(c0.shell_energy(coef))
    xf = carrier.finite_positions()
    c.set_positions(xf)
    c0.set_positions(xf)
    try:
        E, E0, El = c.shell_energy(coef), c0.shell_energy(coef), c.shell_limit_energy(coef)
        assert El > 0 and abs(E - (E0 + El)) <= 64 * lmp.U * max(E0, El)
        assert abs(c.incremental_potential(coef) - c0.incremental_potential(coef) - El) <= 64 * lmp.U * max(E0, El)  # (xTilde = x up to the rest case: the same inertia term)
    finally:
        c.set_positions(carrier.x)
        c0.set_positions(carrier.x)


def test_stretches_against_mpmath_and_the_exact_maximum(carrier, unlimited):
    sigma, ratio = carrier.c.shell_stretch()
    ref = np.vstack([cs["sigma"] for cs in carrier.cases])
    rel = lmp.ratio(sigma - ref, np.abs(ref))
    print(f"worst relative error of a stretch: {rel.max() / lmp.U:.3g} u")
    assert np.all(np.abs(sigma - ref) <= 8 * lmp.U * np.abs(ref))
    lim = carrier.limit > 0
    assert ratio == np.max(sigma[lim, 0] / carrier.limit[lim]) and ratio > 1.0  # (the case over its limit)
    s0, r0 = unlimited.c.shell_stretch()
    assert np.array_equal(s0, sigma) and r0 == 0.0  # works without a limit; no limited triangle: 0


def test_newton_assembly_carries_the_limit_term(carrier, unlimited):
    """ipcgpu_assemble_newton and ipcgpu_gradient through the stepper's shell terms: with the limit minus without = the limit term alone"""
    c, c0 = carrier.c, unlimited.c
    coef = COEFS[1]
    g, g0 = c.assemble_newton(coef, True, with_gradient=True), c0.assemble_newton(coef, True, with_gradient=True)
    a, a0 = c.get_a(), c0.get_a()
    gl = c.shell_limit_gradient_add(coef, True)
    c.set_zero()
    c.shell_limit_hessian_add(coef, True)
    al = c.get_a()
    assert np.abs(g - g0 - gl).max() <= 64 * lmp.U * max(np.abs(g0).max(), np.abs(gl).max())
    assert np.abs(a - a0 - al).max() <= 64 * lmp.U * max(np.abs(a0).max(), np.abs(al).max())
    assert np.abs(c.gradient(coef, True) - c0.gradient(coef, True) - gl).max() <= 64 * lmp.U * max(np.abs(g0).max(), np.abs(gl).max())
