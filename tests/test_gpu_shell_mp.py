"""The shell kernels through the C ABI against the mpmath cases of shell_mp.py (tests/golden/shell_mp_cases.npz).  Every case is one connected component of
ONE carrier mesh without tetrahedra (node ranges side by side), so each case's energy terms, gradient rows and dense block are its own; the tolerance is
shell_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_shell_mp.py."""
import numpy as np
import pytest

import codim_common as cc
import shell_mp as smp

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)


class Carrier:
    def __init__(self, gpu_lib, cases):
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]).astype(int)
        # (a rigid shift would change the stored inputs: the cases stay where they are, overlapping in space -- there is no contact here, only elasticity)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.tri = np.vstack([c["tri"] + o for c, o in zip(cases, self.off)]).astype(np.int32)
        cat = lambda k: np.concatenate([c[k] for c in cases])
        self.dbc = cat("dbc")
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, np.zeros((0, 4), dtype=np.int32), YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, cat("h"), cat("YM"), cat("PR"), cat("rho"), bend_scale=1.0)
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

    def pattern_mask(self):
        ia, ja = self.c.get_pattern()
        P = np.zeros((len(ia) - 1, len(ia) - 1), dtype=bool)
        P[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = True
        return P


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, smp.load())


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    perTri, perHinge = c.shell_energy_per_elem()
    hinges = c.shell_get()["hinges"]
    triOwner = np.searchsorted(off, carrier.tri[:, 0], side="right") - 1
    hingeOwner = np.searchsorted(off, hinges[:, 0], side="right") - 1
    for coef in COEFS:
        Eall = c.shell_energy(coef)
        Esum = sum(smp.expected(cs, "E", coef)[0] for cs in cases)
        assert abs(Eall - Esum) <= sum(smp.expected(cs, "E", coef)[1] for cs in cases)
        cc.compare(smp, cases, "E", lambda i: coef * (perTri[triOwner == i].sum() + perHinge[hingeOwner == i].sum()), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.shell_gradient_add(coef, proj)
            c.set_zero()
            c.shell_hessian_add(coef, proj)
            A = carrier.dense_upper()
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(smp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(smp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i in range(len(cases)):  # nothing between the components
                A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]] = 0.0
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {smp.M:g})")
    assert not bad, "\n".join(bad)


def test_newton_assembly_adds_the_shell_terms_to_mass_and_inertia(carrier):
    """ipcgpu_assemble_newton / ipcgpu_gradient / ipcgpu_incremental_potential on the same state: mass (or identity) on the diagonal plus the shell blocks"""
    c, cases, off = carrier.c, carrier.cases, carrier.off
    coef = COEFS[1]
    mass = c.shell_get()["mass"]
    for proj in (True, False):
        g = c.assemble_newton(coef, proj, with_gradient=True)
        A = carrier.dense_upper()
        dropped = (carrier.dbc == 1) | ((carrier.dbc == 2) & proj)
        D = np.repeat(np.where(dropped, 1.0, mass), 3)
        g2 = c.gradient(coef, proj)
        worst, bad = {}, []
        cc.compare(smp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "assemble_newton")
        cc.compare(smp, cases, "g", lambda i: g2[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "gradient")
        # the diagonal holds fl(m + H_ii): that one rounding, u (m + |H_ii|), is not part of the Hessian's tolerance and is taken off before measuring
        H = A - np.diag(D)
        slack = np.diag(2 * smp.U * np.maximum(D, np.abs(np.diag(H))))
        def block(i):
            s = slice(3 * off[i], 3 * off[i + 1])
            ref = np.triu(smp.expected(cases[i], "H", coef, proj)[0])
            err = H[s, s] - ref
            return ref + np.sign(err) * np.maximum(np.abs(err) - slack[s, s], 0.0)
        cc.compare(smp, cases, "H", block, coef, proj, worst, bad, "assemble_newton")
        assert not bad, "\n".join(bad)
    E = c.incremental_potential(coef)
    want = sum(smp.expected(cs, "E", coef)[0] for cs in cases)
    assert abs(E - want) <= sum(smp.expected(cs, "E", coef)[1] for cs in cases)  # (xTilde = x: no inertia term)


def test_shell_get_matches_the_reference_constants(carrier):
    info = carrier.c.shell_get()
    assert info["nTri"] == len(carrier.tri)
    want_h, want_rest, want_w, want_area = [], [], [], []
    mass = np.zeros(len(carrier.X))
    for cs, o in zip(carrier.cases, carrier.off):
        X = cs["X"].tolist()
        for t, tri in enumerate(cs["tri"]):
            _, A = smp.rest_triangle(smp.NP, [X[v] for v in tri])
            want_area.append(A)
            mass[tri + o] += cs["rho"][t] * cs["h"][t] * A / 3
        for (v0, v1, v2, v3, ta, tb) in smp.hinges_of(cs["tri"]):
            th, w, _ = smp.hinge_constants(smp.NP, [X[v] for v in (v0, v1, v2, v3)], [(cs["h"][t], cs["YM"][t], cs["PR"][t]) for t in (ta, tb)])
            want_h.append([v0 + o, v1 + o, v2 + o, v3 + o])
            want_rest.append(th)
            want_w.append(w)
    assert info["nHinge"] == len(want_h) and np.array_equal(info["hinges"], np.array(want_h))
    assert np.allclose(info["restAngle"], want_rest, rtol=0, atol=1e-14)
    assert np.allclose(info["hingeWeight"], want_w, rtol=1e-13, atol=0)
    assert np.allclose(info["area"], want_area, rtol=1e-13, atol=0)
    assert np.allclose(info["mass"], mass, rtol=1e-13, atol=0)


def test_pattern_holds_every_block_of_the_reference_matrix(carrier):
    P = carrier.pattern_mask()
    for cs, o, e in zip(carrier.cases, carrier.off[:-1], carrier.off[1:]):
        nz = np.triu(np.abs(cs["H"]) > 0.0)
        assert np.all(P[3 * o:3 * e, 3 * o:3 * e][nz]), cs["name"]
