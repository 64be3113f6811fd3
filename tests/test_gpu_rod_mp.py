"""The rod kernels through the C ABI against the mpmath cases of rod_mp.py (tests/golden/rod_mp_cases.npz).  Every case is one connected component of ONE
carrier mesh without tetrahedra (node ranges side by side), so each case's energy terms, gradient rows and dense block are its own; the tolerance is
rod_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_rod_mp.py."""
import numpy as np
import pytest

import codim_common as cc
import rod_mp as rmp

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)


class Carrier:
    def __init__(self, gpu_lib, cases):
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]).astype(int)
        # (a rigid shift would change the stored inputs: the cases stay where they are, overlapping in space -- there is no contact here, only elasticity)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.seg = np.vstack([c["seg"] + o for c, o in zip(cases, self.off)]).astype(np.int32)
        cat = lambda k: np.concatenate([c[k] for c in cases])
        self.dbc = cat("dbc")
        self.r, self.YM, self.rho = cat("r"), cat("YM"), cat("rho")
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, np.zeros((0, 4), dtype=np.int32), YM=1e5, PR=0.3, density=1000.0)
        c.set_rod(self.seg, self.r, self.YM, self.rho, bend_scale=1.0)
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
    return Carrier(gpu_lib, rmp.load())


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    perSeg, perBend = c.rod_energy_per_elem()
    bend = c.rod_get()["bend"]
    segOwner = np.searchsorted(off, carrier.seg[:, 0], side="right") - 1
    bendOwner = np.searchsorted(off, bend[:, 1], side="right") - 1
    for coef in COEFS:
        Eall = c.rod_energy(coef)
        Esum = sum(rmp.expected(cs, "E", coef)[0] for cs in cases)
        assert abs(Eall - Esum) <= sum(rmp.expected(cs, "E", coef)[1] for cs in cases)
        cc.compare(rmp, cases, "E", lambda i: coef * (perSeg[segOwner == i].sum() + perBend[bendOwner == i].sum()), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.rod_gradient_add(coef, proj)
            c.set_zero()
            c.rod_hessian_add(coef, proj)
            A = carrier.dense_upper()
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(rmp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(rmp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i in range(len(cases)):  # nothing between the components
                A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]] = 0.0
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {rmp.M:g})")
    assert not bad, "\n".join(bad)


def test_newton_assembly_adds_the_rod_terms_to_mass_and_inertia(carrier):
    """ipcgpu_assemble_newton / ipcgpu_gradient / ipcgpu_incremental_potential on the same state: mass (or identity) on the diagonal plus the rod blocks"""
    c, cases, off = carrier.c, carrier.cases, carrier.off
    coef = COEFS[1]
    mass = c.rod_get()["mass"]
    for proj in (True, False):
        g = c.assemble_newton(coef, proj, with_gradient=True)
        A = carrier.dense_upper()
        dropped = (carrier.dbc == 1) | ((carrier.dbc == 2) & proj)
        D = np.repeat(np.where(dropped, 1.0, mass), 3)
        g2 = c.gradient(coef, proj)
        worst, bad = {}, []
        cc.compare(rmp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "assemble_newton")
        cc.compare(rmp, cases, "g", lambda i: g2[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "gradient")
        # the diagonal holds fl(m + H_ii): that one rounding, u (m + |H_ii|), is not part of the Hessian's tolerance and is taken off before measuring
        H = A - np.diag(D)
        slack = np.diag(2 * rmp.U * np.maximum(D, np.abs(np.diag(H))))
        def block(i):
            s = slice(3 * off[i], 3 * off[i + 1])
            ref = np.triu(rmp.expected(cases[i], "H", coef, proj)[0])
            err = H[s, s] - ref
            return ref + np.sign(err) * np.maximum(np.abs(err) - slack[s, s], 0.0)
        cc.compare(rmp, cases, "H", block, coef, proj, worst, bad, "assemble_newton")
        assert not bad, "\n".join(bad)
    E = c.incremental_potential(coef)
    want = sum(rmp.expected(cs, "E", coef)[0] for cs in cases)
    assert abs(E - want) <= sum(rmp.expected(cs, "E", coef)[1] for cs in cases)  # (xTilde = x: no inertia term)


def test_rod_get_matches_the_reference_constants(carrier):
    info = carrier.c.rod_get()
    assert info["nSeg"] == len(carrier.seg)
    want_b, want_kb, want_rest, want_L, want_ks = [], [], [], [], []
    mass = np.zeros(len(carrier.X))
    for cs, o in zip(carrier.cases, carrier.off):
        X = cs["X"].tolist()
        for s, (a, b) in enumerate(cs["seg"]):
            L = rmp.rest_length(rmp.NP, X[a], X[b])
            want_L.append(L)
            want_ks.append(cs["YM"][s] * np.pi * cs["r"][s] ** 2 / L)
            mass[[a + o, b + o]] += cs["rho"][s] * np.pi * cs["r"][s] ** 2 * L / 2
        for (a, b, c3, s0, s1) in rmp.triples_of(cs["seg"], len(X)):
            want_b.append([a + o, b + o, c3 + o])
            want_kb.append(rmp.bend_stiffness(rmp.NP, [X[a], X[b], X[c3]], ((cs["r"][s0], cs["YM"][s0]), (cs["r"][s1], cs["YM"][s1]))))
            want_rest.append(np.sqrt(rmp.curvature(rmp.NP, [X[a], X[b], X[c3]])[0]))
    assert info["nBend"] == len(want_b) and np.array_equal(info["bend"], np.array(want_b))
    assert np.allclose(info["restLen"], want_L, rtol=1e-14, atol=0) and np.allclose(info["ks"], want_ks, rtol=1e-13, atol=0)
    assert np.allclose(info["kb"], want_kb, rtol=1e-13, atol=0)
    assert np.allclose(info["restKb"], want_rest, rtol=1e-13, atol=1e-7)  # (a straight rest node: sqrt of a rounding)
    assert np.allclose(info["mass"], mass, rtol=1e-13, atol=0)
    assert np.allclose(carrier.c.features()["mass"], mass, rtol=1e-13, atol=0)


def test_pattern_holds_every_block_of_the_reference_matrix(carrier):
    P = carrier.pattern_mask()
    for cs, o, e in zip(carrier.cases, carrier.off[:-1], carrier.off[1:]):
        nz = np.triu(np.abs(cs["H"]) > 0.0)
        assert np.all(P[3 * o:3 * e, 3 * o:3 * e][nz]), cs["name"]


def test_exact_fold_is_plus_infinity_through_the_energy_call(gpu_lib):
    """x_c = x_a on dyadic coordinates (every product exact): d = |e0||e1| + e0 . e1 = 0, the node's energy +infinity, not NaN.  Only the energy is asked
    for: no derivative exists there."""
    X = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0]])
    x = np.array([[0.25, 0.5, 0.0], [0.5, 0.5, 0.125], [0.25, 0.5, 0.0]])
    c = gpu_lib.Context(0)
    c.set_mesh(X, np.zeros((0, 4), dtype=np.int32))
    c.set_rod([[0, 1], [1, 2]], 0.002, 1e7, 1000.0)
    c.opt_init(0.01, False)
    assert np.isfinite(c.rod_energy()) and c.rod_energy() <= 1e-12  # at rest
    c.set_positions(x)
    for coef in COEFS:
        E = c.rod_energy(coef)
        assert E == np.inf and not np.isnan(E)
    perSeg, perBend = c.rod_energy_per_elem()
    assert np.all(np.isfinite(perSeg)) and perBend.tolist() == [np.inf]
