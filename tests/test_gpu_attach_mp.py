"""The attachment kernels through the C ABI against the mpmath cases of attach_mp.py (tests/golden/attach_mp_cases.npz).  Every case is a node range of its
own in ONE carrier mesh without tetrahedra (ranges side by side), so each case's energy terms, gradient rows and dense block are its own.  Two cases have
a one-triangle shell on the triangle they tie to and two a one-segment rod on their edge, so the pattern comes from three sources (shell, rod and
attachment pairs).  The tolerance is attach_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_attach_mp.py."""
import numpy as np
import pytest

import attach_mp as amp
import codim_common as cc

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)
# (case, its local nodes): single elements that share no edge and no node, so every matrix entry receives one addend per shell / rod kernel
SHELL_ON = {"node - triangle point": (0, 1, 2), "triangle point - triangle point": (0, 1, 2)}
ROD_ON = {"node - edge point": (1, 2), "edge point - triangle point": (0, 1)}


class Carrier:
    def __init__(self, gpu_lib, cases):
        self.cases = cases
        self.off = off = np.concatenate([[0], np.cumsum([len(c["x"]) for c in cases])]).astype(int)
        # (a rigid shift would change the stored inputs: the cases stay where they are, overlapping in space -- there is no contact here).  The rest
        # positions are the current ones: the shell triangles and the rod segments are at rest
        self.x = np.vstack([c["x"] for c in cases])
        cat = lambda k: np.concatenate([c[k] for c in cases])
        shift = lambda k: np.concatenate([np.where(c[k] >= 0, c[k] + o, -1) for c, o in zip(cases, off)]).astype(np.int32)
        self.dbc = cat("dbc")
        self.nA, self.nB, self.wA, self.wB, self.k, self.L = shift("nA"), shift("nB"), cat("wA"), cat("wB"), cat("k"), cat("L")
        self.owner = np.searchsorted(off, self.nA[:, 0], side="right") - 1
        by = {c["name"]: o for c, o in zip(cases, off)}
        self.tri = np.array([[by[n] + v for v in loc] for n, loc in SHELL_ON.items()], dtype=np.int32)
        self.seg = np.array([[by[n] + v for v in loc] for n, loc in ROD_ON.items()], dtype=np.int32)
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.x, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, 1e-3, 1e5, 0.3, 1000.0)
        c.set_rod(self.seg, 0.002, 1e7, 1000.0)
        c.set_attachments(self.nA, self.nB, self.k, self.L, self.wA, self.wB)
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
    return Carrier(gpu_lib, amp.load())


def test_energy_gradient_hessian_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    per = c.attach_energy_per_elem()
    assert np.all(np.isfinite(per))
    for cs, i in zip(cases, range(len(cases))):  # the per-attachment terms one by one: each within its case's energy tolerance
        assert np.all(np.abs(per[carrier.owner == i] - cs["perE"]) <= amp.expected(cs, "E")[1]), cs["name"]
    for coef in COEFS:
        Eall = c.attach_energy(coef)
        Esum = sum(amp.expected(cs, "E", coef)[0] for cs in cases)
        assert abs(Eall - Esum) <= sum(amp.expected(cs, "E", coef)[1] for cs in cases)
        cc.compare(amp, cases, "E", lambda i: coef * per[carrier.owner == i].sum(), coef, True, worst, bad, f"coef {coef:g}")
        for proj in (True, False):
            g = c.attach_gradient_add(coef, proj)
            c.set_zero()
            c.attach_hessian_add(coef, proj)
            A = carrier.dense_upper()
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(amp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(amp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert dropped.any() and np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i, cs in enumerate(cases):
                s = slice(3 * off[i], 3 * off[i + 1])
                if cs["name"] == "coincident points with a rest length":  # no direction: nothing is written at all
                    assert np.all(g[s] == 0.0) and np.all(A[s, s] == 0.0)
                A[s, s] = 0.0  # ... and nothing between the cases
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {amp.M:g})")
    assert not bad, "\n".join(bad)


def test_newton_assembly_adds_the_attachments_to_mass_inertia_shell_and_rod(carrier):
    """ipcgpu_assemble_newton / ipcgpu_gradient / ipcgpu_incremental_potential on the same state.  The shell triangles and rod segments are at rest and single
    (one addend per entry and kernel: no summation order), so what they add is taken off with their own entry points: a matrix entry holds
    fl(fl(m + s) + h) -- mass or identity m, shell / rod s, attachment h -- and those two roundings, at most u (|m + s| + |m + s + h|), are no part of the
    attachment Hessian's tolerance and are taken off before measuring (as test_gpu_rod_mp.py does for the diagonal)."""
    c, cases, off = carrier.c, carrier.cases, carrier.off
    coef = COEFS[1]
    mass = c.features()["mass"]
    for proj in (True, False):
        g = c.assemble_newton(coef, proj, with_gradient=True)
        A = carrier.dense_upper()
        g2 = c.gradient(coef, proj)
        gOther = c.rod_gradient_add(coef, proj, c.shell_gradient_add(coef, proj))
        c.set_zero()
        c.shell_hessian_add(coef, proj)
        c.rod_hessian_add(coef, proj)
        Sm = carrier.dense_upper()
        dropped = (carrier.dbc == 1) | ((carrier.dbc == 2) & proj)
        Sm += np.diag(np.repeat(np.where(dropped, 1.0, mass), 3))
        H = A - Sm
        slack = amp.U * (np.abs(Sm) + np.abs(A))
        worst, bad = {}, []
        cc.compare(amp, cases, "g", lambda i: (g - gOther)[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "assemble_newton")
        cc.compare(amp, cases, "g", lambda i: (g2 - gOther)[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, "gradient")
        def block(i):
            s = slice(3 * off[i], 3 * off[i + 1])
            ref = np.triu(amp.expected(cases[i], "H", coef, proj)[0])
            err = H[s, s] - ref
            return ref + np.sign(err) * np.maximum(np.abs(err) - slack[s, s], 0.0)
        cc.compare(amp, cases, "H", block, coef, proj, worst, bad, "assemble_newton")
        assert not bad, "\n".join(bad)
    E = c.incremental_potential(coef)
    want = sum(amp.expected(cs, "E", coef)[0] for cs in cases) + c.shell_energy(coef) + c.rod_energy(coef)
    assert abs(E - want) <= sum(amp.expected(cs, "E", coef)[1] for cs in cases)  # (xTilde = x: no inertia term)


def test_state_and_get_against_mpmath_and_the_python_merge(carrier):
    """length l = |d| and force k (l - L).  Tolerance from the arithmetic: d_a = sum of m <= 6 products, each rounded once and summed with m - 1 roundings:
    |delta d_a| <= (m + 1) u sum |c_i| |x_i,a| <= 8 u dm_a; l is 1-Lipschitz in d, and the dot product and the square root add 3 u l at most:
    |delta l| <= 8 u |dm| + 4 u l.  The force adds the rounding of the difference and of the product: k |delta l| + 2 u k (l + L)."""
    c, cases = carrier.c, carrier.cases
    l, f = c.attach_state()
    info = c.attach_get()
    assert info["n"] == len(carrier.k) and np.array_equal(info["k"], carrier.k) and np.array_equal(info["L"], carrier.L)
    worst = 0.0
    for i, cs in enumerate(cases):
        mine = np.flatnonzero(carrier.owner == i)
        for j, (ids, coef) in zip(mine, amp.stencils(cs)):
            m = len(ids)
            assert info["count"][j] == m and info["nodes"][j, :m].tolist() == [v + carrier.off[i] for v in ids] and info["coefs"][j, :m].tolist() == coef
            assert np.all(info["nodes"][j, m:] == info["nodes"][j, 0]) and np.all(info["coefs"][j, m:] == 0.0)
            dm = np.linalg.norm((np.abs(coef)[:, None] * np.abs(cs["x"][ids])).sum(axis=0))
            k, L = carrier.k[j], carrier.L[j]
            lref, fref = cs["len"][j - mine[0]], cs["force"][j - mine[0]]
            tl = amp.U * (8 * dm + 4 * lref)
            tf = k * tl + 2 * amp.U * k * (lref + L)
            worst = max(worst, abs(l[j] - lref) / tl, abs(f[j] - fref) / tf)
            assert abs(l[j] - lref) <= tl and abs(f[j] - fref) <= tf, cs["name"]
            assert abs(info["restDist"][j] - lref) <= tl  # (the rest positions of the carrier are the current ones)
    print(f"worst error of length and force over its bound: {worst:.3g}")


def test_pattern_holds_every_block_of_the_reference_matrix(carrier):
    ia, ja = carrier.c.get_pattern()
    P = np.zeros((len(ia) - 1, len(ia) - 1), dtype=bool)
    P[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = True
    for cs, o, e in zip(carrier.cases, carrier.off[:-1], carrier.off[1:]):
        full = np.array(amp.reference(amp.NP, cs, project=False)[2], dtype=np.float64)
        assert np.all(P[3 * o:3 * e, 3 * o:3 * e][np.triu(np.abs(full) > 0.0)]), cs["name"]
