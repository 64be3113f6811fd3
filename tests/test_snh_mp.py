"""The mpmath restatement of the stable neo-Hookean energy (snh_mp.py) pinned on differentiation of psi and on itself, the stored file against a fresh evaluation,
the branches the cases must enter, and the margin M against the float64 NumPy restatement.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import snh_mp as smp

EPS = mpf("1e-60")  # closed form against closed form, relative to the size of the quantity
EPS_DIFF = mpf("1e-40")  # against mp.diff (numerical differentiation at 100 digits)


@pytest.fixture(scope="module")
def elems():
    return smp.load(prefix="e_")


@pytest.fixture(scope="module")
def blocks():
    return smp.load(prefix="b_")


def _F(case):
    return smp.deformation(case["Xr"], case["X"])[0]


def _lame(case):
    return emp.lame(case["YM"], case["PR"])


def _stiff(elems):
    return [c for c in elems if c["YM"] > 0]


def _dpsi(F, muL, lamL, idx):
    """mixed derivative of psi in the entries idx = ((i, j), ...) of F"""
    def f(*x):
        G = [list(r) for r in F]
        for (i, j), v in zip(idx, x):
            G[i][j] = G[i][j] + v
        return smp.psi(G, muL, lamL)
    return mp.diff(f, tuple(mpf(0) for _ in idx), tuple(1 for _ in idx))


def test_the_file_is_what_the_module_places(elems, blocks):
    for stored, fresh in ((elems, smp.element_cases()), (blocks, smp.block_cases())):
        assert [c["name"] for c in stored] == [c["name"] for c in fresh]
        for a, b in zip(stored, fresh):
            for k in smp.E_IN:
                assert np.array_equal(a[k], b[k]), (a["name"], k)
    Z = np.load(emp.GOLDEN)
    assert np.array_equal(np.array([c["X"] for c in blocks]), Z["m_X"][Z["m_F"]]) and np.array_equal(np.array([c["Xr"] for c in blocks]), Z["m_V"][Z["m_F"]])


def test_stored_references_against_a_fresh_evaluation(elems):
    for c in elems[::5]:
        r, sens = smp.evaluate_element(c, 9000 + 2 * c["index"])
        for k in smp.E_REF:
            got, want = (emp._triu(r[k]), emp._triu(c["ref_" + k])) if k == "H" else (r[k], c["ref_" + k])  # (the file keeps the upper triangle)
            assert np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True), (c["name"], k)
        for k in smp.QUANT:
            assert np.array_equal(emp._triu(sens[k]) if k == "H" else sens[k], emp._triu(c["sens_" + k]) if k == "H" else c["sens_" + k], equal_nan=True), (c["name"], k)


def test_rest_is_a_stress_free_zero_of_the_energy():
    I = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    for PR, YM in ((0.4, 1e5), (0.499, 1e9), (0.0, 1e3)):
        muL, lamL = emp.lame(YM, PR)
        assert abs(smp.psi(I, muL, lamL)) <= EPS * muL
        assert max(abs(v) for r in smp.piola(I, muL, lamL) for v in r) <= EPS * muL


def test_the_reparametrisation_gives_hooke_at_rest():
    """d2psi/dF2 at F = I is lam_L dd + mu_L (dd + dd) of the UNMAPPED Lame parameters"""
    I = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    d = lambda a, b: int(a == b)
    for PR, YM in ((0.4, 1e5), (0.499, 1e9), (0.0, 1e3)):
        muL, lamL = emp.lame(YM, PR)
        H = smp.d2psi(I, muL, lamL)
        for i in range(3):
            for j in range(3):
                for r in range(3):
                    for l in range(3):
                        hooke = lamL * d(i, j) * d(r, l) + muL * (d(i, r) * d(j, l) + d(i, l) * d(j, r))
                        assert abs(H[3 * i + j, 3 * r + l] - hooke) <= EPS * (muL + lamL), (PR, i, j, r, l)


def test_piola_is_the_derivative_of_psi(elems):
    for c in _stiff(elems)[::3]:
        F, (muL, lamL) = _F(c), _lame(c)
        P = smp.piola(F, muL, lamL)
        top = max(abs(v) for r in P for v in r) + muL
        for i in range(3):
            for j in range(3):
                assert abs(P[i][j] - _dpsi(F, muL, lamL, ((i, j),))) <= EPS_DIFF * top, (c["name"], i, j)


def test_the_9x9_is_the_second_derivative_of_psi(elems):
    rng = np.random.default_rng(3)
    for c in _stiff(elems)[::4]:
        F, (muL, lamL) = _F(c), _lame(c)
        H = smp.d2psi(F, muL, lamL)
        top = max(abs(H[i, j]) for i in range(9) for j in range(9)) + muL
        for _ in range(6):
            p, q = (int(v) for v in rng.integers(0, 9, 2))
            idx = ((p // 3, p % 3), (q // 3, q % 3))
            if p == q:
                G = lambda x: smp.psi([[F[i][j] + (x if (i, j) == idx[0] else 0) for j in range(3)] for i in range(3)], muL, lamL)
                ref = mp.diff(G, mpf(0), 2)
            else:
                ref = _dpsi(F, muL, lamL, idx)
            assert abs(H[p, q] - ref) <= EPS_DIFF * top, (c["name"], p, q)


def test_sigma_forms_against_differentiation_in_sigma_space(elems):
    for c in _stiff(elems)[::3]:
        muL, lamL = _lame(c)
        s = emp.signed_singular_values(_F(c))
        dE, A, B = smp.sigma_forms(s, muL, lamL)
        top = muL + lamL * (1 + max(abs(v) for v in s)) ** 4

        def psi_at(*x):
            return smp.psi_sigma([s[i] + x[i] for i in range(3)], muL, lamL)
        for i in range(3):
            o = [0, 0, 0]
            o[i] = 1
            assert abs(dE[i] - mp.diff(psi_at, (0, 0, 0), tuple(o))) <= EPS_DIFF * top
            for j in range(3):
                o2 = list(o)
                o2[j] += 1
                assert abs(A[i, j] - mp.diff(psi_at, (0, 0, 0), tuple(o2))) <= EPS_DIFF * top
        for n, (i, j, m) in enumerate(smp.PAIRS):  # the two divided differences of the scheme reduce exactly
            if abs(s[i] - s[j]) > mpf("1e-3"):
                assert abs(B[n][0] - (dE[i] - dE[j]) / (s[i] - s[j])) <= EPS * top
            if abs(s[i] + s[j]) > mpf("1e-3"):
                assert abs(B[n][1] - (dE[i] + dE[j]) / (s[i] + s[j])) <= EPS * top


def test_sigma_forms_against_the_unprojected_9x9(elems):
    """T^T (d2psi/dF2) T has A on (00, 11, 22), [[mu c, -k s_m], [-k s_m, mu c]] on every pair, and nothing else"""
    for c in _stiff(elems):
        if c["name"] in ("SNH all four nodes at one point, F = 0",):
            continue  # F = 0: the 9 x 9 is zero in every basis (checked below)
        F, (muL, lamL) = _F(c), _lame(c)
        T, s = smp.sigma_basis(F)
        H = smp.d2psi(F, muL, lamL)
        Ms = T.T * H * T
        want = smp.sigma_matrix(s, muL, lamL, False)
        top = max(abs(H[i, j]) for i in range(9) for j in range(9))
        assert max(abs(Ms[i, j] - want[i, j]) for i in range(9) for j in range(9)) <= mpf("1e-80") * top, c["name"]
    point = [c for c in elems if c["name"].endswith("F = 0")][0]
    H = smp.d2psi(_F(point), *_lame(point))
    assert max(abs(H[i, j]) for i in range(9) for j in range(9)) == 0


def test_projection(elems, blocks):
    """the projected matrix is PSD; it equals the unprojected one wherever that is PSD; built the kernel's way (SVD, sigma-space blocks) it is the same matrix"""
    n_psd = 0
    for c in _stiff(elems) + blocks[::8]:
        F, (muL, lamL) = _F(c), _lame(c)
        H = smp.d2psi(F, muL, lamL)
        P9, ev = smp.eig_clamp(H, 9)
        top = max(abs(H[i, j]) for i in range(9) for j in range(9)) + muL * mpf("1e-30")
        assert min(mp.eigsy(P9, eigvals_only=True)) >= -mpf("1e-80") * top
        assert bool(c["ref_psd"]) == (min(ev) >= 0)
        if min(ev) >= 0:
            n_psd += 1
            assert max(abs(P9[i, j] - H[i, j]) for i in range(9) for j in range(9)) <= mpf("1e-80") * top, c["name"]
            assert c["ref_negA"] == 0 and not c["ref_clamped"].any()
        else:
            assert c["ref_negA"] > 0 or c["ref_clamped"].any(), c["name"]
        Ps = smp.project_sigma(F, muL, lamL)
        assert max(abs(P9[i, j] - Ps[i, j]) for i in range(9) for j in range(9)) <= mpf("1e-70") * top, c["name"]
    assert n_psd >= 3


def test_every_branch_is_entered(elems):
    by = {c["name"][4:]: c for c in elems}
    s = lambda n: by[n]["ref_s"]
    assert by["A indefinite (Jacobi path of make_pd3)"]["ref_negA"] >= 1 and by["A indefinite, PR 0.499"]["ref_negA"] >= 1
    assert by["A definite (fast exit of make_pd3)"]["ref_negA"] == 0
    assert by["a 2 x 2 block clamped"]["ref_clamped"].any() and by["all three 2 x 2 blocks clamped"]["ref_clamped"].all()
    assert not by["no 2 x 2 block clamped"]["ref_clamped"].any()
    assert by["nothing projected"]["ref_psd"] and by["rest"]["ref_negA"] == 0
    assert s("s_2 < 0, one flipped axis")[2] < 0 and s("s_2 < 0, one flipped axis")[1] > 0
    assert np.allclose(s("reflection of rest"), (1, 1, -1), atol=0, rtol=0)
    assert s("flat, J = 0")[2] == 0 and abs(s("flat, J = 0, rotated")[2]) < 1e-15
    assert np.all(s("all four nodes at one point, F = 0") == 0) and np.isfinite(by["all four nodes at one point, F = 0"]["ref_E"])
    assert abs(s("two equal singular values")[0] - s("two equal singular values")[1]) < 1e-14
    assert np.ptp(np.abs(s("three equal singular values 0.5"))) < 1e-15
    assert abs(s("compression to 1e-3")[2] - 1e-3) < 1e-15 and abs(s("stretch to 1e2")[0] - 1e2) < 1e-12
    assert by["zero stiffness"]["ref_E"] == 0.0 and not by["zero stiffness"]["ref_H"].any()
    assert {tuple(int(v) for v in c["dtype"]) for c in elems} >= {(1, 0, 2, 0), (1, 0, 0, 0), (0, 0, 2, 2)} or sum(c["dtype"].any() for c in elems) >= 5
    assert len({(c["YM"], c["PR"]) for c in elems}) >= 4
    assert {c["size"] for c in elems} >= {1e-2, 1.0, 1e2}
    for c in elems:  # every case a factor 50 from the thresholds it was searched for keeps its branch under the perturbation that measures sens
        assert np.all(np.isfinite(c["ref_E"])) and np.all(np.isfinite(c["ref_g"])) and np.all(np.isfinite(c["ref_H"]))


def test_tolerances_are_tight(elems, blocks):
    """no stored tolerance exceeds 1e-6 of its quantity's scale (1e-4 for the sliver and the flat elements): a check that passes everything cannot come back"""
    for c in _stiff(elems) + blocks:
        loose = "sliver" in c["name"] or "flat" in c["name"] or "1e-3" in c["name"]
        for k in ("E", "g", "H"):
            assert np.max(smp.tol(c, k, projectDBC=False)) <= (1e-4 if loose else 1e-6) * c["ref_" + k + "scale"], (c["name"], k)


def test_numpy_restatement_meets_the_tolerance():
    """M is 8 x the worst ratio of the float64 restatement, rounded up to a power of two"""
    with np.errstate(all="ignore"):
        r = smp.numpy_ratios()
    worst = max(v[0] for v in r.values())
    print({k: (f"{v[0]:.3g}", v[1], f"{v[2]:.3g}") for k, v in r.items()})
    assert abs(worst - smp.NUMPY_WORST_RATIO) <= 0.05 * smp.NUMPY_WORST_RATIO
    assert smp.M == 2.0 ** np.ceil(np.log2(8 * smp.NUMPY_WORST_RATIO))


def test_stress_is_P_FT_over_J(elems):
    for c in _stiff(elems)[::3]:
        if not smp.stress_checked(c):
            continue
        F, (muL, lamL) = _F(c), _lame(c)
        P, J = smp.piola(F, muL, lamL), emp._det(F)
        sg = smp.cauchy(F, muL, lamL)
        full = [[sum(P[i][q] * F[j][q] for q in range(3)) / J for j in range(3)] for i in range(3)]
        top = max(abs(v) for v in sg)
        for n, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))):
            assert abs(sg[n] - full[i][j]) <= EPS * top and abs(full[i][j] - full[j][i]) <= EPS * top, c["name"]
