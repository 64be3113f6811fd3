"""Properties of the plastic-flow reference itself (tests/plastic_mp.py), at 100 digits, and the float64 restatement against its tolerance: what shows the
tolerance of test_gpu_plastic_mp.py is attainable without a GPU.  No GPU, no library."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import plastic_mp as pm

EPS = mpf("1e-60")


@pytest.fixture(autouse=True)
def _precision():
    with mp.workdps(pm.DPS):  # (the mp helper modules of this folder leave 50 or 100 digits behind, whichever was imported last)
        yield
CASES = pm.cases()
PAR = lambda c: (c["yield"], c["creep"], c["harden"], c["alpha"], c["dt"])


@pytest.fixture(scope="module")
def refs():
    with mp.workdps(pm.DPS):
        return [pm.reference(c, seed=i) for i, c in enumerate(CASES)]


def test_case_list_covers_every_branch(refs):
    import snh_mp as smp
    assert (pm.M, pm.U) == (smp.M, smp.U)  # the tolerance is built as snh_mp.tol, with its M and u
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert sum(r["yielded"] for r in refs) >= 16 and sum(r["skipped"] for r in refs) == 4
    assert sum((not r["yielded"]) and (not r["skipped"]) and r["decided"] for r in refs) >= 8
    by = dict(zip(names, refs))
    assert not by["one ulp below the yield surface"]["yielded"] and by["one ulp above the yield surface"]["yielded"]
    assert not by["one ulp below the yield surface"]["decided"] and not by["one ulp above the yield surface"]["decided"]
    assert by["pure dilation"]["n"] < 1e-90 and by["pure dilation, yield 0"]["n"] < 1e-90 and not by["pure dilation, yield 0"]["yielded"]  # n = 0 is rejected at y = 0
    assert np.isnan(by["switched off"]["n"]) and not by["switched off"]["skipped"]


def test_flow_is_isochoric_and_identity_below_yield(refs):
    for c, r in zip(CASES, refs):
        G = pm.flow_G(c["X"], c["A"], *PAR(c))
        assert abs(emp._det(G) - 1) < EPS, c["name"]
        assert all(abs(G[i][j] - G[j][i]) < EPS for i in range(3) for j in range(3))
        if not r["yielded"]:
            assert all(abs(G[i][j] - (1 if i == j else 0)) < EPS for i in range(3) for j in range(3)), c["name"]  # (A^-1 A in mp: the identity to 1e-100)
            assert r["alpha1"] == c["alpha"] and np.array_equal(r["A1"], c["A"])
        else:
            assert r["alpha1_mp"] > c["alpha"]
            assert abs(emp._det(r["A1_mp"]) / emp._det(pm._m(c["A"])) - 1) < EPS  # the rest volume does not change


def test_rate_independent_return_lands_on_the_yield_surface_and_stays(refs):
    for c, r in zip(CASES, refs):
        if not r["yielded"] or c["creep"] != pm.INF or c["harden"] != 0.0:
            continue
        n1 = pm.strain_norm(c["X"], r["A1_mp"])
        assert abs(n1 - mpf(c["yield"])) < EPS, c["name"]
        # a second flow: n = y up to 1e-100, so whichever way the comparison falls nothing moves beyond that
        A2, al2, _, _ = pm.flow(c["X"], r["A1_mp"], c["yield"], c["creep"], c["harden"], r["alpha1_mp"], c["dt"])
        assert max(abs(A2[i][j] - r["A1_mp"][i][j]) for i in range(3) for j in range(3)) < EPS and abs(al2 - r["alpha1_mp"]) < EPS


def test_excess_shrinks_by_exp_minus_creep_dt_whatever_the_hardening(refs):
    seen = set()
    for c, r in zip(CASES, refs):
        if not r["yielded"]:
            continue
        for K in (c["harden"], 0.0, 0.7, 3.0):
            A1, al1, n0, _ = pm.flow(c["X"], c["A"], c["yield"], c["creep"], K, c["alpha"], c["dt"])
            if n0 <= mpf(c["yield"]) + mpf(K) * mpf(c["alpha"]):
                continue
            before = n0 - (mpf(c["yield"]) + mpf(K) * mpf(c["alpha"]))
            after = pm.strain_norm(c["X"], A1) - (mpf(c["yield"]) + mpf(K) * al1)
            factor = mpf(0) if c["creep"] == pm.INF else mp.exp(-mpf(c["creep"]) * mpf(c["dt"]))
            assert abs(after - factor * before) < EPS, (c["name"], K)
            seen.add((c["creep"] == pm.INF, K > 0))
    assert len(seen) == 4


def test_rigid_motion_of_the_current_positions_changes_nothing(refs):
    Q, t = emp._rot(555), np.array([0.3, -1.2, 2.5])
    Qm = [[mpf(float(v)) for v in r] for r in Q]
    # Q is orthogonal to 1e-16 only: orthonormalise it in mp (Gram-Schmidt) so that the statement is exact
    for i in range(3):
        for k in range(i):
            dot = sum(Qm[i][j] * Qm[k][j] for j in range(3))
            Qm[i] = [Qm[i][j] - dot * Qm[k][j] for j in range(3)]
        nrm = mp.sqrt(sum(v * v for v in Qm[i]))
        Qm[i] = [v / nrm for v in Qm[i]]
    for c, r in zip(CASES, refs):
        Xq = [[sum(Qm[i][j] * mpf(float(p[j])) for j in range(3)) + mpf(float(t[i])) for i in range(3)] for p in c["X"]]
        A1, al1, _, yl = pm.flow(Xq, c["A"], *PAR(c))
        if not r["decided"]:
            continue
        assert yl == r["yielded"]
        assert max(abs(A1[i][j] - r["A1_mp"][i][j]) for i in range(3) for j in range(3)) < EPS and abs(al1 - r["alpha1_mp"]) < EPS, c["name"]


def test_numpy_restatement_meets_the_tolerance(refs):
    worst = 0.0
    for c, r in zip(CASES, refs):
        A1, al1, n, yl = pm.flow_np(c["X"], c["A"], *PAR(c))
        assert np.all(np.isfinite(A1)) and np.isfinite(al1), c["name"]
        if r["decided"]:
            assert yl == r["yielded"], c["name"]
            if not yl:
                assert np.array_equal(A1, c["A"]) and al1 == c["alpha"]
        worst = max(worst, float((np.abs(A1 - r["A1"]) / r["tolA"]).max()) * pm.M)
        if r["tolAlpha"] > 0:  # (zero for a skipped or switched-off element that starts at alpha = 0: alpha must then stay exactly 0)
            worst = max(worst, abs(al1 - r["alpha1"]) / r["tolAlpha"] * pm.M)
        assert np.all(np.abs(A1 - r["A1"]) <= r["tolA"]), (c["name"], np.abs(A1 - r["A1"]) / r["tolA"])
        assert abs(al1 - r["alpha1"]) <= r["tolAlpha"], c["name"]
    print(f"worst err / (sens + u scale) of the NumPy restatement: {worst:.3g} (M = {pm.M:g})")
