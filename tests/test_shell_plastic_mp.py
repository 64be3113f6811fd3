"""The mpmath reference of the shells' plastic flow (tests/shell_plastic_mp.py) obeys the properties shell_plastic_kernels.h states, and its tolerances are
attainable: a float64 NumPy restatement by another route stays inside them.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import plastic_mp as pmp
import shell_plastic_mp as spm

INF = float("inf")
TINY = mpf(10) ** -80  # mp identities hold to the working precision (100 digits)


def test_constants_are_the_tetrahedral_reference_s():
    assert (spm.DPS, spm.U, spm.M) == (pmp.DPS, pmp.U, pmp.M) == (100, 2.0 ** -53, 128.0)


def _flowed(case, harden=None, creep=None, dt=None):
    K = case["harden"] if harden is None else harden
    cr = case["creep"] if creep is None else creep
    dt = case["dt"] if dt is None else dt
    return spm.flow_tri(case["X"], case["B"], *case["k"], case["yield"], cr, K, case["alpha"], dt), K, cr, dt


@pytest.mark.parametrize("harden", [0.0, 2.0])
@pytest.mark.parametrize("creep,dt", [(INF, 0.01), (5.0, 0.01), (5.0, 0.1)])
def test_the_new_norm_is_n_minus_delta_and_the_excess_shrinks_by_exp_minus_creep_dt(harden, creep, dt):
    with mp.workdps(spm.DPS):
        for case in [c for c in spm.tri_cases() if c["yield"] < INF][:12]:
            (B1, al1, n, yielded, f), K, cr, _ = _flowed(case, harden, creep, dt)
            if not yielded:
                continue
            Delta = al1 - mpf(case["alpha"])
            n1 = spm.tri_strain(case["X"], B1, *case["k"])[3]
            assert abs(n1 - (n - Delta)) < TINY, case["name"]
            y0, y1 = mpf(case["yield"]) + mpf(K) * mpf(case["alpha"]), mpf(case["yield"]) + mpf(K) * al1
            shrink = mpf(0) if cr == INF else mp.exp(-mpf(cr) * mpf(dt))
            assert abs((n1 - y1) - shrink * (n - y0)) < TINY, case["name"]


def test_det_G_times_the_thickness_change_conserves_h_A():
    """the plastic thickness stretch is exp(-f e3) with e3 = -c (e1 + e2) flowing like the in-plane strains would NOT conserve volume unless nu = 1/2; the model
    instead lets the thickness take up det G: h'A' = (h / det G) (A det G) -- the rest area grows by det G = det B / det B', which tri_reference calls ratio"""
    with mp.workdps(spm.DPS):
        for case in spm.tri_cases():
            B1, _, n, yielded, f = spm.flow_tri(case["X"], case["B"], *case["k"], case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
            B = spm._m(case["B"])
            det = lambda Z: Z[0][0] * Z[1][1] - Z[0][1] * Z[1][0]
            detG = det(B1) / det(B)
            if not yielded:
                assert detG == 1
                continue
            e = spm.tri_strain(case["X"], B, *case["k"])[0]
            assert abs(detG - mp.exp(-f * (e[0] + e[1]))) < TINY, case["name"]  # det G = exp(-f tr e)
            h, A = mpf(case["thickness"]), 1 / (2 * abs(det(B)))  # rest area = |det Dm| / 2
            A1 = 1 / (2 * abs(det(B1)))
            assert abs((h * detG) * A1 - h * A) < TINY  # the thickness that keeps h A: h det G


def test_G_is_continuous_across_equal_stretches():
    with mp.workdps(spm.DPS):
        base = spm.tri_case("equal", (1.2, 1.2))
        G0 = _G(base)
        for eps in (1e-6, 1e-9, 1e-12):
            for F2 in ((1.2 + eps, 1.2), (1.2, 1.2 + eps), [[1.2, eps], [0.0, 1.2]]):
                G1 = _G(spm.tri_case("near", F2))
                assert max(abs(G1[i][j] - G0[i][j]) for i in range(2) for j in range(2)) < 10 * eps
        # a multiple of the identity -- to the rounding of the case's doubles (X and B are rounded, so the two stretches differ by a few U)
        assert abs(G0[0][1]) < 64 * spm.U and abs(G0[0][0] - G0[1][1]) < 64 * spm.U


def _G(case):
    B1 = spm.flow_tri(case["X"], case["B"], *case["k"], case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])[0]
    B = spm._m(case["B"])
    d = B[0][0] * B[1][1] - B[0][1] * B[1][0]
    Bi = [[B[1][1] / d, -B[0][1] / d], [-B[1][0] / d, B[0][0] / d]]
    return [[sum(Bi[i][k] * B1[k][j] for k in range(2)) for j in range(2)] for i in range(2)]


def test_closed_form_of_the_norm_in_p_and_q():
    with mp.workdps(spm.DPS):
        for case in spm.tri_cases():
            st = spm.tri_strain(case["X"], case["B"], *case["k"])
            if st is None:
                continue
            e, _, _, n = st
            c = mpf(case["k"][1]) / (2 * mpf(case["k"][0]))
            p, q = (e[0] + e[1]) / mp.sqrt(2), (e[0] - e[1]) / mp.sqrt(2)
            assert abs(n * n - ((1 + 2 * c) ** 2 / 3 * p * p + q * q)) < TINY, case["name"]


def test_the_new_rest_angle_lies_between_the_old_one_and_theta():
    with mp.workdps(spm.DPS):
        seen = 0
        for case in spm.hinge_cases():
            t1, a1, eps, yielded, theta = spm.flow_hinge(case["X"], case["thetaBar"], case["g"], case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
            tb = mpf(case["thetaBar"])
            if not yielded:
                assert t1 == tb and a1 == mpf(case["alpha"])
                continue
            seen += 1
            assert min(tb, theta) <= t1 <= max(tb, theta), case["name"]
            assert -mp.pi < t1 <= mp.pi
            # the excess shrinks by exp(-creep dt), as for the membrane
            K = mpf(case["harden"])
            y0, y1 = mpf(case["yield"]) + K * mpf(case["alpha"]), mpf(case["yield"]) + K * a1
            shrink = mpf(0) if case["creep"] == INF else mp.exp(-mpf(case["creep"]) * mpf(case["dt"]))
            assert abs((mpf(case["g"]) * abs(theta - t1) - y1) - shrink * (eps - y0)) < TINY, case["name"]
        assert seen >= 8


def _ratio(err, tol):
    """err / tol entry by entry, 0 where both are 0 (a value that is handed through has tolerance 0 and must come back exactly)"""
    err, tol = np.atleast_1d(np.abs(err)).astype(float).ravel(), np.atleast_1d(tol).astype(float).ravel()
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, np.finfo(float).tiny))))


def test_float64_restatements_stay_inside_the_tolerances():
    worst = 0.0
    for i, case in enumerate(spm.tri_cases()):
        ref = spm.tri_reference(case, seed=i)
        B1, al1, n, yielded = spm.flow_tri_np(case["X"], case["B"], *case["k"], case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
        if ref["decided"]:
            assert yielded == ref["yielded"], case["name"]
        r = max(_ratio(B1 - ref["B1"], ref["tolB"]), _ratio(al1 - ref["alpha1"], ref["tolAlpha"]))
        worst = max(worst, r)
        assert r <= 1.0, (case["name"], r)
    for i, case in enumerate(spm.hinge_cases()):
        ref = spm.hinge_reference(case, seed=i)
        t1, a1, eps, yielded = spm.flow_hinge_np(case["X"], case["thetaBar"], case["g"], case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
        if ref["decided"]:
            assert yielded == ref["yielded"], case["name"]
        r = max(_ratio(t1 - ref["thetaBar1"], ref["tolTheta"]), _ratio(a1 - ref["alphaB1"], ref["tolAlpha"]))
        worst = max(worst, r)
        assert r <= 1.0, (case["name"], r)
    print(f"worst float64 restatement error / tolerance: {worst:.3f}")


def test_the_cases_cover_what_they_claim():
    refs = [spm.tri_reference(c, seed=i) for i, c in enumerate(spm.tri_cases())]
    assert sum(r["yielded"] for r in refs) >= 20 and sum(r["skipped"] for r in refs) == 2
    assert sum(1 for r in refs if not r["decided"]) >= 2
    h = [spm.hinge_reference(c, seed=i) for i, c in enumerate(spm.hinge_cases())]
    assert sum(r["yielded"] for r in h) >= 8 and sum(r["skipped"] for r in h) == 1
    ks = [c for c, r in zip(spm.hinge_cases(), h) if r["yielded"] and "changes sign" in c["name"]]
    assert ks and all(np.sign(r["theta"] - c["thetaBar"]) != np.sign(c["thetaBar"]) for c, r in zip(spm.hinge_cases(), h) if "changes sign" in c["name"])
