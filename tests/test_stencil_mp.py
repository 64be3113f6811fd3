"""The mpmath reference of stencil_mp.py on configurations with closed forms, the stored file against a fresh evaluation, and the oracle under the
tolerance the GPU tests use (which pins the margin M of stencil_mp.py)."""
import numpy as np
import pytest
from mpmath import mp, mpf

import stencil_mp as smp


def P(*rows):
    return [[mpf(v) for v in r] for r in rows]


def test_distances_on_closed_forms():
    h = mpf("0.375")
    tri = P((0, 0, 0), (2, 0, 0), (0, 3, 0))
    assert smp.dist2(smp.K_PT, P((0.5, 0.25, 0.375)) + tri) == h * h  # a point at height h over the plane z = 0
    assert smp.dist2(smp.K_PT, P((7, -5, -0.375)) + tri) == h * h  # the PLANE's distance: the foot need not lie in the triangle
    assert smp.dist2(smp.K_EE, P((-1, 0, 0), (1, 0, 0), (0, -1, 0.375), (0, 2, 0.375))) == h * h  # crossing perpendicular edges
    assert smp.dist2(smp.K_PE, P((0.3, 0.375, 0), (-1, 0, 0), (4, 0, 0))) == h * h
    assert smp.dist2(smp.K_PP, P((1, 2, 3), (1, 2, 3.375))) == h * h
    assert smp.cross_norm(P((0, 0, 0), (2, 0, 0), (0, 0, 1), (0, 3, 1))) == 36
    assert smp.mollifier(mpf(1) / 2, mpf(1)) == mpf(3) / 4 and smp.mollifier(mpf(2), mpf(1)) == 1 and smp.mollifier(mpf(1), mpf(1)) == 1


def test_barrier_vanishes_to_second_order_at_dhat():
    dHat = mpf(smp.DHAT)
    for k in (10, 20, 30):
        t = mpf(10) ** -k
        d = dHat * (1 - t)
        b2 = (smp.barrier_d1(d * (1 + t / 1000), dHat) - smp.barrier_d1(d * (1 - t / 1000), dHat)) / (2 * d * t / 1000)
        assert abs(smp.barrier(d, dHat)) <= 2 * t ** 3 * dHat ** 2 and abs(smp.barrier_d1(d, dHat)) <= 4 * t ** 2 * dHat and abs(b2) <= 8 * t
    assert smp.barrier(dHat, dHat) == 0 and smp.barrier_d1(dHat, dHat) == 0
    assert smp.barrier(dHat / 2, dHat) == (dHat / 2) ** 2 * mp.log(2)


def test_central_differences_and_projection_on_a_quadratic():
    A = np.array([[2.0, 1.0, 0.0], [1.0, -1.0, 0.5], [0.0, 0.5, 0.25]])
    y = [mpf(0.3), mpf(-1.25), mpf(2)] + [mpf(0)] * 9
    E = lambda z: sum(A[i, j] * z[i] * z[j] for i in range(3) for j in range(3)) / 2
    E0, g, H = smp._derivs(E, y, [0, 1, 2], mpf("1e-20"))
    assert np.allclose(smp._f(g)[:3], A @ np.array([0.3, -1.25, 2.0]), rtol=1e-15)
    assert np.abs(np.array([smp._f(r) for r in H])[:3, :3] - A).max() < 1e-15
    w, Q = np.linalg.eigh(A)
    got = np.array([smp._f(r) for r in smp.project_psd(H, [0, 1, 2])])[:3, :3]
    assert np.abs(got - (Q * np.maximum(w, 0)) @ Q.T).max() < 1e-14 and np.linalg.eigvalsh(got).min() > -1e-15


def test_friction_potential_is_c1_and_frictionless_at_rest():
    eps = mpf("1e-4")
    assert smp.f0(mpf(0), eps) == eps / 3 and smp.f0(eps, eps) == eps and smp.f0(2 * eps, eps) == 2 * eps
    t = mpf("1e-30")
    assert abs((smp.f0(eps, eps) - smp.f0(eps - t, eps)) / t - 1) < 1e-20  # slope 1 from below, as beyond eps


def test_the_cases_cover_what_they_claim():
    cs = smp.load(prefix="c_")
    bins = np.bincount([smp.bin_of(c) for c in cs], minlength=8)
    assert bins[6] == 0 and all(bins[b] >= 20 for b in (0, 1, 2, 3, 4, 5, 7))  # a mollified pair has no point-triangle distance stencil
    assert {c["mult"] for c in cs if c["kind"] in (smp.K_PP, smp.K_PE) and not c["para"]} == {1, 2, 3}
    assert {float(c["kappa"]) for c in cs} == set(smp.KAPPAS)
    for c in cs:
        assert 0 < c["ref_d"] <= smp.DHAT, c["name"]  # (the exact d is below dHat; rounded to double it may be dHat itself)
    ulp = [c for c in cs if "one ulp below" in c["name"]]
    assert len(ulp) == 4 and all(c["ref_d"] >= np.nextafter(smp.DHAT, 0) for c in ulp)
    assert sum(1 for c in cs if (c["dbc"] >= 0).any()) >= 20
    fr = smp.load(prefix="f_")
    assert sum(1 for c in fr if np.all(c["Xn"] == c["X"])) == 4 and len({float(c["eps2"]) for c in fr}) == 7


def test_stored_references_are_current():
    """a fixed random tenth of the cases evaluated afresh from the inputs IN the file: a stale file (reference or case changed, file not rebuilt) fails"""
    rng = np.random.default_rng(11)
    for pre, fn, keys in (("c_", smp.evaluate_contact, ("d", "gd", "E", "g", "H")), ("f_", smp.evaluate_friction, ("lam", "coord", "basis", "E", "g", "H")),
                          ("h_", smp.evaluate_contact, ("E", "g", "H"))):
        cs = smp.load(prefix=pre)
        for i in rng.choice(len(cs), size=max(len(cs) // (10 if pre != "h_" else 60), 1), replace=False):
            ref, sens = fn(cs[i], smp.reference_seed(int(i)))
            for k in keys:
                assert np.all(np.abs(np.asarray(ref[k]) - cs[i]["ref_" + k]) <= 1e-15 * np.abs(cs[i]["ref_" + k])), (cs[i]["name"], k)
                assert np.all(np.abs(sens[k] - cs[i]["sens_" + k]) <= 1e-15 * np.abs(cs[i]["sens_" + k])), (cs[i]["name"], k)


def test_oracle_meets_the_tolerance(orc):
    """the margin: M = 8 x the oracle's worst err / (sens + u scale), rounded up to a power of two; no case may need more than 128"""
    worst = max(r for r, _ in smp.oracle_ratios(orc).values())
    assert worst <= 128.0, smp.oracle_ratios(orc)
    assert smp.M == 2.0 ** np.ceil(np.log2(8 * worst)), worst
    assert worst == pytest.approx(smp.ORACLE_WORST_RATIO, rel=0.05)
