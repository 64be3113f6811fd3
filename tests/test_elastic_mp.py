"""The mpmath reference of elastic_mp.py on configurations with closed forms, the stored file against a fresh evaluation, what the cases enter, the two layers
of the step bound, and the oracle under the tolerance the GPU tests use (which pins the margins of elastic_mp.py)."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp


def test_energies_on_closed_forms():
    mu, lam = emp.lame(1e5, 0.4)
    assert abs(mu - mpf(1e5) / mpf("2.8")) < mpf("1e-10") and abs(lam - mpf(1e5) * mpf("0.4") / (mpf("1.4") * mpf("0.2"))) < mpf("1e-9")
    I = [[mpf(i == j) for j in range(3)] for i in range(3)]
    assert emp.psi(emp.NH, I, mu, lam) == 0 and emp.psi(emp.FCR, I, mu, lam) == 0
    D = [[mpf(2), 0, 0], [0, mpf("0.5"), 0], [0, 0, mpf(3)]]
    assert abs(emp.psi(emp.NH, D, mu, lam) - (mu / 2 * (4 + mpf("0.25") + 9 - 3) - mu * mp.log(3) + lam / 2 * mp.log(3) ** 2)) < mpf("1e-90")
    assert abs(emp.psi(emp.FCR, D, mu, lam) - (mu * (1 + mpf("0.25") + 4) + lam / 2 * 4)) < mpf("1e-90")
    R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]  # a rotation changes neither; a reflection puts the sign on the smallest singular value
    assert abs(emp.psi(emp.FCR, emp._mul([[mpf(v) for v in r] for r in R], D), mu, lam) - emp.psi(emp.FCR, D, mu, lam)) < mpf("1e-90")
    assert [float(v) for v in emp.signed_singular_values([[mpf(2), 0, 0], [0, mpf(-3), 0], [0, 0, mpf("0.5")]])] == [3.0, 2.0, -0.5]
    A, vol = emp.rest(2.0 * emp.UNIT)
    assert vol == mpf(8) / 6 and A[0][0] == mpf("0.5") and A[0][1] == 0


def test_pd2d_is_the_documented_rule_not_the_eigen_projection():
    a, b, d = emp.pd2d(mpf(1), mpf(2), mpf(1))  # eigenvalues 3 and -1: the eigen-projection is 3/2 [[1, 1], [1, 1]]
    assert (a, b, d) == (mpf(4) / 3, mpf(4) / 3, mpf(4) / 3)
    assert emp.pd2d(mpf(3), mpf(1), mpf(2)) == (3, 1, 2) and emp.pd2d(mpf(-3), mpf(1), mpf(-2)) == (0, 0, 0) and emp.pd2d(mpf(2), mpf(0), mpf(-1)) == (2, 0, 0)


def test_the_cases_cover_what_they_claim():
    cs = emp.load(prefix="e_")
    by = {c["name"]: c for c in cs}
    assert len(by) == len(cs)
    for en in ("NH", "FCR"):
        for k in (1, 2, 3):
            if (en, k) != ("FCR", 3):
                assert by[f"{en} A3 with {k} negative eigenvalue(s)"]["ref_negA3"] == k
        assert list(by[f"{en} no block clamped"]["ref_branch"]) == [0, 0, 0] and by[f"{en} no block clamped"]["ref_negA3"] == 0
        assert list(by[f"{en} all three 2 x 2 blocks clamped"]["ref_branch"]) == [3, 3, 3]
        assert by[f"{en} F = I"]["ref_threshold"].all() and by[f"{en} pure rotation"]["ref_threshold"].all()
        assert np.all(by[f"{en} zero stiffness"]["ref_H"] == 0.0) and np.all(by[f"{en} zero stiffness"]["ref_g"] == 0.0)
    assert 1 in by["FCR both block eigenvalues negative"]["ref_branch"]
    assert {int(c["ref_negA3"]) for c in cs} == {0, 1, 2, 3}
    assert by["FCR inverted, s_2 -0.5"]["ref_s"][2] == pytest.approx(-0.5, rel=1e-12) and by["FCR inverted, s_2 -1e-3"]["ref_s"][2] == pytest.approx(-1e-3, rel=1e-9)
    for c in cs:  # validity: away from the kernel's clamp except the two named cases; where no 2 x 2 block is touched the rule is the 9 x 9 eigen-projection
        s = c["ref_s"]
        smin = min(s[k] + s[kp] for k, kp in emp.PAIRS)
        assert (smin < emp.SS_CLAMP) if c["name"] in emp.CLAMP_CASES else (smin >= 1e-3), c["name"]
        if not c["ref_branch"].any() and not c["ref_threshold"].any() and c["name"] not in emp.CLAMP_CASES:
            assert c["ref_gap"] < 1e-25, c["name"]
        if c["ref_threshold"].any():  # only an element at rest or rotated sits on makePD2d's discontinuity
            assert np.abs(np.abs(s) - 1.0).max() < 1e-12, c["name"]
    print("largest gap between the makePD2d rule and the 9 x 9 eigen-projection: %.3g of the block (%s)" % max((float(c["ref_gap"]), c["name"]) for c in cs))
    assert {tuple(int(k) for k in c["dtype"]).count(t) for c in cs for t in (1, 2)} >= {1, 2, 3, 4}
    # not placed, and so not covered by the GPU tests: makePD2d's `b2 == 0` branch (it needs BL == rc bit for bit) and an FCR A3 with three negative eigenvalues
    # (A3 = 2 mu I + lam (...) : a search over 0.02 <= |s_i| <= 50, either sign, at PR 0.3, 0.45, 0.49 and 0.499 finds at most two)
    assert not any(2 in c["ref_branch"] for c in cs) and "FCR A3 with 3 negative eigenvalue(s)" not in by
    st = emp.load(prefix="s_")
    assert {c["ref_path"] for c in st} == {"linear", "quadratic", "cubic"}
    assert {int(c["ref_which"]) for c in st if c["name"].startswith("three real roots")} == {0, 1, 2}
    assert {float(c["tmax"]) for c in st} == {1.0, 0.3}
    assert sum(1 for c in st if c["ref_root"] < 0) >= 2 and sum(1 for c in st if c["ref_root"] > c["tmax"]) >= 3
    assert [c["name"] for c in st if not c["layer_b"]] == ["element scale 1e-2: the quadratic path"]


def test_no_tolerance_passes_everything():
    """every Hessian check is tight: entry by entry within 1e-6 of the block's largest entry, or -- where the entries depend on the SVD basis -- the spectrum
    within 1e-6 of its largest eigenvalue; gradients within 1e-6 of their largest entry unless the element is at rest"""
    n_amb = 0
    for pre in ("e_", "b_"):
        for c in emp.load(prefix=pre):
            if c["YM"] == 0.0:
                continue
            if c["ref_ambiguous"]:
                n_amb += 1
                assert np.all(c["Xr"] == emp.UNIT) and not c["dtype"].any(), c["name"]
                assert (emp.M * (c["sens_S"] + emp.U * emp.spectrum_scale(c))).max() <= 1e-6 * emp.spectrum_scale(c), c["name"]
            else:
                assert emp.tol(c, "H").max() <= 1e-6 * c["ref_Hscale"], c["name"]
            assert emp.tol(c, "E") <= 1e-6 * c["ref_Escale"], c["name"]
            at_rest = c["ref_threshold"].any()  # no force to compare with: the force of a strain of 1e-6 instead (unit size)
            frac = 1e-3 if c["name"] in emp.CLAMP_CASES else 1e-6  # (at s_1 + s_2 = 1e-9 the polar factor of F, and with it the FCR stress, moves by 4 ulp / 1e-9)
            assert emp.tol(c, "g").max() <= frac * (c["ref_Hscale"] if at_rest else c["ref_gscale"]), c["name"]
    assert 8 <= n_amb <= 24 and not any(c["ref_ambiguous"] for c in emp.load(prefix="b_"))


def test_the_spectrum_is_read_out_of_the_block():
    by = {c["name"]: c for c in emp.load(prefix="e_")}
    for nm in ("NH uniform scale 0.5", "FCR uniform scale 0.5, rotated", "NH two equal singular values, rotated"):
        c = by[nm]
        assert c["ref_ambiguous"] and emp.spectrum_ratio(c, c["ref_H"]) <= 32.0, nm
        assert emp.spectrum_ratio(c, 0.999999 * c["ref_H"]) > emp.M and emp.hessian_ratio(c, np.zeros((12, 12))) > emp.M
    c = by["NH F = I"]  # on the threshold: either outcome of each block, nothing else
    assert emp.spectrum_ratio(c, c["ref_H"]) <= 32.0 and emp.hessian_ratio(c, 0.75 * c["ref_H"]) > emp.M


def test_step_cases_are_valid_and_the_layers_agree():
    """step_reference asserts layer (a) == layer (b) wherever the case has a layer (b)"""
    for c in emp.load(prefix="s_"):
        assert emp.step_valid(c), c["name"]
        r = emp.step_reference(c)
        assert r["bound"] == c["ref_bound"] and r["path"] == c["ref_path"], c["name"]


def test_stored_references_are_current():
    """a fixed random sample of the cases evaluated afresh from the inputs IN the file, and the generator's inputs against the file's: a stale file fails"""
    cs = emp.load(prefix="e_")
    fresh = emp.element_cases()
    assert [c["name"] for c in fresh] == [c["name"] for c in cs]
    for a, b in zip(fresh, cs):
        assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Xr"], b["Xr"]) and a["YM"] == b["YM"] and a["PR"] == b["PR"], a["name"]
    for a, b in zip(emp.step_cases(), emp.load(prefix="s_")):
        assert a["name"] == b["name"] and np.array_equal(a["X"], b["X"]) and np.array_equal(a["P"], b["P"]) and a["tmax"] == b["tmax"]
    blk = emp.load(prefix="b_")
    for a, b in zip(emp.block_cases(), blk):
        assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Xr"], b["Xr"])
    for cs, i, seed0 in ((cs, 22, 0), (blk, 7, 2000)):  # one case of each family (an evaluation at 100 digits takes about a second)
        ref, sens = emp.evaluate_element(cs[i], emp.reference_seed(seed0 + i))
        for k in ("E", "g", "H"):
            assert np.all(np.abs(np.asarray(ref[k]) - cs[i]["ref_" + k]) <= 1e-15 * np.abs(cs[i]["ref_" + k])), (cs[i]["name"], k)
            assert np.all(np.abs(sens[k] - cs[i]["sens_" + k]) <= 1e-12 * np.abs(cs[i]["sens_" + k])), (cs[i]["name"], k)


def test_oracle_meets_the_tolerance(orc):
    """the margin: M = 8 x the oracle's worst err / (sens + u scale), rounded up to a power of two; no case may need more than 100 x the median of its quantity
    (the two Hessians inside the clamp have their own measured margin, see elastic_mp.py)"""
    r = emp.oracle_ratios(orc)
    print({k: "worst %.3g (%s), median %.3g" % v for k, v in r.items()}, "M =", emp.M, "M_CLAMP_H =", emp.M_CLAMP_H)
    worst = max(r[k][0] for k in ("E", "g", "H", "bound"))
    assert r["H"][0] <= 100 * r["H"][2] and r["g"][0] <= 100 * r["g"][2] and r["E"][0] <= 100 * r["E"][2], r
    assert emp.M == 2.0 ** np.ceil(np.log2(8 * worst)), worst
    assert worst == pytest.approx(emp.ORACLE_WORST_RATIO, rel=0.05)
    assert r["H clamp"][0] == pytest.approx(emp.CLAMP_H_RATIO, rel=0.05) and emp.M_CLAMP_H == 2.0 ** np.ceil(np.log2(8 * r["H clamp"][0]))
