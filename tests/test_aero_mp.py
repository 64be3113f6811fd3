"""The mpmath restatement of the air-drag potential (tests/aero_mp.py) pinned by itself: the gradient against mp.diff of D, the Hessian against mp.diff of
the gradient, its smallest eigenvalue, the momentum identity, what the named cases are, and the tolerance constant M against the recorded error of the
float64 restatement.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import aero_mp as am

TINY = mpf(10) ** -25
CASES = am.cases()
BY = {c["name"]: c for c in CASES}
NAMES = ["u = 0", "pure normal flow", "pure tangential flow", "oblique flow", "one-sided, leeward", "one-sided, exactly at u_n = 0", "sliver",
         "far from the origin", "Dirichlet nodes", "Dirichlet nodes moved, dt = 1e-4"]


def _D(case, flat):
    """D of the whole case (mpmath) at the positions `flat` (3 nV mpf numbers)"""
    x = [flat[3 * i:3 * i + 3] for i in range(len(case["x"]))]
    return am.reference(am.MP, case, x)["E"]


def _grad(case, flat):
    x = [flat[3 * i:3 * i + 3] for i in range(len(case["x"]))]
    return am.reference(am.MP, case, x)["g"]


def _scales(case):
    m = am.reference(am.MP, case, magnitudes=True)
    u = max(abs(v) for t, lag in zip(case["tri"], case["lag"])
            for v in am.triangle(am.MP, [[mpf(float(q)) for q in case["x"][int(i)]] for i in t], [mpf(float(q)) for q in lag], mpf(float(case["cn"])), mpf(float(case["ct"])),
                                 bool(case["one"]), [mpf(float(q)) for q in case["w"]], mpf(float(case["rho"])), mpf(float(case["dt"])))["u"])
    return max(m["g"]) + 1, max(max(r) for r in m["H"]) + 1, u


@pytest.mark.parametrize("name", NAMES)
def test_gradient_and_hessian_against_mp_diff_eigenvalues_and_momentum(name):
    case = BY[name]
    n3 = 3 * len(case["x"])
    x = [mpf(float(v)) for v in case["x"].ravel()]
    r = am.reference(am.MP, case)
    sg, sH, _ = _scales(case)
    # mp.diff steps by about 10^-(dps / 2) relative to the unit: at u = 0 (|u|^3, C2 but not C3) its quotient is of the order of that step, no rounding
    # error -- covered by the 1e-15 (sH, the curvature scale, times the step) below, which is far under anything the float64 tolerances resolve
    slack = mpf(10) ** -15
    for a in range(n3):
        d = mp.diff(lambda t: _D(case, x[:a] + [t] + x[a + 1:]), x[a])
        assert abs(d - r["g"][a]) <= slack * sg, (name, a, d, r["g"][a])
    for a in range(n3):
        for b in range(n3):
            d = mp.diff(lambda t: _grad(case, x[:b] + [t] + x[b + 1:])[a], x[b])
            assert abs(d - r["H"][a][b]) <= slack * sH * 1e3, (name, a, b, d, r["H"][a][b])
            assert abs(r["H"][a][b] - r["H"][b][a]) <= TINY * sH  # symmetric (to the working precision)
    w = mp.eigsy(mp.matrix(r["H"]), eigvals_only=True)
    assert min(w) >= -TINY * sH, (name, min(w))  # PSD as it stands: no projection
    # momentum: the nodal forces of every triangle sum to the force on its centroid, -(rho A / 2) (Cn |s_n| s_n n + Ct |u_t| u_t), stated here on its own
    total = [mpf(0)] * 3
    for t, lag in zip(case["tri"], case["lag"]):
        q = am.triangle(am.MP, [[mpf(float(v)) for v in case["x"][int(i)]] for i in t], [mpf(float(v)) for v in lag], mpf(float(case["cn"])), mpf(float(case["ct"])),
                        bool(case["one"]), [mpf(float(v)) for v in case["w"]], mpf(float(case["rho"])), mpf(float(case["dt"])))
        n, A = [mpf(float(v)) for v in lag[:3]], mpf(float(lag[3]))
        ut = [q["u"][a] - q["un"] * n[a] for a in range(3)]
        for a in range(3):
            f = -(mpf(float(case["rho"])) * A / 2) * (mpf(float(case["cn"])) * abs(q["sn"]) * q["sn"] * n[a] + mpf(float(case["ct"])) * q["lt"] * ut[a])
            total[a] += f
    nodal = [-sum(r["g"][3 * k + a] for k in range(len(case["x"]))) for a in range(3)]
    forces = [sum(row[a] for row in r["F"]) for a in range(3)]
    for a in range(3):
        assert abs(nodal[a] - total[a]) <= TINY * sg and abs(forces[a] - total[a]) <= TINY * sg
    assert r["power"] >= 0


def test_the_named_cases_are_what_their_names_say():
    assert [c["name"] for c in CASES] == NAMES
    q = {}
    for c in CASES:
        q[c["name"]] = [am.triangle(am.MP, [[mpf(float(v)) for v in c["x"][int(i)]] for i in t], [mpf(float(v)) for v in lag], mpf(float(c["cn"])), mpf(float(c["ct"])),
                                    bool(c["one"]), [mpf(float(v)) for v in c["w"]], mpf(float(c["rho"])), mpf(float(c["dt"]))) for t, lag in zip(c["tri"], c["lag"])]
    t = q["u = 0"][0]
    c = BY["u = 0"]
    assert np.array_equal(c["x"], c["X"]) and np.all(c["w"] == 0)
    # in mpmath the exact centroid differs from the float64 record by that record's rounding, so u is a rounding over dt there; in float64 -- the kernels'
    # arithmetic: the same sums in the same order on both sides -- it is exactly zero and nothing is on
    assert max(abs(v) for v in t["u"]) <= 2 * am.U * np.abs(c["x"]).max() / c["dt"]
    f = am.triangle(am.NP, [[float(v) for v in c["x"][int(i)]] for i in c["tri"][0]], [float(v) for v in c["lag"][0]], float(c["cn"]), float(c["ct"]), False,
                    [0.0] * 3, float(c["rho"]), float(c["dt"]))
    assert all(v == 0.0 for v in f["u"]) and not f["nOn"] and not f["tOn"] and f["E"] == 0.0 and all(v == 0.0 for v in f["g"]) and all(v == 0.0 for r in f["K9"] for v in r)
    t = q["pure normal flow"][0]
    assert abs(t["un"]) > 2 and t["lt"] < 1e-12 * abs(t["un"])
    t = q["pure tangential flow"][0]
    assert t["lt"] > 1.5 and abs(t["un"]) < 1e-12 * t["lt"] and not BY["pure tangential flow"]["one"]
    t = q["oblique flow"][0]
    assert t["un"] > 1 and t["lt"] > 0.3 and BY["oblique flow"]["one"] and t["nOn"] and t["tOn"]
    t = q["one-sided, leeward"][0]
    assert t["un"] < -1 and t["sn"] == 0 and not t["nOn"] and not t["tOn"] and BY["one-sided, leeward"]["ct"] == 0  # nothing is written at all
    t = q["one-sided, exactly at u_n = 0"][0]
    assert t["un"] == 0 and not t["nOn"] and t["tOn"] and t["lt"] > 0.5 and np.array_equal(BY["one-sided, exactly at u_n = 0"]["lag"][0][:3], [0.0, 0.0, 1.0])
    s = BY["sliver"]
    edge = max(np.linalg.norm(s["X"][i] - s["X"][j]) for i, j in ((0, 1), (1, 2), (2, 0)))
    assert 0.3e-6 < s["lag"][0][3] / edge ** 2 < 3e-6
    f = BY["far from the origin"]
    assert np.abs(f["x"]).min() > 1e3 * 0.24 and max(np.linalg.norm(f["X"][i] - f["X"][j]) for i, j in ((0, 1), (1, 2), (2, 0))) < 0.3
    for name in ("Dirichlet nodes", "Dirichlet nodes moved, dt = 1e-4"):
        assert sorted(BY[name]["dbc"].tolist()) == [0, 0, 1, 2] and len(BY[name]["tri"]) == 2
    mv = BY["Dirichlet nodes moved, dt = 1e-4"]
    moved = np.any(mv["x"] != mv["X"], axis=1)
    assert mv["dt"] == 1e-4 and np.array_equal(moved, mv["dbc"] > 0)  # only the Dirichlet nodes move, and their motion loads the triangles
    assert all(t["nOn"] for t in q["Dirichlet nodes moved, dt = 1e-4"])
    for c in CASES:  # the unit normals are unit, the areas positive
        for lag in c["lag"]:
            assert abs(np.linalg.norm(lag[:3]) - 1) < 1e-9 and lag[3] > 0 and lag[7] == 0


def test_rest_record_against_mpmath():
    """the float64 record the plan states: within a few ulp of the mpmath record, relative to |e1| |e2| for the normal of a sliver (its cross product cancels)"""
    for c in CASES:
        for t, lag in zip(c["tri"], c["lag"]):
            X = [c["X"][int(i)] for i in t]
            n, A, cen = am.record_mp(*X)
            e1, e2 = np.linalg.norm(X[1] - X[0]), np.linalg.norm(X[2] - X[0])
            cancel = e1 * e2 / (2 * float(A))  # how much of the cross product cancels; each edge carries the rounding of a subtraction of coordinates of size |X|
            rel = 8 * am.U * cancel * (1 + np.abs(np.array(X)).max() / min(e1, e2))
            assert all(abs(mpf(float(lag[a])) - n[a]) <= rel for a in range(3)), c["name"]
            assert abs(mpf(float(lag[3])) - A) <= rel * float(A)
            assert all(abs(mpf(float(lag[4 + a])) - cen[a]) <= 3 * am.U * np.abs(np.array(X)[:, a]).max() for a in range(3))


def test_stored_cases_match_the_generator():
    stored = am.load()
    assert [c["name"] for c in stored] == NAMES
    for s, c in zip(stored, CASES):
        for k in am.INPUTS:
            assert np.array_equal(np.asarray(s[k]), np.asarray(c[k])), (c["name"], k)
    r = am.evaluate(CASES[3])
    for k in am.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[3][k]))
    assert len(am.environments(stored)) >= 3


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in am.load():
        n = am.numpy_restatement(c)
        for k in am.QUANT:
            worst = max(worst, float(np.max(am.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + am.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= am.NUMPY_WORST_RATIO * 1.01
    assert am.M == 2.0 ** np.ceil(np.log2(8 * am.NUMPY_WORST_RATIO))
