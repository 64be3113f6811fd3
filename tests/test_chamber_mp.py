"""The mpmath restatement of the pressure-chamber energy (tests/chamber_mp.py) pinned by itself: derivatives against mp.diff, the projection against
mp.eigsy, what a closed surface guarantees (no dependence on the reference point or a translation, zero net force and torque), the unit cube, the
eigenvalue gap of the stored cases, and the tolerance constant M against the recorded error of the float64 restatement.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import chamber_mp as cm
from rod_mp import rot

TINY = mpf(10) ** -25
BY = {c["name"]: c for c in cm.cases()}


def _tri_inputs(case, t):
    ids = [int(v) for v in case["tri"][t]]
    return [[mpf(float(v)) for v in case["x"][i]] for i in ids], [mpf(float(v)) for v in case["r"]], mpf(float(case["p"]))


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(3)]


def _flat_diff(fun, x, k):
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


@pytest.mark.parametrize("name,t", [("tetrahedron", 3), ("negative pressure", 2)])
def test_gradient_and_hessian_against_mp_diff_and_projection_against_eigsy(name, t):
    xr, r, p = _tri_inputs(BY[name], t)
    x = [v for row in xr for v in row]
    E = lambda f: cm.triangle(cm.MP, _rows(f), r, p)[0]
    _, g, Hp = cm.triangle(cm.MP, xr, r, p)
    full = cm.triangle(cm.MP, xr, r, p, project=False)[2]
    scale = abs(p)
    Hd = mp.matrix(9, 9)
    for a in range(9):
        assert abs(_flat_diff(E, x, a) - g[a]) <= TINY * scale
        for b in range(9):
            Hd[a, b] = _flat_diff(lambda f: cm.triangle(cm.MP, _rows(f), r, p)[1][a], x, b)
    w, Q = mp.eigsy((Hd + Hd.T) / 2)
    assert abs(sum(w)) <= TINY * scale and min(w) < 0 < max(w)  # trace 0: indefinite
    for a in range(9):
        for b in range(9):
            assert abs(full[a][b] - Hd[a, b]) <= TINY * scale
            clamped = sum(Q[a, m] * (w[m] if w[m] > 0 else 0) * Q[b, m] for m in range(9))
            assert abs(Hp[a][b] - clamped) <= TINY * scale
    for I in range(3):  # the stated blocks: zero diagonal blocks
        assert all(full[3 * I + a][3 * I + b] == 0 for a in range(3) for b in range(3))
    assert min(mp.eigsy(mp.matrix(Hp), eigvals_only=True)) >= -TINY * scale  # PSD


def _moved(case, x, r=None):
    return dict(case, x=np.asarray(x, dtype=np.float64), r=case["r"] if r is None else np.asarray(r, dtype=np.float64))


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "two cubes in one chamber"])
def test_closed_surface_ignores_reference_point_and_translation_and_has_no_net_force_or_torque(name):
    case = BY[name]
    n = len(case["x"])
    E0, g0, _ = cm.reference(cm.MP, case, project=False)
    mag = cm.reference(cm.MP, case, magnitudes=True)
    G0 = np.array(g0, dtype=object).reshape(n, 3)
    X = np.array([[mpf(float(v)) for v in row] for row in case["x"]], dtype=object)
    # zero net force and torque (exactly, up to the working precision: the float64 inputs are exact numbers)
    assert max(abs(v) for v in G0.sum(axis=0)) <= TINY * float(max(mag[1]))
    torque = sum((np.array(cm._cross(list(X[i]), list(G0[i])), dtype=object) for i in range(n)), np.array([mpf(0)] * 3, dtype=object))
    assert max(abs(v) for v in torque) <= TINY * float(max(mag[1]))
    # another reference point: V (= -E / p) and the gradient stay
    E1, g1, _ = cm.reference(cm.MP, _moved(case, case["x"], case["r"] + [0.7, -1.3, 2.1]), project=False)
    assert abs(E1 - E0) <= TINY * float(mag[0]) * 1e3 and max(abs(a - b) for a, b in zip(g1, g0)) <= TINY * float(max(mag[1])) * 1e3
    # a translation, carried out in mpmath (exact), with r left behind
    E2, g2, _ = cm.reference(cm.MP, dict(case, x=[[v + mpf(4) for v in row] for row in X]), project=False)
    assert abs(E2 - E0) <= TINY * float(mag[0]) * 1e4 and max(abs(a - b) for a, b in zip(g2, g0)) <= TINY * float(max(mag[1])) * 1e4
    # a rotation about r rotates the gradient (the rotation matrix and the moved coordinates are float64: relative 1e-15)
    R = rot([2, -1, 3], 73.0)
    E3, g3, _ = cm.reference(cm.MP, _moved(case, (case["x"] - case["r"]) @ R.T + case["r"]), project=False)
    Rm = np.array([[mpf(float(v)) for v in row] for row in R], dtype=object)
    assert abs(E3 - E0) <= 1e-13 * float(mag[0])
    assert max(abs(v) for v in (np.array(g3, dtype=object).reshape(n, 3) - G0 @ Rm.T).ravel()) <= 1e-13 * float(max(mag[1]))


def test_unit_cube_volume_and_the_plan_restatements():
    unit = {"x": cm.CUBE_X, "tri": cm.CUBE_TRI, "r": cm.ref_point(cm.CUBE_X, cm.CUBE_TRI), "p": 1.0}
    V, A, _, _ = cm.volume_area(unit)
    assert abs(V - 1) <= TINY and abs(A - 6) <= TINY  # (the division by 6 rounds at the working precision, whatever another module has set it to)
    assert np.array_equal(unit["r"], [0.5, 0.5, 0.5]) and cm.rest_volume(cm.CUBE_X, cm.CUBE_TRI, unit["r"]) == 1.0
    tet = {"x": cm.TET_X, "tri": cm.TET_TRI, "r": cm.ref_point(cm.TET_X, cm.TET_TRI), "p": 1.0}
    assert abs(cm.volume_area(tet)[0] - mpf(1) / 6) <= TINY
    assert cm.rest_volume(cm.CUBE_X, cm.CUBE_TRI[:, ::-1], unit["r"]) == -1.0  # inward
    for c in cm.cases():  # every stored chamber is outward and E = -p V
        assert cm.rest_volume(c["x"], c["tri"], c["r"]) > 0
        assert abs(cm.reference(cm.MP, c)[0] + mpf(float(c["p"])) * cm.volume_area(c)[0]) <= TINY * (1 + abs(float(c["p"])))


def test_eigenvalues_of_every_triangle_stay_away_from_zero():
    """the projection is not evaluated at its kink: smallest |lambda| at least 1e-3 of the largest, per triangle of every pressurised case"""
    for c in cm.cases():
        if c["p"] == 0.0:
            continue
        w = np.abs(cm.triangle_eigenvalues(c))
        assert np.all(w.min(axis=1) >= 1e-3 * w.max(axis=1)), (c["name"], (w.min(axis=1) / w.max(axis=1)).min())


def test_stored_cases_match_the_generator():
    stored, now = cm.load(), cm.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    assert [c["name"] for c in now] == ["tetrahedron", "cube", "cube far from the origin", "negative pressure", "zero pressure", "Dirichlet nodes",
                                        "two cubes in one chamber"]
    for s, c in zip(stored, now):
        for k in cm.INPUTS:
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = cm.evaluate(now[0])
    for k in cm.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[0][k]))
    far = BY["cube far from the origin"]
    assert np.linalg.norm(far["r"]) > 1e3 * 0.25 and np.abs(far["r"] - far["x"].mean(axis=0)).max() < 0.05  # r at the body, ~1e3 edge lengths out
    assert sorted(BY["Dirichlet nodes"]["dbc"].tolist())[-2:] == [1, 2]


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in cm.load():
        n = cm.numpy_restatement(c)
        for k in cm.QUANT:
            worst = max(worst, float(np.max(cm.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + cm.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= cm.NUMPY_WORST_RATIO * 1.01
    assert cm.M == 2.0 ** np.ceil(np.log2(8 * cm.NUMPY_WORST_RATIO))
