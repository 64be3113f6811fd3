"""The mpmath restatement of the shell energies (tests/shell_mp.py) pinned by itself: derivatives against mp.diff, rigid motions, a closed form, hand-placed
hinges; and the tolerance constant M against the recorded error of the float64 restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import shell_mp as smp

H, YM, PR = mpf("0.01"), mpf(1e5), mpf("0.3")


def _mpv(A):
    return [[mpf(float(v)) for v in r] for r in np.asarray(A)]


def _flat_diff(fun, x, k):
    """d fun / d (coordinate k) at the flattened point x (list of mpf)"""
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


TRI_CASES = [c for c in smp.cases() if len(c["tri"]) == 1]
HINGE_CASES = [c for c in smp.cases() if len(c["tri"]) == 2]


@pytest.mark.parametrize("case", TRI_CASES[1:7], ids=lambda c: c["name"])
def test_membrane_gradient_and_unprojected_hessian_against_mp_diff(case):
    X, x = _mpv(case["X"]), [v for r in _mpv(case["x"]) for v in r]
    E = lambda f: smp.membrane(smp.MP, X, _rows(f), H, YM, PR, hessian=False)[0]
    _, g, Hm = smp.membrane(smp.MP, X, _rows(x), H, YM, PR, project=False)
    for k in range(9):
        assert abs(_flat_diff(E, x, k) - g[k]) <= mpf(10) ** -30 * (1 + abs(g[k]))
        for l in range(9):
            d = _flat_diff(lambda f: smp.membrane(smp.MP, X, _rows(f), H, YM, PR, hessian=False)[1][k], x, l)
            assert abs(d - Hm[k][l]) <= mpf(10) ** -28 * (1 + abs(Hm[k][l]))


@pytest.mark.parametrize("case", HINGE_CASES[1:4] + HINGE_CASES[6:9], ids=lambda c: c["name"])
def test_hinge_gradient_against_mp_diff(case):
    X, x = _mpv(case["X"]), [v for r in _mpv(case["x"]) for v in r]
    mat = ((H, YM, PR), (2 * H, 3 * YM, mpf("0.2")))
    E = lambda f: smp.hinge(smp.MP, X, _rows(f), mat, mpf(1))[0]
    e, g, Hg = smp.hinge(smp.MP, X, _rows(x), mat, mpf(1))
    thetaBar, w, kb = smp.hinge_constants(smp.MP, X, mat)
    theta, gt = smp.hinge_angle(smp.MP, _rows(x), True)
    for k in range(12):
        assert abs(_flat_diff(E, x, k) - g[k]) <= mpf(10) ** -30 * (1 + abs(g[k]))
        for l in range(12):
            assert abs(Hg[k][l] - 2 * kb * w * gt[k] * gt[l]) <= mpf(10) ** -40 * (1 + abs(Hg[k][l]))  # Gauss-Newton: rank one


def test_zero_energy_and_gradient_at_rest_and_under_rigid_motion():
    R, t = smp.rot([2, -1, 3], 73.0), np.array([0.3, -0.2, 0.5])
    for c in (TRI_CASES[0], HINGE_CASES[0], [c for c in HINGE_CASES if c["name"] == "hinge rest 40 at 40"][0]):
        for x in (c["X"], c["X"] @ R.T + t):
            E, g, _ = smp.patch_reference(smp.MP, dict(c, x=x))
            scale = float(smp.patch_reference(smp.MP, dict(c, x=x), magnitudes=True)[0])
            assert abs(float(E)) <= 1e-28 * scale  # (the rotation matrix is float64: |R^T R - I| ~ 1e-16, squared in the energy)
            assert max(abs(float(v)) for v in g) <= 1e-13 * scale


def test_equal_biaxial_stretch_closed_form():
    X = _mpv(TRI_CASES[0]["X"])
    c = [sum(X[k][i] for k in range(3)) / 3 for i in range(3)]
    mu, lam = smp.lame(YM, PR)
    _, A = smp.rest_triangle(smp.MP, X)
    for s in (mpf("0.5"), mpf("0.9"), mpf("1.3"), mpf(2)):
        x = [[c[i] + s * (X[k][i] - c[i]) for i in range(3)] for k in range(3)]
        E = smp.membrane(smp.MP, X, x, H, YM, PR, hessian=False)[0]
        want = H * A * (mu + lam) * (s * s - 1) ** 2 / 2
        assert abs(E - want) <= mpf(10) ** -40 * want


def test_hand_placed_hinge_angles():
    for deg in (0, 90, -90, 170, -170):
        theta, _ = smp.hinge_angle(smp.MP, _mpv(smp.hinge_nodes(deg)))
        assert abs(float(theta) - np.radians(deg)) <= 1e-15 * max(1.0, abs(np.radians(deg))) * 4
    # +90 degrees by hand: triangle (x0, x1, x2) in z = 0 with x2 at y > 0, the other triangle standing on the edge
    theta, _ = smp.hinge_angle(smp.MP, _mpv([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1]]))
    assert abs(theta - mp.pi / 2) <= mpf(10) ** -45


def test_projected_membrane_hessian_is_psd_and_clamps_under_compression():
    c = [c for c in TRI_CASES if c["name"] == "triangle compressed"][0]
    X, x = _mpv(c["X"]), _mpv(c["x"])
    raw = np.array(smp.membrane(smp.MP, X, x, H, YM, PR, project=False)[2], dtype=object).astype(np.float64)
    proj = np.array(smp.membrane(smp.MP, X, x, H, YM, PR)[2], dtype=object).astype(np.float64)
    assert np.linalg.eigvalsh(raw).min() < -1e-3 * np.abs(raw).max()
    assert np.linalg.eigvalsh(proj).min() > -1e-12 * np.abs(proj).max()


def test_stored_cases_match_the_generator():
    stored, now = smp.load(), smp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in ("X", "x", "tri", "h", "YM", "PR", "dbc"):
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = smp.evaluate(now[2])
    for k in smp.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[2][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in smp.load():
        n = smp.numpy_restatement(c)
        for k in smp.QUANT:
            worst = max(worst, float(np.max(np.abs(n[k] - c[k]) / (np.asarray(c["sens_" + k]) + smp.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= smp.NUMPY_WORST_RATIO * 1.01
    assert smp.M == 2.0 ** np.ceil(np.log2(8 * smp.NUMPY_WORST_RATIO))
