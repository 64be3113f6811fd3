"""Pins tests/fiber_mp.py, the mpmath reference of the fibre energy (ipc_amd/csrc/fiber_kernels.h), on the CPU: the gradient is the mp derivative of W, the
unclamped Hessian the derivative of the gradient, the clamped Hessian is PSD and equals the unclamped one wherever psi'' >= 0 and psi' >= 0, W is invariant and
the gradient covariant under a rigid rotation; the float64 restatement meets the tolerance the GPU tests use."""
import numpy as np
import pytest
from mpmath import mp, mpf

import fiber_mp as fm

EV = fm.evaluated()
IDS = [c["name"] for c, _ in EV]
DIFF_TOL = mpf(10) ** -30  # mp.diff at 50 digits


def _smooth(c, r):
    """cases where W is twice differentiable at x with a margin: not l == 0, not the exponent's overflow, not within rounding of a tension-only threshold"""
    el, l = c["elems"][0], r["len"][0]
    if not l > 0 or c["overflow"]:
        return False
    edge = 1.0 if el["law"] == fm.EXP else el["l0"] if el["tension_only"] else None
    return edge is None or abs(l - edge) > 1e-9


def _W(c, flat):
    x = [[flat[3 * i + a] for a in range(3)] for i in range(len(c["x"]))]
    return fm.reference(fm.MP, c, x)[0]


def _g(c, flat, project=False):
    x = [[flat[3 * i + a] for a in range(3)] for i in range(len(c["x"]))]
    return fm.reference(fm.MP, c, x, project=project)


def _partial(f, flat, j):
    return mp.diff(lambda v: f(flat[:j] + [v] + flat[j + 1:]), flat[j])


def test_the_cases_cover_what_the_issue_lists():
    names = " | ".join(IDS)
    for needle in ("l = l0 to rounding", "1 - 1e-6", "1 + 1e-6", "tensiononly True", "tensiononly False", "l = 0.8 < 1", "l = 3", "overflows", "l = 0", "oblique",
                   "act -0.2", "act 0.0", "act 0.3", "sliver"):
        assert needle in names, needle
    c, r = next(e for e in EV if e[0]["overflow"])
    assert r["E"] == np.inf and not np.isnan(r["E"])
    assert [r["len"][0] for c, r in EV if c["name"].startswith("l = 0")] == [0.0, 0.0]


@pytest.mark.parametrize("c,r", [e for e in EV if _smooth(*e)], ids=[e[0]["name"] for e in EV if _smooth(*e)])
def test_gradient_and_hessian_are_the_derivatives(c, r):
    flat = [mpf(float(v)) for v in c["x"].ravel()]
    _, g, H, _, _ = _g(c, flat)
    gs = max(max(abs(v) for v in g), mpf(1))
    Hs = max(max(abs(v) for row in H for v in row), mpf(1))
    for j in range(12):
        assert abs(_partial(lambda f: _W(c, f), flat, j) - g[j]) <= DIFF_TOL * gs, j
    for j in range(12):
        dg = mp.diff(lambda v: mp.matrix(_g(c, flat[:j] + [v] + flat[j + 1:])[1]), flat[j])
        for i in range(12):
            assert abs(dg[i] - H[i][j]) <= DIFF_TOL * Hs, (i, j)


@pytest.mark.parametrize("c,r", [e for e in EV if not e[0]["overflow"]], ids=[e[0]["name"] for e in EV if not e[0]["overflow"]])
def test_clamped_hessian_is_psd_and_equals_the_full_one_where_nothing_is_clamped(c, r):
    flat = [mpf(float(v)) for v in c["x"].ravel()]
    _, _, Hc, _, _ = _g(c, flat, project=True)
    _, _, Hf, _, _ = _g(c, flat, project=False)
    Hs = max(max(abs(v) for row in Hc for v in row), mpf(1))
    ev = mp.eigsy(mp.matrix(Hc), eigvals_only=True)
    assert min(ev) >= -DIFF_TOL * Hs
    assert max(abs(Hc[i][j] - Hc[j][i]) for i in range(12) for j in range(12)) <= DIFF_TOL * Hs  # symmetric (to mp rounding)
    el = c["elems"][0]
    x = [[mpf(float(v)) for v in row] for row in c["x"]]
    _, _, _, l, d1 = fm.element(fm.MP, [mpf(float(v)) for v in el["b"]], x, mpf(el["vk"]), mpf(el["k2"]), el["law"], el["tension_only"], mpf(el["l0"]))
    d2 = fm.law(fm.MP, l, mpf(el["vk"]), mpf(el["k2"]), el["law"], el["tension_only"], mpf(el["l0"]))[2]
    if (d1 >= 0 and d2 >= 0) or not l > 0:  # (l == 0: no block either way)
        assert all(Hc[i][j] == Hf[i][j] for i in range(12) for j in range(12))
    else:  # a compressed spring fibre: the transverse eigenvalue psi' / l is negative and clamped
        assert min(mp.eigsy(mp.matrix(Hf), eigvals_only=True)) < 0


@pytest.mark.parametrize("c,r", [e for e in EV if not e[0]["overflow"]], ids=[e[0]["name"] for e in EV if not e[0]["overflow"]])
def test_rigid_rotation(c, r):
    Q = mp.matrix(fm._R([0.3, -1.0, 0.7], 61.0).tolist())
    q, _ = mp.qr(Q)  # (the float64 rotation is orthogonal to 1e-16 only: orthonormalised in mp)
    x = [mp.matrix([mpf(float(v)) for v in row]) for row in c["x"]]
    xr = [list(q * v) for v in x]
    E0, g0, _, _, _ = fm.reference(fm.MP, c, [list(v) for v in x])
    E1, g1, _, _, _ = fm.reference(fm.MP, c, xr)
    assert abs(E1 - E0) <= DIFF_TOL * max(abs(E0), mpf(1))
    gs = max(max(abs(v) for v in g0), mpf(1))
    for i in range(4):
        rot = q * mp.matrix(g0[3 * i:3 * i + 3])
        assert max(abs(rot[a] - g1[3 * i + a]) for a in range(3)) <= DIFF_TOL * gs


@pytest.mark.parametrize("c,r", EV, ids=IDS)
def test_numpy_restatement_meets_the_tolerance(c, r):
    n = fm.numpy_restatement(c)
    if c["overflow"]:
        assert n["E"] == np.inf and r["E"] == np.inf
        return
    for k in ("E", "g", "H", "perW"):
        worst = float(np.max(fm.ratio(np.asarray(n[k]) - np.asarray(r[k]), np.asarray(fm.tolerance(r, k)) / fm.M)))
        assert worst <= fm.M, (k, worst)
        assert not np.any(np.isnan(np.asarray(n[k])))


def test_b_is_A_a_and_F_a():
    """b = A a gives F a = sum c_i x_i: against numpy's F = Ds A"""
    for c, r in EV:
        A9, vol = fm.rest_inputs(c["X"], c["T"][0])
        A = A9.reshape(3, 3, order="F")
        a = fm.unit(c["a"])
        assert np.allclose(c["elems"][0]["b"], A @ a, rtol=1e-14, atol=0)
        Ds = np.column_stack([c["x"][i] - c["x"][0] for i in (1, 2, 3)])
        l = np.linalg.norm(Ds @ A @ a)
        assert abs(l - r["len"][0]) <= 1e-9 * max(1.0, np.abs(A).max() * np.abs(c["x"]).max())
