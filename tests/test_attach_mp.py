"""The mpmath restatement of the attachment energy (tests/attach_mp.py) pinned by itself: derivatives against mp.diff, the closed-form clamp against
mp.eigsy, rigid motions, the closed forms of a stitch, coincident points; and the tolerance constant M against the recorded error of the float64
restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import attach_mp as amp
from rod_mp import rot

TINY = mpf(10) ** -25


def _one(case, i=0):
    """(c, x rows as mpf, k, L) of attachment i of a case"""
    ids, c = amp.stencils(case)[i]
    return [mpf(v) for v in c], [[mpf(float(v)) for v in case["x"][n]] for n in ids], mpf(float(case["k"][i])), mpf(float(case["L"][i]))


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


def _flat_diff(fun, x, k):
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


BY = {c["name"]: c for c in amp.cases()}
SMOOTH = ["node - node, stitch", "node - node, stretched", "node - node, compressed", "node - edge point", "node - triangle point",
          "edge point - triangle point", "one node in both points"]


@pytest.mark.parametrize("name", SMOOTH)
def test_gradient_and_clamped_hessian_against_mp_diff_and_eigsy(name):
    """the gradient against mp.diff; the unprojected Hessian against mp.diff of the gradient; the projected one is PSD and equals the mp.eigsy
    decomposition of the full one with its eigenvalues clamped at 0; the spectrum of the full Hessian is |c|^2 x (k, k (1 - L / l) twice) and zeros"""
    c, xr, k, L = _one(BY[name])
    x = [v for r in xr for v in r]
    n = len(x)
    E = lambda f: amp.spring(amp.MP, c, _rows(f), k, L)[0]
    _, g, Hc, l, force = amp.spring(amp.MP, c, xr, k, L)
    full = amp.spring(amp.MP, c, xr, k, L, project=False)[2]
    Hd = mp.matrix(n, n)
    for a in range(n):
        assert abs(_flat_diff(E, x, a) - g[a]) <= mpf(10) ** -30 * (1 + abs(g[a]))
        for b in range(n):
            Hd[a, b] = _flat_diff(lambda f: amp.spring(amp.MP, c, _rows(f), k, L)[1][a], x, b)
    Hd = (Hd + Hd.T) / 2
    w, Q = mp.eigsy(Hd)
    c2 = sum(v * v for v in c)
    side = k * (1 - L / l) if L > 0 else k
    want = sorted([c2 * k, c2 * side, c2 * side] + [mpf(0)] * (n - 3))
    for a, b in zip(sorted(w), want):
        assert abs(a - b) <= TINY * k
    for a in range(n):
        for b in range(n):
            clamped = sum(Q[a, m] * (w[m] if w[m] > 0 else 0) * Q[b, m] for m in range(n))
            assert abs(full[a][b] - Hd[a, b]) <= TINY * k
            assert abs(Hc[a][b] - clamped) <= TINY * k
    wc = mp.eigsy(mp.matrix(Hc), eigvals_only=True)
    assert min(wc) >= -TINY * k  # PSD
    assert (min(w) < -mpf(10) ** -3 * k) == (name == "node - node, compressed")  # the clamp acts exactly on the compressed spring
    assert abs(force - k * (l - L)) <= TINY * k


def test_invariance_under_rigid_motion():
    R, t = rot([2, -1, 3], 73.0), np.array([0.3, -0.2, 0.5])
    for name in ("edge point - triangle point", "triangle point - triangle point", "node ids descending"):
        case = BY[name]
        E0, g0, H0 = amp.reference(amp.MP, case)
        E1, g1, H1 = amp.reference(amp.MP, dict(case, x=case["x"] @ R.T + t))
        m = amp.reference(amp.MP, case, magnitudes=True)
        # (the rotation matrix and the moved coordinates are float64: relative 1e-15 on d)
        assert abs(E1 - E0) <= 1e-13 * float(m[0])
        n = len(case["x"])
        G0, G1 = np.array(g0, dtype=object).reshape(n, 3), np.array(g1, dtype=object).reshape(n, 3)
        Rm = np.array([[mpf(float(v)) for v in r] for r in R], dtype=object)
        assert max(abs(v) for v in (G1 - G0 @ Rm.T).ravel()) <= 1e-13 * float(max(m[1]))
        # translation: the gradient sums over the nodes to (sum of the coefficients) x force x t per attachment, and the float64 coefficients sum to
        # zero up to their own rounding (k |d| >= |force| for a stitch, whose gradient is k c_i d)
        per = amp.reference(amp.MP, case, parts=True)[3]
        bound = sum(abs(sum(mpf(v) for v in c)) * max(abs(f), mpf(float(k)) * l) for (ids, c), f, l, k in zip(amp.stencils(case), per[2], per[1], case["k"]))
        assert max(abs(v) for v in G0.sum(axis=0)) <= bound + mpf(10) ** -40
        for ids, c in amp.stencils(case):
            assert abs(sum(c)) <= 4 * amp.U


def test_stitch_closed_forms_and_coincident_points():
    c, xr, k, L = _one(BY["triangle point - triangle point"])
    assert L == 0
    E, g, H, l, force = amp.spring(amp.MP, c, xr, k, L)
    d = [sum(c[i] * xr[i][a] for i in range(len(c))) for a in range(3)]
    assert abs(E - k * sum(v * v for v in d) / 2) <= mpf(10) ** -45
    for i in range(len(c)):
        for a in range(3):
            assert abs(g[3 * i + a] - k * c[i] * d[a]) <= mpf(10) ** -45
            for j in range(len(c)):
                for b in range(3):
                    assert H[3 * i + a][3 * j + b] == (k * c[i] * c[j] if a == b else 0)  # B = k I
    assert abs(force - k * l) <= mpf(10) ** -45
    # d = 0: a stitch has zero energy and force and keeps its block; a tether keeps its energy k L^2 / 2 alone
    for ops in (amp.MP, amp.NP):
        E, g, H = amp.reference(ops, BY["coincident points, stitch"])
        assert E == 0 and all(v == 0 for v in g) and H[0][0] == 500 and H[0][3] == -500 and H[0][1] == 0
        E, g, H, per = amp.reference(ops, BY["coincident points with a rest length"], parts=True)
        assert abs(float(E) - 300.0 * 0.1 ** 2 / 2) <= 1e-15 and not E != E
        assert all(v == 0 for v in g) and all(v == 0 for row in H for v in row)
        assert per[1][0] == 0 and abs(float(per[2][0]) + 30.0) <= 1e-14


def test_merge_restates_the_plan():
    assert amp.stencils(BY["one node in both points"])[0] == ([0, 1, 2], [0.5, 0.25, -0.75])
    assert amp.stencils(BY["node ids descending"])[0] == ([3, 2, 0], [1.0, -0.5, -0.5])
    assert amp.merge([4, 7, -1], [0.5, 0.5, 0.0], [7, 4, -1], [0.5, 0.5, 0.0]) == ([], [])  # the same point: everything cancels
    assert [len(amp.stencils(c)[0][0]) for c in (BY["edge point - triangle point"], BY["triangle point - triangle point"])] == [5, 6]


def test_stored_cases_match_the_generator():
    stored, now = amp.load(), amp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in amp.INPUTS:
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = amp.evaluate(now[7])
    for k in amp.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[7][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in amp.load():
        n = amp.numpy_restatement(c)
        for k in amp.QUANT:
            worst = max(worst, float(np.max(amp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + amp.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= amp.NUMPY_WORST_RATIO * 1.01
    assert amp.M == 2.0 ** np.ceil(np.log2(8 * amp.NUMPY_WORST_RATIO))
