"""Pins the mpmath restatement of the contact report (tests/contact_report_mp.py) on cases computable by hand.  No GPU."""
import numpy as np
from mpmath import mpf

import contact_report_mp as crm
import stencil_mp as smp

DHAT, KAPPA = 1.0e-6, 2.5e4


def _f(v):
    return np.array([float(x) for x in v])


def test_pp_pair_along_x():
    """forces +-kappa mult b'(d) 2 (a - b), torques equal and opposite"""
    X = np.array([[0.25, 0.5, -0.75], [0.25 + 6e-4, 0.5, -0.75], [9.0, 9.0, 9.0]])
    comp = np.array([1, 0, 0])  # primitive 1 lies in the higher component: side A is primitive 2
    t = dict(src="active", kind=smp.K_PP, nodes=[0, 1], mult=3, idx=7)
    r = crm.record(t, X, None, comp, DHAT, KAPPA)
    a, b = [mpf(float(c)) for c in X[0]], [mpf(float(c)) for c in X[1]]
    d = (a[0] - b[0]) ** 2
    assert abs(r["d"] - d) < mpf("1e-80")
    f0 = [-mpf(KAPPA) * 3 * smp.barrier_d1(d, mpf(DHAT)) * 2 * (a[c] - b[c]) for c in range(3)]  # the force on node 0 = primitive 1 = side B here
    assert r["key"] == (0, 1)
    assert np.allclose(_f(r["F"][1]), _f(f0), rtol=1e-25, atol=0) or np.array_equal(_f(r["F"][1]), _f(f0))
    assert max(abs(x + y) for x, y in zip(r["F"][0], r["F"][1])) < mpf("1e-30") * abs(f0[0])
    assert f0[0] < 0  # a barrier pushes node 0 (the smaller x) away from node 1
    assert max(abs(x + y) for x, y in zip(r["T"][0], r["T"][1])) < mpf("1e-30") * abs(f0[0])  # (a - b) x f = 0
    tq = crm._cross(a, f0)
    assert max(abs(x - y) for x, y in zip(r["T"][1], tq)) < mpf("1e-30") * abs(f0[0])
    rows = crm.row_table([None, r, r])
    assert len(rows) == 1 and rows[0]["counts"] == [2, 0, 0, 0, 0] and rows[0]["argmin"] == 7 and rows[0]["members"] == [1, 2]
    assert abs(rows[0]["vals"][3] - 2 * f0[0]) < mpf("1e-30") * abs(f0[0])


def test_tuple_at_or_beyond_dhat_contributes_nothing():
    X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0 ** -10]])
    t = dict(src="active", kind=smp.K_PP, nodes=[0, 1], mult=1, idx=0)
    assert crm.record(t, X, None, np.zeros(2, int), 2.0 ** -20, KAPPA) is None
    X[1, 2] = np.nextafter(X[1, 2], 0.0)
    assert crm.record(t, X, None, np.zeros(2, int), 2.0 ** -20, KAPPA) is not None


def test_half_space_vertex():
    """f = -kappa b'(dist^2) 2 dist n, torque x x f, row (component, -1 - h)"""
    n = np.array([0.0, 0.6, 0.8])
    X = np.array([[5.0, 5.0, 5.0], [0.3, -0.2, 0.4 + 5e-4 / 0.8]])
    D = -(n @ np.array([0.3, -0.2, 0.4]))
    t = dict(src="hs", kind=smp.K_PP, nodes=[1], mult=1, idx=1, h=2, n=n, D=D)
    r = crm.record(t, X, None, np.array([0, 4]), DHAT, KAPPA)
    x = [mpf(float(c)) for c in X[1]]
    dist = sum(mpf(float(n[c])) * x[c] for c in range(3)) + mpf(float(D))
    f = [-mpf(KAPPA) * smp.barrier_d1(dist ** 2, mpf(DHAT)) * 2 * dist * mpf(float(n[c])) for c in range(3)]
    assert r["key"] == (4, -3) and abs(r["d"] - dist ** 2) < mpf("1e-80")
    assert max(abs(a - b) for a, b in zip(r["F"][0], f)) < mpf("1e-30") * abs(f[2]) and f[2] > 0
    assert max(abs(a - b) for a, b in zip(r["T"][0], crm._cross(x, f))) < mpf("1e-30") * abs(f[2])
    assert all(v == 0 for v in r["F"][1] + r["T"][1])
    rows = crm.row_table([r])
    assert rows[0]["counts"] == [1, 0, 0, 0, 0] and rows[0]["argmin"] == 1 and (rows[0]["a"], rows[0]["b"]) == (4, -3)


def test_row_order():
    assert crm.row_order([(1, -1), (0, -2), (1, 1), (0, 3), (0, -1), (0, 0), (1, 2)]) == [(0, 0), (0, 3), (0, -1), (0, -2), (1, 1), (1, 2), (1, -1)]
