"""The mpmath restatement of the shells' strain limit (tests/shell_limit_mp.py) pinned by itself: the gradient and the Hessian against mp.diff, the
closed-form eigenvalues against mp.eigsy (all >= 0), C^2 continuity at the onset, the special cases (below the onset, over the limit, a collapsed triangle,
equal stretches), the Dirichlet rule; and the tolerance constant M against the recorded error of the float64 restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import shell_limit_mp as lmp

H_, E_ = mpf(0.01), mpf(1e5)  # (the float64 values of the cases)
BY = {c["name"]: c for c in lmp.cases()}
SMOOTH = ("one stretch active", "both stretches active", "stretches 1e-9 apart", "stretch 1e-6 of the range below the limit", "triangle collapsed to a line",
          "sheared and rotated rest triangle", "stiff 2.5, onset 1.05")


def _mpv(A):
    return [[mpf(float(v)) for v in r] for r in np.asarray(A)]


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


def _flat_diff(fun, x, k):
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


def _term(case, xflat, t=0):
    X = _mpv(case["X"])
    return lmp.limit_term(lmp.MP, X, _rows(xflat), mpf(float(case["h"][t])), mpf(float(case["YM"][t])), mpf(float(case["onset"][t])),
                          mpf(float(case["limit"][t])), mpf(float(case["stiff"][t])))


@pytest.mark.parametrize("name", SMOOTH)
def test_gradient_and_hessian_against_mp_diff_and_eigenvalues_against_eigsy(name):
    """single-triangle cases away from the onset: the closed-form gradient is mp.diff of the energy, the closed-form Hessian mp.diff of the gradient, and its
    eigenvalues (mp.eigsy) are >= 0 up to the tolerance of the case"""
    case = BY[name]
    x = [v for r in _mpv(case["x"]) for v in r]
    e, g, Hc = _term(case, x)
    scale = max(abs(v) for row in Hc for v in row)
    Hd = mp.matrix(9, 9)
    for k in range(9):
        assert abs(_flat_diff(lambda f: _term(case, f)[0], x, k) - g[k]) <= mpf(10) ** -25 * (1 + max(abs(v) for v in g))
        for l in range(9):
            Hd[k, l] = _flat_diff(lambda f: _term(case, f)[1][k], x, l)
    for k in range(9):
        for l in range(9):
            assert abs(Hd[k, l] - Hc[k][l]) <= mpf(10) ** -20 * scale, (name, k, l)
    w, _ = mp.eigsy((Hd + Hd.T) / 2)
    tol = float(np.max(lmp.tolerance(lmp.evaluate(case), "H")))
    assert min(w) >= -tol, (name, min(w))
    assert max(w) > 0


def test_hessian_in_F_has_the_stated_eigenpairs():
    """rest triangle (0, 0), (1, 0), (0, 1): Dm = I, so the rows and columns of nodes 1 and 2 ARE the 6 x 6 Hessian in F; its spectrum (mp.eigsy) is
    k { b''1, b''2, (b'1 + b'2) / (s1 + s2), (b'1 - b'2) / (s1 - s2), b'1 / s1, b'2 / s2 }"""
    on, lim = mpf(1), mpf(1.2)  # (the float64 1.2 of the case)
    a, b = mpf("1.15"), mpf("1.05")
    R = lmp.rot([1, 2, 3], 50)
    xr = (lmp.P_RIGHT * [float(a), float(b), 1.0]) @ R.T
    case = lmp._case("F", lmp.P_RIGHT, xr)
    x = [v for r in _mpv(xr) for v in r]
    _, _, Hc = _term(case, x)
    s1, s2, m = lmp.stretches(lmp.MP, _mpv(lmp.P_RIGHT), _rows(x))
    k = H_ * m["A"] * E_
    b1, b2 = lmp.barrier(lmp.MP, s1, on, lim), lmp.barrier(lmp.MP, s2, on, lim)
    want = sorted(k * v for v in (b1[2], b2[2], (b1[1] + b2[1]) / (s1 + s2), (b1[1] - b2[1]) / (s1 - s2), b1[1] / s1, b2[1] / s2))
    w, _ = mp.eigsy(mp.matrix([[Hc[i][j] for j in range(3, 9)] for i in range(3, 9)]))
    for got, ref in zip(sorted(w), want):
        assert abs(got - ref) <= mpf(10) ** -30 * want[-1]
    assert want[0] > 0
    # the barrier's derivatives themselves against mp.diff
    for s in (s1, s2):
        bb = lambda t: lmp.barrier(lmp.MP, t, on, lim)[0]
        got = lmp.barrier(lmp.MP, s, on, lim)
        assert abs(mp.diff(bb, s) - got[1]) <= mpf(10) ** -30 * got[1] and abs(mp.diff(bb, s, 2) - got[2]) <= mpf(10) ** -25 * got[2]


def test_divided_difference_tends_to_the_second_derivative():
    """(b'1 - b'2) / (s1 - s2) in the cancellation-free form: the plain quotient at 50 digits for stretches 1e-9 apart, b'' for equal ones"""
    case = BY["stretches 1e-9 apart"]
    X, x = _mpv(case["X"]), _mpv(case["x"])
    s1, s2, m = lmp.stretches(lmp.MP, X, x)
    assert mpf(10) ** -10 < s1 - s2 < mpf(10) ** -8
    on, lim = mpf(1), mpf(float(case["limit"][0]))
    b1, b2 = lmp.barrier(lmp.MP, s1, on, lim), lmp.barrier(lmp.MP, s2, on, lim)
    plain = (b1[1] - b2[1]) / (s1 - s2)
    y1, z1, L1, y2, z2, L2 = b1[3], b1[4], b1[5], b2[3], b2[4], b2[5]
    q = (y1 - y2) / z2
    closed = ((y1 + y2 - y1 * y2) / (z1 * z2) - 2 * (L1 + y2 * mp.log1p(-q) / q / z2)) / (lim - on) ** 2
    assert abs(plain - closed) <= mpf(10) ** -35 * plain
    assert abs(plain - b1[2]) <= mpf(10) ** -7 * plain
    # equal stretches exactly: the flip eigenvalue is b'', the whole in-plane block isotropic; float64 agrees with mpmath to rounding there
    eq = lmp.load()[[c["name"] for c in lmp.cases()].index("equal stretches exactly")]
    n = lmp.numpy_restatement(eq)
    assert np.array_equal(n["g"], eq["g"]) and np.array_equal(n["H"], eq["H"])  # (dyadic data: every operation of the restatement is exact but ln)


def test_c2_at_the_onset():
    """b, b' and b'' are exactly 0 at the onset and from below, and tend to 0 from above like eps^3, 3 eps^2, 6 eps (in units of the range)"""
    on, lim = mpf("1.05"), mpf("1.3")
    w = lim - on
    for s in (on, on - mpf(10) ** -30, mpf("0.5")):
        assert lmp.barrier(lmp.MP, s, on, lim)[:3] == (0, 0, 0)
    for p in (6, 12, 24):
        eps = mpf(10) ** -p
        b, d1, d2 = lmp.barrier(lmp.MP, on + eps * w, on, lim)[:3]
        assert abs(b / eps ** 3 - 1) <= 2 * eps and abs(d1 * w / (3 * eps ** 2) - 1) <= 2 * eps and abs(d2 * w * w / (6 * eps) - 1) <= 2 * eps
    # and through a whole triangle: energy, gradient and Hessian are continuous across the onset
    lo = lmp._case("lo", lmp.P_SHEARED, lmp.scaled(lmp.P_SHEARED, 1.0 - 1e-12, 0.9))
    hi = lmp._case("hi", lmp.P_SHEARED, lmp.scaled(lmp.P_SHEARED, 1.0 + 1e-12, 0.9))
    rl, rh = lmp.patch_reference(lmp.MP, lo), lmp.patch_reference(lmp.MP, hi)
    k = float(H_ * E_ * mpf("0.4"))
    assert rl[0] == 0 and all(v == 0 for v in rl[1]) and all(v == 0 for row in rl[2] for v in row)
    assert 0 < rh[0] < k * 1e-30 and max(abs(v) for v in rh[1]) < k * 1e-20 and max(abs(v) for row in rh[2] for v in row) < k * 1e-8


def test_special_cases():
    st = {c["name"]: c for c in lmp.load()}
    below = st["both stretches below the onset"]
    assert below["E"] == 0.0 and not below["g"].any() and not below["H"].any() and below["scale_H"] == 0.0
    over = st["stretch over the limit"]
    assert over["E"] == np.inf and not over["g"].any() and not over["H"].any()
    for ops in (lmp.MP, lmp.NP):
        e = lmp.patch_reference(ops, over)[0]
        assert e == ops.inf and not e != e
    line = st["triangle collapsed to a line"]
    assert line["sigma"][0, 1] == 0.0 and 1.0 < line["sigma"][0, 0] < 1.2 and np.all(np.isfinite(line["H"])) and line["E"] > 0
    n = lmp.numpy_restatement(line)
    assert np.all(np.isfinite(n["g"])) and np.all(np.isfinite(n["H"]))
    mixed = st["limited and unlimited triangle sharing an edge"]
    assert not mixed["g"][9:].any() and not mixed["H"][9:, :].any() and mixed["g"][:9].any()  # node 3 belongs to the unlimited triangle alone
    eq = st["equal stretches exactly"]
    assert eq["sigma"][0, 0] == eq["sigma"][0, 1] == 1.125
    near = st["stretch 1e-6 of the range below the limit"]
    assert abs((1.2 - near["sigma"][0, 0]) / 0.2 / 1e-6 - 1) < 1e-6
    for c in st.values():  # every stored Hessian is PSD to its tolerance
        if c["H"].any():
            assert np.linalg.eigvalsh(c["H"]).min() >= -float(np.max(lmp.tolerance(c, "H"))) - 1e-12 * np.abs(c["H"]).max(), c["name"]


def test_dirichlet_rule_of_expected():
    c = {x["name"]: x for x in lmp.load()}["two triangles, Dirichlet nodes of both types"]
    assert sorted(c["dbc"].tolist()) == [0, 0, 1, 2]
    for proj in (True, False):
        g, _ = lmp.expected(c, "g", 1.0, proj)
        H, _ = lmp.expected(c, "H", 1.0, proj)
        assert not g[0:3].any() and not H[0:3, :].any() and not H[:, 0:3].any()  # type 1: always
        assert g[6:9].any() != proj and H[6:9, 6:9].any() != proj  # type 2: with projectDBC


def test_stored_cases_match_the_generator():
    stored, now = lmp.load(), lmp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in lmp.CASE_KEYS:
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = lmp.evaluate(now[2])
    for k in lmp.QUANT + ("sigma",):
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[2][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in lmp.load():
        n = lmp.numpy_restatement(c)
        if c["E"] == np.inf:
            assert n["E"] == np.inf and not n["g"].any() and not n["H"].any()
            continue
        for k in lmp.QUANT:
            worst = max(worst, float(np.max(lmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + lmp.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= lmp.NUMPY_WORST_RATIO * 1.01
    assert lmp.M == 2.0 ** np.ceil(np.log2(8 * lmp.NUMPY_WORST_RATIO))
