"""The mpmath restatement of the shells' rubber membrane (tests/shell_rubber_mp.py) pinned by itself: the gradient and the Hessian against mp.diff, invariance
under rigid motions, the closed form psi(l1, l2) on diagonal F, the unclamped Hessian at rest against the shell_mp StVK Hessian with nu = 1/2 and E = 3 mu,
the clamp against mp.eigsy, +infinity at collinear nodes, the Dirichlet rule; and the tolerance constant M against the recorded error of the float64
restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import shell_mp as smp
import shell_rubber_mp as rmp

BY = {c["name"]: c for c in rmp.cases()}
SMOOTH = ("rotated, alpha 0.1", "biaxial stretch 2, alpha 0.5", "uniaxial 2, lateral 1/sqrt 2, alpha 0.1", "sheared, alpha 0", "compressed to 0.3, alpha 0.1",
          "det C about 1e-6, alpha 0.1")


def _mpv(A):
    return [[mpf(float(v)) for v in r] for r in np.asarray(A)]


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


def _flat_diff(fun, x, k):
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


def _term(case, xflat, t=0, project=False, X=None):
    X = _mpv(case["X"] if X is None else X)
    return rmp.rubber(rmp.MP, X, _rows(xflat), mpf(float(case["h"][t])), mpf(float(case["YM"][t])), mpf(float(case["alpha"][t])), project=project)


@pytest.mark.parametrize("name", SMOOTH)
def test_gradient_and_hessian_against_mp_diff_and_the_clamp_against_eigsy(name):
    """the closed-form gradient is mp.diff of the energy, the unclamped closed-form Hessian mp.diff of the gradient; the clamped one is the eigenvalue clamp
    (mp.eigsy) of the differentiated matrix"""
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
    w, Q = mp.eigsy((Hd + Hd.T) / 2)
    clamped = _term(case, x, project=True)[2]
    for i in range(9):
        for j in range(9):
            want = sum(Q[i, k] * max(w[k], 0) * Q[j, k] for k in range(9))
            assert abs(clamped[i][j] - want) <= mpf(10) ** -18 * scale
    assert max(w) > 0
    if name.startswith("compressed"):
        assert min(w) < -mpf(10) ** -6 * scale  # the clamp is active


def test_det_is_the_squared_cross_product():
    """det C = C11 C22 - C12^2 = |f1 x f2|^2: the form the restatement and the kernels use is the issue's det C"""
    for c in rmp.cases()[:12]:
        X, x = _mpv(c["X"]), _mpv(c["x"])
        B, _ = smp.rest_triangle(rmp.MP, X)
        e = [smp._sub(x[1], x[0]), smp._sub(x[2], x[0])]
        f = [[e[0][i] * B[0][al] + e[1][i] * B[1][al] for i in range(3)] for al in range(2)]
        n = smp._cross(f[0], f[1])
        det = smp._dot(f[0], f[0]) * smp._dot(f[1], f[1]) - smp._dot(f[0], f[1]) ** 2
        assert abs(det - smp._dot(n, n)) <= mpf(10) ** -40 * (1 + abs(det))


def test_invariant_under_rigid_motions():
    case = BY["sheared, alpha 0.1"]
    R = _mpv(rmp.rot([3, -1, 2], 77))
    t = [mpf("0.3"), mpf("-1.2"), mpf("2.5")]
    x = _mpv(case["x"])
    xr = [[sum(R[i][j] * p[j] for j in range(3)) + t[i] for i in range(3)] for p in x]
    # (R is a float64 rotation read into mpmath: orthogonal to 1e-16 only; re-orthogonalise in mpmath)
    Q, _ = mp.qr(mp.matrix(R))
    xr = [[sum(Q[i, j] * p[j] for j in range(3)) + t[i] for i in range(3)] for p in x]
    e0, g0, H0 = _term(case, [v for r in x for v in r], project=True)
    e1, g1, H1 = _term(case, [v for r in xr for v in r], project=True)
    assert abs(e0 - e1) <= mpf(10) ** -40 * e0
    for k in range(3):  # the gradient rotates with the body
        for i in range(3):
            assert abs(g1[3 * k + i] - sum(Q[i, j] * g0[3 * k + j] for j in range(3))) <= mpf(10) ** -38 * max(abs(v) for v in g0)
    scale = max(abs(v) for row in H0 for v in row)
    for k in range(3):
        for l in range(3):
            for i in range(3):
                for j in range(3):
                    want = sum(Q[i, a] * H0[3 * k + a][3 * l + b] * Q[j, b] for a in range(3) for b in range(3))
                    assert abs(H1[3 * k + i][3 * l + j] - want) <= mpf(10) ** -30 * scale
    # translations are in the null space of the Hessian and the forces sum to zero
    for i in range(3):
        assert abs(sum(g0[3 * k + i] for k in range(3))) <= mpf(10) ** -40 * max(abs(v) for v in g0)
        for r in range(9):
            assert abs(sum(H0[r][3 * k + i] for k in range(3))) <= mpf(10) ** -30 * scale


@pytest.mark.parametrize("alpha", rmp.ALPHAS)
def test_closed_form_on_diagonal_F(alpha):
    """rest triangle scaled by (l1, l2) in its plane: W = h A psi(l1, l2); alpha = 0 is the incompressible neo-Hookean membrane"""
    h, E = mpf("0.01"), mpf(10) ** 5
    X = _mpv(rmp.P_SHEARED)
    A = smp.rest_triangle(rmp.MP, X)[1]
    for l1, l2 in ((mpf(1), mpf(1)), (mpf("1.5"), mpf("1.2")), (mpf(2), 1 / mp.sqrt(2)), (mpf("0.3"), mpf("0.3")), (mpf(4), mpf(4))):
        x = [[p[0] * l1, p[1] * l2, p[2]] for p in X]
        e = rmp.rubber(rmp.MP, X, x, h, E, mpf(alpha), hessian=False)[0]
        want = h * A * rmp.psi_principal(l1, l2, E / 3, mpf(alpha))
        assert abs(e - want) <= mpf(10) ** -40 * (1 + want)
        if alpha == 0:
            assert abs(want - h * A * E / 6 * (l1 ** 2 + l2 ** 2 + (l1 * l2) ** -2 - 3)) <= mpf(10) ** -40 * (1 + want)
    assert rmp.psi_principal(mpf(1), mpf(1), mpf(7), mpf(alpha)) == 0


@pytest.mark.parametrize("alpha", rmp.ALPHAS)
def test_unclamped_hessian_at_rest_is_the_stvk_hessian_with_nu_one_half(alpha):
    """both are the exact quadratic form of the same small-strain law (incompressible plane stress: mu = E / 3, lambda_ps = 2 mu), whatever alpha"""
    case = BY["at rest, alpha 0"]
    X = _mpv(case["X"])
    h, E = mpf("0.01"), mpf(10) ** 5
    e, g, H = rmp.rubber(rmp.MP, X, X, h, E, mpf(alpha), project=False)
    e0, g0, H0 = smp.membrane(smp.MP, X, X, h, E, mpf(1) / 2, project=False)
    scale = max(abs(v) for row in H0 for v in row)
    assert abs(e) <= mpf(10) ** -40 and max(abs(v) for v in g) <= mpf(10) ** -38 * scale
    for i in range(9):
        for j in range(9):
            assert abs(H[i][j] - H0[i][j]) <= mpf(10) ** -38 * scale


def test_collinear_nodes_give_plus_infinity_and_no_derivative():
    st = {c["name"]: c for c in rmp.load()}
    line = st["exactly collinear, alpha 0.1"]
    assert line["E"] == np.inf and not line["g"].any() and not line["H"].any() and line["sigma"][0, 1] == 0.0
    for ops in (rmp.MP, rmp.NP):
        e, g, H = rmp.patch_reference(ops, line)
        assert e == ops.inf and not e != e and all(v == 0 for v in g) and all(v == 0 for row in H for v in row)
    thin = st["det C about 1e-6, alpha 0.1"]
    assert abs((thin["sigma"][0, 0] * thin["sigma"][0, 1]) ** 2 / 1e-6 - 1) < 1e-6 and np.isfinite(thin["E"]) and thin["E"] > 0
    # float64 only: a J that underflows 1 / J^3 is degenerate too, not NaN
    tiny = rmp._case("tiny", rmp.P_SHEARED, rmp.scaled(rmp.P_SHEARED, 1.0, 1e-60))
    e, g, H = rmp.patch_reference(rmp.NP, tiny)
    assert e == np.inf and not np.any(g) and not np.any(H)


def test_special_cases():
    st = {c["name"]: c for c in rmp.load()}
    for al in rmp.ALPHAS:
        rest = st[f"at rest, alpha {al:g}"]
        assert abs(rest["E"]) <= rmp.tolerance(rest, "E") and np.all(np.abs(rest["g"]) <= rmp.tolerance(rest, "g"))
    mixed = st["StVK and rubber triangle sharing an edge"]
    assert mixed["model"].tolist() == [0, 1]
    assert not mixed["g"][6:9].any() and not mixed["H"][6:9, :].any() and mixed["g"][9:].any()  # node 2 belongs to the StVK triangle alone
    for name in ("compressed to 0.3, alpha 0", "compressed to 0.3, alpha 0.1", "compressed to 0.3, alpha 0.5"):
        raw = np.array(rmp.patch_reference(rmp.NP, dict(st[name]))[2])
        assert np.linalg.eigvalsh(st[name]["H"]).min() >= -float(np.max(rmp.tolerance(st[name], "H")))
        X = _mpv(st[name]["X"])
        un = rmp.rubber(rmp.MP, X, _mpv(st[name]["x"]), mpf(0.01), mpf(1e5), mpf(float(st[name]["alpha"][0])), project=False)[2]
        assert min(mp.eigsy(mp.matrix(un))[0]) < 0 and raw.shape == (9, 9)  # the clamp is active there
    for c in st.values():  # every stored Hessian is PSD to its tolerance
        if c["H"].any():
            assert np.linalg.eigvalsh(c["H"]).min() >= -float(np.max(rmp.tolerance(c, "H"))) - 1e-12 * np.abs(c["H"]).max(), c["name"]
    up, dn = st["strip, up triangle"], st["strip, down triangle"]
    for c in (up, dn):  # dyadic data: translating such a triangle by a multiple of the cell changes no edge vector
        assert np.array_equal(c["x"], c["X"] @ rmp.STRIP_MAP.T) and np.array_equal((c["x"] + 3 * rmp.STRIP_H * 1.5) - 3 * rmp.STRIP_H * 1.5, c["x"])


def test_dirichlet_rule_of_expected():
    c = {x["name"]: x for x in rmp.load()}["two rubber triangles, Dirichlet nodes of both types"]
    assert sorted(c["dbc"].tolist()) == [0, 0, 1, 2]
    for proj in (True, False):
        g, _ = rmp.expected(c, "g", 1.0, proj)
        H, _ = rmp.expected(c, "H", 1.0, proj)
        assert not g[0:3].any() and not H[0:3, :].any() and not H[:, 0:3].any()  # type 1: always
        assert g[6:9].any() != proj and H[6:9, 6:9].any() != proj  # type 2: with projectDBC


def test_stored_cases_match_the_generator():
    stored, now = rmp.load(), rmp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in rmp.CASE_KEYS:
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = rmp.evaluate(now[4])
    for k in rmp.QUANT + ("sigma",):
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[4][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in rmp.load():
        n = rmp.numpy_restatement(c)
        if c["E"] == np.inf:
            assert n["E"] == np.inf and not n["g"].any() and not n["H"].any()
            continue
        for k in rmp.QUANT:
            worst = max(worst, float(np.max(rmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + rmp.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= rmp.NUMPY_WORST_RATIO * 1.01
    assert rmp.M == 2.0 ** np.ceil(np.log2(8 * rmp.NUMPY_WORST_RATIO))
