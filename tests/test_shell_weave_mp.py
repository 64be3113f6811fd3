"""The mpmath restatement of the shells' woven cloth (tests/shell_weave_mp.py) pinned by itself: the gradient and the Hessian against mp.diff, the clamp against
mp.eigsy, invariance under rigid motions, d against -d, the isotropic parameters against shell_mp's StVK membrane for three directions, the uniaxial closed forms
along warp, along weft and on the bias; and the tolerance constant M against the recorded error of the float64 restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import shell_mp as smp
import shell_weave_mp as wmp

BY = {c["name"]: c for c in wmp.cases()}
SMOOTH = ("rigid rotation", "stretch on the 45 degree bias", "pure shear", "compression to 0.3", "a oblique", "E1 / E2 = 100, G12 = E1 / 1000", "nu12 near its bound")


def _mpv(A):
    return [[mpf(float(v)) for v in r] for r in np.asarray(A)]


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


def _flat_diff(fun, x, k):
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


def _term(case, xflat, t=0, project=False, d=None):
    X = _mpv(case["X"][case["tri"][t]])
    d = [mpf(float(v)) for v in (case["dir"][t] if d is None else d)]
    return wmp.weave(wmp.MP, X, _rows(xflat), mpf(float(case["h"][t])), d, *[mpf(float(case[k][t])) for k in ("E1", "E2", "G12", "nu12")], project=project)


def _x(case, t=0):
    return [v for r in _mpv(case["x"][case["tri"][t]]) for v in r]


@pytest.mark.parametrize("name", SMOOTH)
def test_gradient_and_hessian_against_mp_diff_and_the_clamp_against_eigsy(name):
    """the closed-form gradient is mp.diff of the energy, the unclamped closed-form Hessian mp.diff of the gradient (this pins every factor of the header: the 2 in
    s_wf, the 4 G12 of the shear products, the 1 / 2 of dEwf/dF); the clamped one is the eigenvalue clamp (mp.eigsy) of the differentiated matrix"""
    case = BY[name]
    x = _x(case)
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
    if name.startswith("compression"):
        assert min(w) < -mpf(10) ** -6 * scale  # the clamp is active (a uniform compression to 0.3 leaves a StVK law no positive eigenvalue at all)
    else:
        assert max(w) > 0


def test_invariant_under_rigid_motions():
    case = BY["pure shear"]
    Q, _ = mp.qr(mp.matrix(_mpv(wmp.rot([3, -1, 2], 77))))  # (a float64 rotation read into mpmath is orthogonal to 1e-16 only)
    t = [mpf("0.3"), mpf("-1.2"), mpf("2.5")]
    x = _rows(_x(case))
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
    for i in range(3):  # translations are in the null space of the Hessian and the forces sum to zero
        assert abs(sum(g0[3 * k + i] for k in range(3))) <= mpf(10) ** -40 * max(abs(v) for v in g0)
        for r in range(9):
            assert abs(sum(H0[r][3 * k + i] for k in range(3))) <= mpf(10) ** -30 * scale
    # a rigid rotation of the rest state costs nothing
    rr = BY["rigid rotation"]
    e, g, _ = _term(rr, _x(rr))
    assert abs(e) <= 1e-20 and max(abs(v) for v in g) <= 1e-12  # (the stored rotation is a float64 one)


def test_d_and_minus_d_give_the_same_law():
    p, m = BY["direction d"], BY["direction -d"]
    assert np.array_equal(p["dir"], -m["dir"]) and np.array_equal(p["x"], m["x"])
    a, b = _term(p, _x(p), project=True), _term(m, _x(m), project=True)
    assert a[0] == b[0] and all(u == v for u, v in zip(a[1], b[1]))
    scale = max(abs(v) for row in a[2] for v in row)
    assert all(abs(u - v) <= mpf(10) ** -40 * scale for ra, rb in zip(a[2], b[2]) for u, v in zip(ra, rb))
    sp, sm = wmp.load()[[c["name"] for c in wmp.cases()].index("direction d")], wmp.load()[[c["name"] for c in wmp.cases()].index("direction -d")]
    assert np.array_equal(sp["S"][:, :3], sm["S"][:, :3]) and np.array_equal(sp["S"][:, 3:], -sm["S"][:, 3:])  # the warp direction turns round, nothing else


@pytest.mark.parametrize("d", [(1.0, 0.0, 0.0), (0.3, -1.0, 0.4), (-0.2, 0.5, 0.9)])
def test_isotropic_parameters_reproduce_the_stvk_membrane(d):
    """E1 = E2 = E, nu12 = nu, G12 = E / (2 (1 + nu)): energy, gradient and unclamped Hessian of shell_mp's StVK membrane to 1e-25 relative, whatever the direction"""
    case = BY["tilted rest triangle, rotated and stretched"]
    X, x = _mpv(case["X"]), _mpv(case["x"])
    h, E, nu = mpf("0.01"), mpf(10) ** 5, mpf("0.3")
    e, g, H = wmp.weave(wmp.MP, X, x, h, [mpf(v) for v in d], E, E, E / (2 * (1 + nu)), nu, project=False)
    e0, g0, H0 = smp.membrane(smp.MP, X, x, h, E, nu, project=False)
    rel = mpf(10) ** -25
    assert abs(e - e0) <= rel * abs(e0)
    assert all(abs(u - v) <= rel * max(abs(w) for w in g0) for u, v in zip(g, g0))
    scale = max(abs(v) for row in H0 for v in row)
    assert all(abs(u - v) <= rel * scale for ra, rb in zip(H, H0) for u, v in zip(ra, rb))


def _uniaxial(angle, Eaxial):
    """a square sheet under uniaxial second Piola-Kirchhoff stress along the in-plane direction at `angle` to the warp: the strain from the compliance of the law
    (1 / E1, -nu12 / E1, 1 / E2, 1 / G12), realised as x = U X with U = sqrt(I + 2 G); returns (Eww, Eff, Ewf, psi, strain along the pull, stress)"""
    E1, E2, G12, nu12 = mpf(10) ** 5, mpf(5) * 10 ** 4, mpf(2000), mpf("0.25")
    sigma = mpf(300)
    c, s = mp.cos(angle), mp.sin(angle)
    sww, sff, swf = sigma * c * c, sigma * s * s, sigma * c * s  # the stress in yarn axes
    Eww, Eff, Ewf = sww / E1 - nu12 * sff / E1, sff / E2 - nu12 * sww / E1, swf / (2 * G12)
    G = mp.matrix([[Eww, Ewf], [Ewf, Eff]])  # warp along x
    Um = mp.sqrtm(mp.eye(2) + 2 * G)
    X = [[mpf(0), mpf(0), mpf(0)], [mpf(1), mpf(0), mpf(0)], [mpf("0.3"), mpf("0.8"), mpf(0)]]
    x = [[Um[0, 0] * p[0] + Um[0, 1] * p[1], Um[1, 0] * p[0] + Um[1, 1] * p[1], mpf(0)] for p in X]
    h = mpf("0.01")
    A = smp.rest_triangle(wmp.MP, X)[1]
    W = wmp.weave(wmp.MP, X, x, h, [mpf(1), mpf(0), mpf(0)], E1, E2, G12, nu12, hessian=False)[0]
    st = wmp.state(wmp.MP, X, x, [mpf(1), mpf(0), mpf(0)])
    assert abs(st[0] - Eww) <= mpf(10) ** -40 and abs(st[1] - Eff) <= mpf(10) ** -40
    C = wmp.moduli(E1, E2, G12, nu12)  # the stress of the law at this strain is the uniaxial one: stiffness and compliance are inverse to each other
    for got, want in ((C[0] * Eww + C[1] * Eff, sww), (C[1] * Eww + C[2] * Eff, sff), (2 * C[3] * Ewf, swf)):
        assert abs(got - want) <= mpf(10) ** -40 * sigma
    Epull = c * c * Eww + s * s * Eff + 2 * c * s * Ewf
    return Eww, Eff, Ewf, W / (h * A), Epull, sigma, (E1, E2, G12, nu12)


def test_uniaxial_stress_along_warp_weft_and_bias():
    Eww, Eff, Ewf, psi, Ep, sigma, (E1, E2, G12, nu12) = _uniaxial(mpf(0), None)
    assert abs(Eff + nu12 * Eww) <= mpf(10) ** -40 and abs(psi - E1 * Eww ** 2 / 2) <= mpf(10) ** -38 * psi and Ewf == 0
    Eww, Eff, Ewf, psi, Ep, sigma, _ = _uniaxial(mp.pi / 2, None)
    nu21 = nu12 * E2 / E1
    assert abs(Eww + nu21 * Eff) <= mpf(10) ** -40 and abs(psi - E2 * Eff ** 2 / 2) <= mpf(10) ** -38 * psi
    Eww, Eff, Ewf, psi, Ep, sigma, _ = _uniaxial(mp.pi / 4, None)
    inv_E45 = (1 / E1 + 1 / E2 - 2 * nu12 / E1 + 1 / G12) / 4
    assert abs(Ep / sigma - inv_E45) <= mpf(10) ** -40 * inv_E45
    assert abs(psi - sigma * Ep / 2) <= mpf(10) ** -38 * psi  # the strain energy of a linear law in G
    assert 1 / inv_E45 < E2 / 5  # the bias is soft: G12 rules it


def test_positive_definite_iff_the_bound_holds():
    for nu, ok in ((mpf("1.4"), True), (mpf("1.42"), False)):  # E1 / E2 = 2: the bound is sqrt 2
        C = wmp.moduli(mpf(10) ** 5, mpf(5) * 10 ** 4, mpf(2000), nu)
        assert (C[0] > 0 and C[0] * C[2] - C[1] ** 2 > 0) == ok


def test_special_cases():
    st = {c["name"]: c for c in wmp.load()}
    rest = st["rest state"]
    assert abs(rest["E"]) <= wmp.tolerance(rest, "E") and np.all(np.abs(rest["g"]) <= wmp.tolerance(rest, "g"))
    assert np.all(np.abs(rest["S"][0, :3]) <= wmp.tolerance(rest, "S")[0, :3])
    mixed = st["StVK and woven triangle sharing an edge"]
    assert mixed["woven"].tolist() == [0, 1] and not mixed["S"][0].any() and mixed["S"][1].any()
    assert not mixed["g"][6:9].any() and not mixed["H"][6:9, :].any() and mixed["g"][9:].any()  # node 2 belongs to the StVK triangle alone
    warp, weft, bias = st["stretch along warp"], st["stretch along weft"], st["stretch on the 45 degree bias"]
    assert abs(warp["S"][0, 0] - 0.22) < 1e-12 and abs(warp["S"][0, 1]) < 1e-12 and abs(weft["S"][0, 1] - 0.22) < 1e-12 and abs(weft["S"][0, 0]) < 1e-12
    assert warp["E"] > weft["E"] > bias["E"] > 0 and abs(bias["S"][0, 2]) > 0.1  # E1 > E2; the bias shears the yarns
    comp = st["compression to 0.3"]
    X = _mpv(comp["X"])
    un = _term(comp, _x(comp))[2]
    assert min(mp.eigsy(mp.matrix(un))[0]) < 0  # the clamp is active there
    for c in st.values():  # every stored Hessian is PSD to its tolerance
        assert np.linalg.eigvalsh(c["H"]).min() >= -float(np.max(wmp.tolerance(c, "H"))) - 1e-12 * np.abs(c["H"]).max(), c["name"]
    thin = st["aspect-1000 triangle"]
    l = np.linalg.norm(thin["X"][1] - thin["X"][0])
    assert l / (2 * 0.5 * 0.001 * 1.0 / l) >= 1000 and np.isfinite(thin["E"]) and thin["E"] > 0
    al, pe = st["a along local axis 1"], st["a perpendicular to local axis 1"]
    for c, want in ((al, [1.0, 0.0]), (pe, [0.0, 1.0])):
        a = wmp.warp_in_plane(wmp.NP, c["X"].tolist(), c["dir"][0].tolist())
        assert np.allclose(a, want, atol=1e-15)
    up = st["strip, up triangle"]  # dyadic data: translating such a triangle by a multiple of the cell changes no edge vector
    assert np.array_equal(up["x"], up["X"] @ wmp.STRIP_MAP.T) and np.array_equal((up["x"] + 3 * wmp.STRIP_H * 1.5) - 3 * wmp.STRIP_H * 1.5, up["x"])


def test_dirichlet_rule_of_expected():
    c = {x["name"]: x for x in wmp.load()}["two woven triangles, Dirichlet nodes of type ZERO and NONZERO"]
    assert sorted(c["dbc"].tolist()) == [0, 0, 1, 2]
    for proj in (True, False):
        g, _ = wmp.expected(c, "g", 1.0, proj)
        H, _ = wmp.expected(c, "H", 1.0, proj)
        assert not g[0:3].any() and not H[0:3, :].any() and not H[:, 0:3].any()  # type 1: always
        assert g[6:9].any() != proj and H[6:9, 6:9].any() != proj  # type 2: with projectDBC


def test_stored_cases_match_the_generator():
    stored, now = wmp.load(), wmp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in wmp.CASE_KEYS:
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = wmp.evaluate(now[4])
    for k in wmp.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[4][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in wmp.load():
        n = wmp.numpy_restatement(c)
        for k in wmp.QUANT:
            worst = max(worst, float(np.max(wmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + wmp.U * np.asarray(c["scale_" + k])))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= wmp.NUMPY_WORST_RATIO * 1.01
    assert wmp.M == 2.0 ** np.ceil(np.log2(8 * wmp.NUMPY_WORST_RATIO))
