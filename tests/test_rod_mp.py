"""The mpmath restatement of the rod energies (tests/rod_mp.py) pinned by itself: derivatives against mp.diff, the closed-form clamp against mp.eigsy,
rigid motions, hand-placed angles, the continuum limit of a curved polyline, the fold, a hanging rod in closed form; and the tolerance constant M against
the recorded error of the float64 restatement over the stored cases.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import rod_mp as rmp

R0, R1, YM = mpf("0.002"), mpf("0.003"), mpf(1e7)


def _mpv(A):
    return [[mpf(float(v)) for v in r] for r in np.asarray(A)]


def _flat_diff(fun, x, k):
    """d fun / d (coordinate k) at the flattened point x (list of mpf)"""
    return mp.diff(lambda t: fun(x[:k] + [t] + x[k + 1:]), x[k])


def _rows(flat):
    return [flat[3 * i:3 * i + 3] for i in range(len(flat) // 3)]


SEG_CASES = [c for c in rmp.cases() if len(c["seg"]) == 1]
ELBOW_CASES = [c for c in rmp.cases() if c["name"].startswith("three nodes")]


@pytest.mark.parametrize("case", SEG_CASES[1:], ids=lambda c: c["name"])
def test_stretch_gradient_and_clamped_hessian_against_mp_diff_and_eigsy(case):
    """the gradient against mp.diff; the closed-form clamp against mp.eigsy of the mp.diff Hessian with its eigenvalues clamped at 0; the spectrum of the
    full Hessian is 2 k_s, 2 k_s (1 - L / l) twice, 0 three times"""
    X, x = _mpv(case["X"]), [v for r in _mpv(case["x"]) for v in r]
    E = lambda f: rmp.stretch(rmp.MP, X, _rows(f), R0, YM)[0]
    _, g, Hc = rmp.stretch(rmp.MP, X, _rows(x), R0, YM)
    Hd = mp.matrix(6, 6)
    for k in range(6):
        assert abs(_flat_diff(E, x, k) - g[k]) <= mpf(10) ** -30 * (1 + abs(g[k]))
        for l in range(6):
            Hd[k, l] = _flat_diff(lambda f: rmp.stretch(rmp.MP, X, _rows(f), R0, YM)[1][k], x, l)
    Hd = (Hd + Hd.T) / 2
    full = rmp.stretch(rmp.MP, X, _rows(x), R0, YM, project=False)[2]
    w, Q = mp.eigsy(Hd)
    L, l = rmp.rest_length(rmp.MP, *X), rmp.rest_length(rmp.MP, *_rows(x))
    ks = YM * mp.pi * R0 * R0 / L
    want = sorted([2 * ks, 2 * ks * (1 - L / l), 2 * ks * (1 - L / l), 0, 0, 0])
    for a, b in zip(sorted(w), want):
        assert abs(a - b) <= mpf(10) ** -25 * ks
    for k in range(6):
        for l_ in range(6):
            clamped = sum(Q[k, m] * (w[m] if w[m] > 0 else 0) * Q[l_, m] for m in range(6))
            assert abs(full[k][l_] - Hd[k, l_]) <= mpf(10) ** -25 * ks
            assert abs(Hc[k][l_] - clamped) <= mpf(10) ** -25 * ks
    compressed = l < L * (1 - mpf(10) ** -3)  # (the rotated segment is shorter by a float64 rounding of its rotation: not compressed)
    assert (min(w) < -mpf(10) ** -3 * ks) == compressed  # the clamp acts exactly on the compressed segment


@pytest.mark.parametrize("case", ELBOW_CASES[1:] + [dict(ELBOW_CASES[1], name="three nodes at 30", x=rmp.elbow(30, 0.09, 0.2))], ids=lambda c: c["name"])
def test_bend_gradient_and_jacobian_against_mp_diff(case):
    X, x = _mpv(case["X"]), [v for r in _mpv(case["x"]) for v in r]
    mat = ((R0, YM), (R1, 3 * YM))
    E = lambda f: rmp.bend(rmp.MP, X, _rows(f), mat, mpf(2))[0]
    e, g, Hg = rmp.bend(rmp.MP, X, _rows(x), mat, mpf(2))
    k2, kb, J = rmp.curvature(rmp.MP, _rows(x), True)
    k = 2 * rmp.bend_stiffness(rmp.MP, X, mat)
    assert abs(k2 - rmp._dot(kb, kb)) <= mpf(10) ** -40 * (1 + k2)  # 4 (p - q) / d = |2 e0 x e1 / d|^2
    for c in range(9):
        assert abs(_flat_diff(E, x, c) - g[c]) <= mpf(10) ** -30 * (1 + abs(g[c]))
        for m in range(3):
            d = _flat_diff(lambda f: rmp.curvature(rmp.MP, _rows(f))[1][m], x, c)
            assert abs(d - J[m][c]) <= mpf(10) ** -30 * (1 + abs(J[m][c]))
        for b in range(9):
            assert abs(Hg[c][b] - 2 * k * sum(J[m][c] * J[m][b] for m in range(3))) <= mpf(10) ** -40 * (1 + abs(Hg[c][b]))  # Gauss-Newton: rank <= 3
    H = np.array(Hg, dtype=object).astype(np.float64)
    assert np.linalg.matrix_rank(H, tol=1e-9 * np.abs(H).max()) <= 3 and np.linalg.eigvalsh(H).min() >= -1e-12 * np.abs(H).max()


def test_zero_energy_and_gradient_at_rest_and_under_rigid_motion_of_a_straight_rod():
    R, t = rmp.rot([2, -1, 3], 73.0), np.array([0.3, -0.2, 0.5])
    V, seg = rmp.chain(5, axis=(0.6, 0.0, 0.8))
    c = rmp._case("straight", V, V, seg, r=[0.002, 0.002, 0.003, 0.003])
    for x in (V, V @ R.T + t):
        E, g, _ = rmp.chain_reference(rmp.MP, dict(c, x=x))
        m = rmp.chain_reference(rmp.MP, dict(c, x=x), magnitudes=True)
        assert 0 <= float(E) <= 1e-28 * float(m[0])  # (the rotation matrix is float64: |R^T R - I| ~ 1e-16, squared in the energy)
        assert max(abs(float(v)) for v in g) <= 1e-13 * float(max(m[1]))


def test_curvature_is_two_tan_half_theta_at_hand_placed_angles():
    for deg in (0, 60, 90, 170):
        t = mp.radians(deg)
        x = [[mpf(-1), mpf(0), mpf(0)], [mpf(0)] * 3, [2 * mp.cos(t), 2 * mp.sin(t), mpf(0)]]  # turning angle deg at the middle node, lengths 1 and 2
        k2, kb, _ = rmp.curvature(rmp.MP, x)
        want = 2 * mp.tan(t / 2)
        assert abs(mp.sqrt(k2) - want) <= mpf(10) ** -40 * (1 + want)
        assert abs(kb[2] - want) <= mpf(10) ** -40 * (1 + want) and kb[0] == 0 and kb[1] == 0  # the binormal: +z for a left turn in the plane z = 0
    # 90 degrees by hand: e0 = (1, 0, 0), e1 = (0, 1, 0): kb = 2 (0, 0, 1) / (1 + 0)
    assert rmp.curvature(rmp.MP, _mpv([[0, 0, 0], [1, 0, 0], [1, 1, 0]]))[1] == [0, 0, 2]


def test_uniformly_curved_polyline_tends_to_the_continuum_bending_energy():
    """n nodes on a circle of radius R: sum W_b = (1/2) E I (2 pi R) / R^2 / cos^2(pi / n) (by hand: |kb| = 2 tan(phi / 2), L = 2 R sin(phi / 2), phi = 2 pi / n):
    the relative excess over the continuum value is tan^2(pi / n) -- second order, a quarter of it per doubling of n"""
    Rr, r, E = 0.5, 0.002, 1e7
    excess = []
    for n in (24, 48, 96):  # (tan^2(h) / tan^2(h / 2) = 4 / (1 - tan^2(h / 2))^2: 4.035 and 4.009 here)
        V, seg = rmp.ring(n, Rr)
        c = rmp._case("ring", V, V, seg, r=r, YM=E)
        _, _, _, per = rmp.chain_reference(rmp.MP, c, parts=True)
        L = rmp.rest_length(rmp.MP, *_mpv(V[:2]))
        cont = mpf(E) * mp.pi * mpf(r) ** 4 / 4 * (n * L) / mpf(Rr) ** 2 / 2
        excess.append(float(sum(per[1]) / cont - 1))
        assert abs(excess[-1] - float(mp.tan(mp.pi / n) ** 2)) <= 1e-12
        assert len(per[1]) == n  # every node of a ring is interior
    assert 3.9 < excess[0] / excess[1] < 4.1 and 3.9 < excess[1] / excess[2] < 4.1


def test_exact_fold_is_plus_infinity_not_nan():
    x = [[0.25, 0.5, 0.0], [0.5, 0.5, 0.125], [0.25, 0.5, 0.0]]  # x_c = x_a
    X = [[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0]]
    for ops in (rmp.MP, rmp.NP):
        e = rmp.bend(ops, [[ops.num(v) for v in r] for r in X], [[ops.num(v) for v in r] for r in x], ((0.002, 1e7), (0.002, 1e7)), 1.0)[0]
        assert e == ops.inf and not e != e
    c = rmp._case("fold", X, x, [[0, 1], [1, 2]])
    assert float(rmp.chain_reference(rmp.NP, c)[0]) == np.inf


def test_hanging_rod_at_its_discrete_equilibrium_carries_the_weights_below():
    """nodes 0 .. n down a vertical line, node 0 held: segment i (between nodes i and i + 1) carries T_i = g x (the mass of the nodes below it) at
    l_i = L (1 + T_i / (E A)), and then dW / dy_j = -m_j g for every free node (force balance with gravity (0, -g, 0)); bending adds nothing: it is straight"""
    n, L, r, E, rho, G = 6, mpf("0.1"), mpf("0.002"), mpf(1e6), mpf(1000), mpf("9.80665")
    A = mp.pi * r * r
    mass = [rho * A * L / 2 * (1 if j in (0, n) else 2) for j in range(n + 1)]
    T = [G * sum(mass[i + 1:]) for i in range(n)]
    y = [mpf(0)]
    for i in range(n):
        y.append(y[-1] - L * (1 + T[i] / (E * A)))
    X = [[mpf(0), -j * L, mpf(0)] for j in range(n + 1)]
    x = [[mpf(0), y[j], mpf(0)] for j in range(n + 1)]
    seg = [[j, j + 1] for j in range(n)]
    g = [mpf(0)] * (3 * (n + 1))
    for s, (a, b) in enumerate(seg):
        _, ge, _ = rmp.stretch(rmp.MP, [X[a], X[b]], [x[a], x[b]], r, E)
        for p, P in enumerate([3 * a, 3 * a + 1, 3 * a + 2, 3 * b, 3 * b + 1, 3 * b + 2]):
            g[P] += ge[p]
    for b in range(1, n):
        _, gb, _ = rmp.bend(rmp.MP, [X[b - 1], X[b], X[b + 1]], [x[b - 1], x[b], x[b + 1]], ((r, E), (r, E)), mpf(1))
        assert all(v == 0 for v in gb)
    for j in range(1, n + 1):
        assert abs(g[3 * j + 1] + mass[j] * G) <= mpf(10) ** -40 * mass[j] * G and g[3 * j] == 0 and g[3 * j + 2] == 0
    assert abs(g[1] - sum(mass[1:]) * G) <= mpf(10) ** -40  # the support carries everything below it


def test_triples_skip_ends_and_junctions():
    by = {c["name"]: c for c in rmp.cases()}
    j = by["three-armed junction"]
    assert [t[:3] for t in rmp.triples_of(j["seg"], len(j["X"]))] == [(0, 1, 4)]  # the hub (node 0, three segments) does not bend
    r = by["closed six-node ring"]
    assert [t[1] for t in rmp.triples_of(r["seg"], 6)] == list(range(6))
    p = by["five-node polyline, Dirichlet nodes"]
    assert [t[:3] for t in rmp.triples_of(p["seg"], 5)] == [(0, 1, 2), (1, 2, 3), (2, 3, 4)] and sorted(p["dbc"].tolist()) == [0, 0, 0, 1, 2]


def test_stored_cases_match_the_generator():
    stored, now = rmp.load(), rmp.cases()
    assert [c["name"] for c in stored] == [c["name"] for c in now]
    for s, c in zip(stored, now):
        for k in ("X", "x", "seg", "r", "YM", "rho", "dbc"):
            assert np.array_equal(s[k], c[k]), (c["name"], k)
    r = rmp.evaluate(now[5])
    for k in rmp.QUANT:
        assert np.array_equal(np.asarray(r[k]), np.asarray(stored[5][k]))


def test_numpy_restatement_meets_the_tolerance():
    worst = 0.0
    for c in rmp.load():
        n = rmp.numpy_restatement(c)
        for k in rmp.QUANT:
            worst = max(worst, float(np.max(np.abs(n[k] - c[k]) / (np.asarray(c["sens_" + k]) + rmp.U * c["scale_" + k]))))
    print("worst ratio of the float64 restatement:", worst)
    assert worst <= rmp.NUMPY_WORST_RATIO * 1.01
    assert rmp.M == 2.0 ** np.ceil(np.log2(8 * rmp.NUMPY_WORST_RATIO))
