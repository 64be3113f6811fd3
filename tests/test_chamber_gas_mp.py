"""Pins tests/chamber_gas_mp.py, the mpmath restatement of the gas law: the gradient against mp.diff of W, the Hessian -gauge d2V + beta u u^T against
mp.diff of the gradient, the gamma > 1 formula tending to the gamma == 1 formula, invariance under translation and rotation, dW/dV = -gauge, the stored
golden states, and the float64 restatement's worst ratio, which sets M."""
import numpy as np
from mpmath import mp, mpf

import chamber_gas_mp as gm
import chamber_mp as cm


def small():
    x = cm.CUBE_X * 0.25 + [0.1, 0.2, 0.3] + 0.01 * (np.random.default_rng(3).random((8, 3)) - 0.5)
    r = cm.ref_point(x, cm.CUBE_TRI)
    return x, dict(tri=cm.CUBE_TRI, r=r, p=1500.0, ambient=1.0e4, gamma=1.4, V0=0.9 * cm.rest_volume(x, cm.CUBE_TRI, r))


def at(ch, x, flat):
    return gm.quantities(cm.MP, ch, [[flat[3 * i + a] for a in range(3)] for i in range(len(x))])


def test_gradient_is_the_derivative_of_the_energy_and_dW_dV_is_minus_the_gauge():
    x, ch = small()
    for gamma in (1.0, 1.4):
        ch["gamma"] = gamma
        flat = [mpf(float(v)) for v in x.ravel()]
        V, gauge, beta, W, u, g = at(ch, x, flat)
        for j in range(0, 24, 5):
            dW = mp.diff(lambda s: at(ch, x, flat[:j] + [s] + flat[j + 1:])[3], flat[j])
            dV = mp.diff(lambda s: at(ch, x, flat[:j] + [s] + flat[j + 1:])[0], flat[j])
            assert abs(dW - g[j]) <= mpf(10) ** -30 * (1 + abs(g[j])) and abs(dV - u[j]) <= mpf(10) ** -30 * (1 + abs(u[j]))
            assert abs(dW + gauge * dV) <= mpf(10) ** -30 * (1 + abs(dW))  # dW/dV = -gauge


def test_hessian_is_minus_gauge_d2V_plus_beta_u_uT():
    x, ch = small()
    flat = [mpf(float(v)) for v in x.ravel()]
    V, gauge, beta, W, u, g = at(ch, x, flat)
    # d2V/dx2: the unprojected Hessian of the constant chamber with p = -1 (W = -p V)
    d2V = cm.reference(cm.MP, dict(x=x, tri=cm.CUBE_TRI, r=ch["r"], p=-1.0), project=False)[2]
    for j in (0, 7, 13, 22):
        for i in (1, 7, 10, 23):
            H = mp.diff(lambda s: at(ch, x, flat[:j] + [s] + flat[j + 1:])[5][i], flat[j])
            assert abs(H - (-gauge * d2V[i][j] + beta * u[i] * u[j])) <= mpf(10) ** -25 * (1 + abs(H))
    assert beta > 0


def test_adiabatic_formula_tends_to_the_isothermal_one():
    x, ch = small()
    ch["gamma"] = 1.0
    W1 = gm.quantities(cm.MP, ch, x)[3]
    prev = None
    for e in (1e-3, 1e-6, 1e-9):
        ch["gamma"] = 1.0 + e
        d = abs(gm.quantities(cm.MP, ch, x)[3] - W1)
        assert d <= 10 * e * abs(W1) + mpf(10) ** -40 and (prev is None or d < prev)
        prev = d


def test_invariance_under_translation_and_rotation():
    x, ch = small()
    ca, sa, cb, sb = mp.cos(0.7), mp.sin(0.7), mp.cos(0.3), mp.sin(0.3)
    R = mp.matrix([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) * mp.matrix([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    xm = [[mpf(float(v)) for v in row] for row in x]
    q0 = gm.quantities(cm.MP, ch, xm)
    shift = [mpf(3), mpf(-2), mpf(5)]
    moved = [[row[a] + shift[a] for a in range(3)] for row in xm]
    turned = [[sum(R[a, b] * row[b] for b in range(3)) + shift[a] / 7 for a in range(3)] for row in xm]  # (the motion itself in mpmath: no rounding)
    for y in (moved, turned):
        q = gm.quantities(cm.MP, ch, y)  # (r stays: V of a closed surface does not depend on it)
        for i in range(4):
            assert abs(q[i] - q0[i]) <= mpf(10) ** -40 * abs(q0[i])
        assert abs(sum(v * v for v in q[5]) - sum(v * v for v in q0[5])) <= mpf(10) ** -40 * sum(v * v for v in q0[5])  # the gradient turns with the body


def test_stored_states_and_the_numpy_restatement():
    X, ch, off = gm.scene()
    stored = gm.load()
    assert [n for n, _, _ in stored] == list(gm.states(X, ch, off))
    worst = 0.0
    for (name, x, refs), y in zip(stored, gm.states(X, ch, off).values()):
        assert np.array_equal(x, y) and sorted(refs) == [1, 2]
        for i, ref in refs.items():
            got = gm.numpy_restatement(ch[i], x)
            for k in gm.QUANT:
                worst = max(worst, gm.ratio(np.asarray(got[k]) - np.asarray(ref[k]), ref, k))
            if name == "compressed":
                assert abs(ref["V"] / ch[i]["V0"] - 0.3) < 1e-12
    one = stored[1]
    fresh = gm.evaluate(ch[2], one[1])  # the stored numbers are what the module computes now
    assert fresh["W"] == one[2][2]["W"] and np.array_equal(fresh["g"], one[2][2]["g"])
    print(f"worst err / (sens + u scale) of the float64 restatement: {worst:.3g}")
    assert abs(worst - gm.NUMPY_WORST_RATIO) <= 5e-4 and worst < gm.M <= 2 * max(worst, 0.5)  # M: the next power of two above
