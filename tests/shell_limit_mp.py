"""mpmath restatement of the strain limit of the elastic shells (ipc_amd/csrc/shell_limit_kernels.h): the log barrier on the principal stretches, its
gradient and its Hessian; a project extension, so there is no oracle to compare with -- this file is the reference, pinned by tests/test_shell_limit_mp.py
(mp.diff, mp.eigsy, continuity at the onset).

Per limited triangle (limit s, onset sHat, stiffness stiff, thickness h, rest area A, Young's modulus E):  F = [x1 - x0, x2 - x0] Dm^-1 as the membrane's
(shell_mp.rest_triangle), C = F^T F, m = (C11 + C22) / 2, d = (C11 - C22) / 2, r = sqrt(d^2 + C12^2), sigma1 = sqrt(m + r), sigma2 = |f1 x f2| / sigma1.
  W = stiff h A E (b(sigma1) + b(sigma2)),  b = 0 up to sHat,  -y^2 ln(1 - y) with y = (sigma - sHat) / (s - sHat) below s,  +infinity from s on.
Gradient k sum b'(sigma_i) u_i v_i^T; Hessian by its eigenpairs (b'' on u_i v_i^T, (b'1 + b'2) / (sigma1 + sigma2) on the twist, (b'1 - b'2) / (sigma1 - sigma2)
on the flip, b'_i / sigma_i on u3 v_i^T), each clamped at 0.  A triangle at or over its limit: energy +infinity, gradient and Hessian zero.

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64): the float64 instance is the "NumPy restatement"
whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/shell_mp.py, rod_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every rest and current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  every term of the barrier's formulas is non-negative already (y, z, -ln z, b, b', b''): per triangle k (b1 + b2) for the energy,
         k (b'1 + b'2) G for the gradient and k (b''1 + b''2 + twist + flip + b'1 / sigma1 + b'2 / sigma2) G^2 for the Hessian, G the largest 1-norm of a row
         of the node weights (Dm^-1 rows and minus their sum); summed over the triangles, the largest entry: one number per case and quantity.  It is 0
         where nothing is active: such a case expects exact zeros.
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_shell_limit_mp_golden.py --measure
         prints it), times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction --, rounded up to a power of two.
         test_shell_limit_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

import shell_mp as smp
from shell_mp import _cross, _dot, _f, _sub, perturbed, rest_triangle, rot

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_shell_limit_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.49, gradient 3.02, Hessian 1.97 (all three: two triangles, Dirichlet nodes of both types -- the one case with nodes moved out of the plane at random;
# the next largest are 0.34 / 0.49 / 0.39).  `scale` counts one rounding of the largest entry, the restatement makes a few dozen on the way to it.
NUMPY_WORST_RATIO = 3.02
M = 32.0  # 8 x 3.02 = 24.2 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_limit_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    log = staticmethod(mp.log)
    log1p = staticmethod(mp.log1p)
    zero = mpf(0)
    inf = mp.inf


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    log = staticmethod(math.log)
    log1p = staticmethod(math.log1p)
    zero = 0.0
    inf = math.inf


def barrier(ops, sigma, on, lim):
    """(b, b', b'', y, z, L) at sigma < lim; zeros at or below the onset"""
    if not sigma > on:
        return ops.zero, ops.zero, ops.zero, ops.zero, ops.zero + 1, ops.zero
    w = lim - on
    y, z = (sigma - on) / w, (lim - sigma) / w
    L = ops.log1p(-y) if y < 0.5 else ops.log(z)
    yz = y / z
    return -y * y * L, (-2 * y * L + y * yz) / w, (-2 * L + 4 * yz + yz * yz) / (w * w), y, z, L


def stretches(ops, X, x):
    """sigma1 >= sigma2 of one triangle, and what the derivatives need: columns f of F, the node weights g[k][alpha], C12, d, r, f1 x f2 and its length, rest area"""
    B, A = rest_triangle(ops, X)
    e = [_sub(x[1], x[0]), _sub(x[2], x[0])]
    f = [[e[0][i] * B[0][al] + e[1][i] * B[1][al] for i in range(3)] for al in range(2)]
    g = [[-B[0][al] - B[1][al] for al in range(2)], B[0], B[1]]
    c11, c12, c22 = _dot(f[0], f[0]), _dot(f[0], f[1]), _dot(f[1], f[1])
    d = (c11 - c22) / 2
    r = ops.sqrt(d * d + c12 * c12)
    n = _cross(f[0], f[1])
    nn = ops.sqrt(_dot(n, n))
    s1 = ops.sqrt((c11 + c22) / 2 + r)
    s2 = min(nn / s1, s1) if s1 > 0 else ops.zero
    return s1, s2, {"f": f, "g": g, "c12": c12, "d": d, "r": r, "n": n, "nn": nn, "A": A}


def limit_term(ops, X, x, h, E, on, lim, stiff, magnitudes=False):
    """(energy, gradient[9], Hessian 9 x 9) of one limited triangle; (+inf, zeros, zeros) at or over the limit; magnitudes: the `scale` of the tolerance,
    one number per quantity spread over the entries"""
    z9 = [ops.zero] * 9
    Z = [[ops.zero] * 9 for _ in range(9)]
    s1, s2, m = stretches(ops, X, x)
    k = stiff * h * m["A"] * E
    if not s1 < lim:
        return (ops.zero, z9, Z) if magnitudes else (ops.inf, z9, Z)
    if not s1 > on:
        return ops.zero, z9, Z
    b1, d11, d21, y1, z1, L1 = barrier(ops, s1, on, lim)
    b2, d12, d22, y2, z2, L2 = barrier(ops, s2, on, lim)
    both = s2 > on
    f, g, r, d, c12 = m["f"], m["g"], m["r"], m["d"], m["c12"]
    w2 = (lim - on) * (lim - on)
    if both:
        q = 2 * r / (s1 + s2) / (lim - on) / z2
        lq = (L1 - L2) / q if q > 0.25 else (ops.log1p(-q) / q if q > 0 else -1)
        flip = max(((y1 + y2 - y1 * y2) / (z1 * z2) - 2 * (L1 + y2 * lq / z2)) / w2, ops.zero)
        twist = (d11 + d12) / (s1 + s2)
    if magnitudes:
        G = max(abs(gk[0]) + abs(gk[1]) for gk in g)
        lam = d21 + d11 / s1 + ((d22 + twist + flip + d12 / s2) if both else 2 * d11 * s1 / max(2 * r, (s1 - s2) * (s1 + s2)))
        return k * (b1 + b2), [k * (d11 + d12) * G] * 9, [[k * lam * G * G] * 9 for _ in range(9)]
    vx, vy = ops.zero + 1, ops.zero
    if r > 0:
        vx, vy = (r + d, c12) if d >= 0 else (c12, r - d)
        il = 1 / ops.sqrt(vx * vx + vy * vy)
        vx, vy = vx * il, vy * il
    u1 = [(f[0][c] * vx + f[1][c] * vy) / s1 for c in range(3)]
    w = [f[1][c] * vx - f[0][c] * vy for c in range(3)]
    sk = [g[k_][0] * vx + g[k_][1] * vy for k_ in range(3)]
    tk = [g[k_][1] * vx - g[k_][0] * vy for k_ in range(3)]
    is2 = 1 / s2 if both else ops.zero
    p1, p2 = k * d11, k * d12 * is2
    grad = [p1 * sk[k_] * u1[c] + p2 * tk[k_] * w[c] for k_ in range(3) for c in range(3)]
    I = lambda a, b: 1 if a == b else 0
    if both:
        al, be = k * (twist + flip) / 2, k * (flip - twist) / 2
        u2 = [v * is2 for v in w]
        u3 = [v / m["nn"] for v in m["n"]]
        n1, n2, h1, h2 = k * d11 / s1, k * d12 * is2, k * d21, k * d22
        S = [[h1 * u1[a] * u1[b] + al * u2[a] * u2[b] + n1 * u3[a] * u3[b] for b in range(3)] for a in range(3)]
        T = [[h2 * u2[a] * u2[b] + al * u1[a] * u1[b] + n2 * u3[a] * u3[b] for b in range(3)] for a in range(3)]
        Xm = [[be * u1[a] * u2[b] for b in range(3)] for a in range(3)]
    else:
        den = max(2 * r, (s1 - s2) * (s1 + s2))
        de = k * d11 / den
        al, ga, n1, h1 = de * s1, de / s1, k * d11 / s1, k * d21
        S = [[(h1 - n1) * u1[a] * u1[b] + n1 * I(a, b) + ga * w[a] * w[b] for b in range(3)] for a in range(3)]
        T = [[al * u1[a] * u1[b] for b in range(3)] for a in range(3)]
        Xm = [[de * u1[a] * w[b] for b in range(3)] for a in range(3)]
    H = [[sk[k_] * sk[l] * S[a][b] + tk[k_] * tk[l] * T[a][b] + tk[k_] * sk[l] * Xm[a][b] + sk[k_] * tk[l] * Xm[b][a] for l in range(3) for b in range(3)]
         for k_ in range(3) for a in range(3)]
    return k * (b1 + b2), grad, H


def patch_reference(ops, case, X=None, x=None, magnitudes=False):
    """E, g[3 n], dense H[3 n, 3 n] of the limit term over the limited triangles of a patch, as lists of ops numbers"""
    X = case["X"] if X is None else X
    x = case["x"] if x is None else x
    n = len(X)
    Xn = [[ops.num(v) for v in r] for r in X]
    xn = [[ops.num(v) for v in r] for r in x]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    for t, nodes in enumerate(np.asarray(case["tri"]).tolist()):
        if not case["limit"][t] > 0:
            continue
        e, ge, He = limit_term(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], ops.num(case["h"][t]), ops.num(case["YM"][t]), ops.num(case["onset"][t]),
                               ops.num(case["limit"][t]), ops.num(case["stiff"][t]), magnitudes)
        E = E + e
        idx = [3 * v + i for v in nodes for i in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + ge[p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + He[p][q]
    return E, g, H


def singular_values(ops, case):
    """[[sigma1, sigma2]] of every triangle of the case"""
    Xn = [[ops.num(v) for v in r] for r in case["X"]]
    xn = [[ops.num(v) for v in r] for r in case["x"]]
    return [list(stretches(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes])[:2]) for nodes in np.asarray(case["tri"]).tolist()]


def evaluate(case):
    """reference, sens and scale of E, g, H of one case (float64 arrays; the differences are taken in mpmath), and the singular values"""
    r = patch_reference(MP, case)
    sens = [0.0, np.zeros(3 * len(case["X"])), np.zeros((3 * len(case["X"]),) * 2)]
    if r[0] != mp.inf:  # (over the limit: the energy is +infinity for every perturbation, the derivatives are exact zeros)
        for s in range(SENS_SAMPLES):
            p = patch_reference(MP, case, perturbed(case["X"], 2 * s + 1), perturbed(case["x"], 2 * s + 2))
            sens[0] = max(sens[0], float(abs(p[0] - r[0])))
            sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
            sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
    m = patch_reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2], "sigma": _f(singular_values(MP, case))}


def numpy_restatement(case):
    E, g, H = patch_reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64)}


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (nothing active: exact zeros are expected) 0 for no error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
P_SHEARED = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.8, 0.0]])
P_RIGHT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TWO = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.8, 0.0], [0.4, -0.9, 0.0]])
TWO_TRI = [[0, 1, 2], [1, 0, 3]]


def _case(name, X, x, tri=((0, 1, 2),), limit=1.2, onset=1.0, stiff=1.0, h=0.01, YM=1e5, dbc=None):
    X, x, tri = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    nt = len(tri)
    per = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (nt,)).copy()
    return {"name": name, "X": X, "x": x, "tri": tri, "h": per(h), "YM": per(YM), "PR": np.full(nt, 0.3), "rho": np.full(nt, 1000.0),
            "limit": per(limit), "onset": per(onset), "stiff": per(stiff), "dbc": np.zeros(len(X), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32)}


def scaled(P, a, b):
    """the in-plane triangle P stretched by a along x and b along y: principal stretches a and b (up to the rounding of the products)"""
    return np.asarray(P) * [a, b, 1.0]


def cases():
    rng = np.random.default_rng(23)
    R = rot([1, 2, 3], 50)
    T = np.array([[0.1, 0.2, 0.3], [1.1, 0.3, 0.2], [0.4, 1.0, 0.5]])
    c = T.mean(axis=0)
    out = [_case("both stretches below the onset", P_SHEARED, scaled(P_SHEARED, 0.9, 0.95)),
           _case("one stretch active", P_SHEARED, scaled(P_SHEARED, 1.1, 0.9)),
           _case("both stretches active", P_SHEARED, scaled(P_SHEARED, 1.15, 1.05) @ R.T + 0.1),
           _case("equal stretches exactly", P_RIGHT, P_RIGHT * 1.125, limit=1.25),
           _case("stretches 1e-9 apart", P_SHEARED @ R.T, scaled(P_SHEARED, 1.1 + 1e-9, 1.1) @ R.T),
           _case("stretch 1e-6 of the range below the limit", P_SHEARED, scaled(P_SHEARED, 1.2 - 1e-6 * 0.2, 1.0)),
           _case("stretch over the limit", P_SHEARED, scaled(P_SHEARED, 1.25, 1.0)),
           _case("triangle collapsed to a line", P_SHEARED, scaled(P_SHEARED, 1.1, 0.0)),
           _case("sheared and rotated rest triangle", T, c + ((T - c) * [1.15, 1.05, 1.0]) @ R.T),
           _case("stiff 2.5, onset 1.05", P_SHEARED, scaled(P_SHEARED, 1.2, 1.1), limit=1.3, onset=1.05, stiff=2.5),
           _case("limited and unlimited triangle sharing an edge", TWO, scaled(TWO, 1.1, 1.05), TWO_TRI, limit=[1.2, 0.0]),
           _case("two triangles, Dirichlet nodes of both types", TWO, scaled(TWO, 1.12, 1.08) + 0.02 * rng.standard_normal(TWO.shape), TWO_TRI, dbc=[1, 0, 2, 0])]
    return out


CASE_KEYS = ("X", "x", "tri", "h", "YM", "PR", "rho", "limit", "onset", "stiff", "dbc")


def pack():
    cs = cases()
    out = {"names": np.array([c["name"] for c in cs])}
    for i, c in enumerate(cs):
        r = evaluate(c)
        for k in CASE_KEYS:
            out[f"c{i}_{k}"] = c[k]
        for k, v in r.items():
            out[f"c{i}_{k}"] = np.asarray(v)
    return out


def load(path=GOLDEN):
    z = np.load(path)
    res = []
    for i, name in enumerate(z["names"]):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        c["name"] = str(name)
        for k in ("E", "sens_E", "scale_E", "scale_g", "scale_H"):
            c[k] = float(c[k])
        res.append(c)
    return res


def expected(case, k, coef=1.0, projectDBC=True):
    """(reference, tolerance) of quantity k at `coef`; gradient entries, rows and columns of projected Dirichlet nodes dropped (type 1 always, 2 with projectDBC)"""
    ref, tol = coef * np.array(case[k], dtype=np.float64), np.array(tolerance(case, k, coef), dtype=np.float64)
    if k == "E":
        return float(ref), float(tol)
    proj = np.repeat((case["dbc"] == 1) | ((case["dbc"] == 2) & bool(projectDBC)), 3)
    ref[proj] = 0.0
    if k == "H":
        ref[:, proj] = 0.0
    return ref, tol
