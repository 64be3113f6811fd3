"""mpmath restatement of the rubber membrane of the elastic shells (ipc_amd/csrc/shell_rubber_kernels.h): the incompressible Mooney-Rivlin membrane, its
gradient and its PSD Hessian; a project extension, so there is no oracle to compare with -- this file is the reference, pinned by
tests/test_shell_rubber_mp.py (mp.diff, rigid motions, the closed form on diagonal F, the StVK Hessian at rest, mp.eigsy, +infinity at collinear nodes).

Per rubber triangle (rest X, current x, thickness h, Young's modulus E, fraction alpha, rest area A):  F = [x1 - x0, x2 - x0] Dm^-1 as the membrane's
(shell_mp.rest_triangle), C = F^T F, tr = C11 + C22, J = det C = |f1 x f2|^2 (Lagrange's identity; the form the kernels use -- test_shell_rubber_mp.py pins
the identity),
  I1 = tr + 1 / J,  I2 = tr / J + J,  W = h A (c1 (I1 - 3) + c2 (I2 - 3)),  c1 = mu (1 - alpha) / 2,  c2 = mu alpha / 2,  mu = E / 3.
Gradient F S with S = a I + b adj C; Hessian 9 x 9 from S (x) I + p (j t^T + t j^T) + q j j^T + (b / 2) (u1 u2^T + u2 u1^T - 2 u12 u12^T) in F (the header
names the vectors), eigenvalues clamped at 0 (mp.eigsy).  A triangle with J <= 0 (collinear nodes) or, in float64, a J or a coefficient that is not finite:
energy +infinity, gradient and Hessian zero.

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64 with numpy.linalg.eigh): the float64 instance is the
"NumPy restatement" whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/shell_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every rest and current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  q with every term of its formula replaced by its magnitude (tr + 1 / J + 3, |coordinates| summed in the edge vectors, |Dm^-1|, products of absolute
         values; the denominators J keep their true value), the largest entry for the gradient and the Hessian: one number per case and quantity
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_shell_rubber_mp_golden.py --measure
         prints it), times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction, Jacobi rotations instead of LAPACK
         --, rounded up to a power of two.  test_shell_rubber_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

import shell_mp as smp
from shell_mp import _cross, _dot, _f, _sub, perturbed, rest_triangle, rot

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_shell_rubber_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.38 (det C about 1e-6), gradient 0.38 (biaxial stretch 2, alpha 0), Hessian 1.57 (biaxial stretch 2, alpha 0: equal stretches, a double eigenvalue,
# where sens is small and the restatement makes a few dozen roundings on the way to the largest entry that `scale` counts once)
NUMPY_WORST_RATIO = 1.57
M = 16.0  # 8 x 1.57 = 12.6 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_rubber_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


class MP(smp.MP):
    inf = mp.inf
    isfinite = staticmethod(lambda v: mp.isfinite(v))


class NP(smp.NP):
    inf = math.inf
    isfinite = staticmethod(math.isfinite)


def constants(h, A, E, alpha):
    """k1 = h A c1, k2 = h A c2"""
    mu = E / 3
    return h * A * mu * (1 - alpha) / 2, h * A * mu * alpha / 2


def psi_principal(l1, l2, mu, alpha):
    """the closed form in the principal stretches"""
    j = (l1 * l2) ** 2
    return mu * (1 - alpha) / 2 * (l1 * l1 + l2 * l2 + 1 / j - 3) + mu * alpha / 2 * ((l1 * l1 + l2 * l2) / j + j - 3)


def rubber(ops, X, x, h, E, alpha, hessian=True, project=True, magnitudes=False):
    """(energy, gradient[9], Hessian 9 x 9 or None) of one rubber triangle; (+inf, zeros, zeros) for a degenerate one; magnitudes: every term replaced by its
    magnitude (the `scale` of the tolerance; 0 for a degenerate triangle)"""
    z9 = [ops.zero] * 9
    Z = [[ops.zero] * 9 for _ in range(9)] if hessian else None
    B, A = rest_triangle(ops, X)
    k1, k2 = constants(h, A, E, alpha)
    e = [_sub(x[1], x[0]), _sub(x[2], x[0])]
    f = [[e[0][i] * B[0][al] + e[1][i] * B[1][al] for i in range(3)] for al in range(2)]
    n = _cross(f[0], f[1])
    J = _dot(n, n)
    c11, c12, c22 = _dot(f[0], f[0]), _dot(f[0], f[1]), _dot(f[1], f[1])
    tr = c11 + c22
    ok = J > 0 and ops.isfinite(J)
    if ok:
        iJ = 1 / J
        s = (k1 + k2 * tr) * (iJ * iJ)
        a, b, p, q = 2 * (k1 + k2 * iJ), 2 * (k2 - s), -k2 * (iJ * iJ), 2 * s * iJ
        W = k1 * ((tr + iJ) - 3) + k2 * ((tr * iJ + J) - 3)
        ok = ops.isfinite(a) and ops.isfinite(b) and ops.isfinite(q) and W < ops.inf
    if not ok:
        return (ops.zero if magnitudes else ops.inf), z9, Z
    Jm = J
    if magnitudes:
        e = [[abs(x[1][i]) + abs(x[0][i]) for i in range(3)], [abs(x[2][i]) + abs(x[0][i]) for i in range(3)]]
        B = [[abs(v) for v in r] for r in B]
        f = [[e[0][i] * B[0][al] + e[1][i] * B[1][al] for i in range(3)] for al in range(2)]
        c11, c12, c22 = _dot(f[0], f[0]), _dot(f[0], f[1]), _dot(f[1], f[1])
        tr = c11 + c22
        Jm = c11 * c22 + c12 * c12
        s = (k1 + k2 * tr) * (iJ * iJ)
        a, b, p, q = 2 * (k1 + k2 * iJ), 2 * (k2 + s), k2 * (iJ * iJ), 2 * s * iJ
        W = k1 * (tr + iJ + 3) + k2 * (tr * iJ + Jm + 3)
    sg = 1 if magnitudes else -1
    S = [[a + b * c22, sg * b * c12], [sg * b * c12, a + b * c11]]
    P = [[S[al][0] * f[0][i] + S[al][1] * f[1][i] for i in range(3)] for al in range(2)]  # dW/df_alpha
    ge = [[P[0][i] * B[k][0] + P[1][i] * B[k][1] for i in range(3)] for k in range(2)]  # dW/de_k
    g = [(-ge[0][i] - ge[1][i]) if not magnitudes else (ge[0][i] + ge[1][i]) for i in range(3)] + ge[0] + ge[1]
    if not hessian:
        return W, g, None
    # the 6-vectors by their coefficients on (f1, f2), index 2 al + mu
    jt = [2 * c22, sg * 2 * c12, sg * 2 * c12, 2 * c11]
    tt, u1, u2, u12 = [2, 0, 0, 2], [2, 0, 0, 0], [0, 0, 0, 2], [0, 1, 1, 0]
    hb = b / 2
    M4 = [[p * (jt[r] * tt[c] + tt[r] * jt[c]) + q * jt[r] * jt[c] + hb * (u1[r] * u2[c] + u2[r] * u1[c] + sg * 2 * u12[r] * u12[c]) for c in range(4)] for r in range(4)]
    d = lambda i, j: 1 if i == j else 0
    Hf = [[[[S[al][be] * d(i, j) + sum(M4[2 * al + m_][2 * be + n_] * f[m_][i] * f[n_][j] for m_ in range(2) for n_ in range(2)) for j in range(3)] for i in range(3)]
           for be in range(2)] for al in range(2)]
    # f_alpha = sum_n w[n][alpha] x_n with w[0] = -(B[0] + B[1]), w[1] = B[0], w[2] = B[1]
    wgt = [[(-B[0][al] - B[1][al]) if not magnitudes else (B[0][al] + B[1][al]) for al in range(2)], B[0], B[1]]
    H = [[sum(wgt[k][al] * wgt[l][be] * Hf[al][be][i][j] for al in range(2) for be in range(2)) for l in range(3) for j in range(3)] for k in range(3) for i in range(3)]
    if project and not magnitudes:
        H = ops.clamp(H, 9)
    return W, g, H


def patch_reference(ops, case, X=None, x=None, magnitudes=False):
    """E, g[3 n], dense H[3 n, 3 n] of the rubber term over the rubber triangles of a patch, as lists of ops numbers"""
    X = case["X"] if X is None else X
    x = case["x"] if x is None else x
    n = len(X)
    Xn = [[ops.num(v) for v in r] for r in X]
    xn = [[ops.num(v) for v in r] for r in x]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    for t, nodes in enumerate(np.asarray(case["tri"]).tolist()):
        if case["model"][t] != 1:
            continue
        e, ge, He = rubber(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], ops.num(case["h"][t]), ops.num(case["YM"][t]), ops.num(case["alpha"][t]),
                           magnitudes=magnitudes)
        E = E + e
        idx = [3 * v + i for v in nodes for i in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + ge[p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + He[p][q]
    return E, g, H


def singular_values(case):
    """[[sigma1, sigma2]] of every triangle of the case (mpmath, as floats): the strain limit's closed form"""
    import shell_limit_mp as lmp
    Xn = [[MP.num(v) for v in r] for r in case["X"]]
    xn = [[MP.num(v) for v in r] for r in case["x"]]
    return _f([list(lmp.stretches(lmp.MP, [Xn[v] for v in nodes], [xn[v] for v in nodes])[:2]) for nodes in np.asarray(case["tri"]).tolist()])


def evaluate(case):
    """reference, sens and scale of E, g, H of one case (float64 arrays; the differences are taken in mpmath), and the singular values"""
    r = patch_reference(MP, case)
    sens = [0.0, np.zeros(3 * len(case["X"])), np.zeros((3 * len(case["X"]),) * 2)]
    if r[0] != mp.inf:  # (degenerate: the energy is +infinity, the derivatives are exact zeros)
        for s in range(SENS_SAMPLES):
            p = patch_reference(MP, case, perturbed(case["X"], 2 * s + 1), perturbed(case["x"], 2 * s + 2))
            sens[0] = max(sens[0], float(abs(p[0] - r[0])))
            sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
            sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
    m = patch_reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2], "sigma": singular_values(case)}


def numpy_restatement(case):
    E, g, H = patch_reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64)}


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (a degenerate triangle: exact zeros are expected) 0 for no error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
P_SHEARED = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.8, 0.0]])
TWO = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.8, 0.0], [0.4, -0.9, 0.0]])
TWO_TRI = [[0, 1, 2], [1, 0, 3]]
ALPHAS = (0.0, 0.1, 0.5)
# the strip of the GPU test (tests/test_gpu_shell_rubber_mp.py): cells of side STRIP_H, every coordinate and the deformation dyadic, so that every "up" triangle
# (a, a + 1, a + n + 1) and every "down" triangle (a, a + n + 1, a + n) of the strip has bit for bit the edge vectors of the one stored here
STRIP_H = 0.125
STRIP_MAP = np.array([[1.5, 0.0, 0.0], [0.0, 1.25, 0.0], [0.25, 0.0, 1.0]])  # x = STRIP_MAP X: stretches and lifts out of the plane
STRIP_UP = np.array([[0.0, 0.0, 0.0], [STRIP_H, 0.0, 0.0], [STRIP_H, STRIP_H, 0.0]])
STRIP_DOWN = np.array([[0.0, 0.0, 0.0], [STRIP_H, STRIP_H, 0.0], [0.0, STRIP_H, 0.0]])


def _case(name, X, x, tri=((0, 1, 2),), model=1, alpha=0.1, h=0.01, YM=1e5, dbc=None):
    X, x, tri = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    nt = len(tri)
    per = lambda v, dt=np.float64: np.broadcast_to(np.asarray(v, dtype=dt), (nt,)).copy()
    return {"name": name, "X": X, "x": x, "tri": tri, "h": per(h), "YM": per(YM), "PR": np.full(nt, 0.3), "rho": np.full(nt, 1000.0),
            "model": per(model, np.int32), "alpha": per(alpha), "dbc": np.zeros(len(X), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32)}


def scaled(P, a, b):
    """the in-plane triangle P stretched by a along x and b along y: principal stretches a and b (up to the rounding of the products)"""
    return np.asarray(P) * [a, b, 1.0]


def deformations():
    R = rot([1, 2, 3], 50)
    T = np.array([[0.1, 0.2, 0.3], [1.1, 0.3, 0.2], [0.4, 1.0, 0.5]])
    c = T.mean(axis=0)
    return [("at rest", T, T), ("rotated", T, c + (T - c) @ R.T), ("biaxial stretch 2", P_SHEARED, scaled(P_SHEARED, 2.0, 2.0) @ R.T + 0.1),
            ("biaxial stretch 4", P_SHEARED, scaled(P_SHEARED, 4.0, 4.0)), ("uniaxial 2, lateral 1/sqrt 2", P_SHEARED, scaled(P_SHEARED, 2.0, 1.0 / np.sqrt(2.0)) @ R.T),
            ("sheared", T, T + np.outer(T[:, 1], [0.4, 0, 0.1])), ("compressed to 0.3", T, c + (T - c) * 0.3),
            ("det C about 1e-6", P_SHEARED, scaled(P_SHEARED, 1.0, 1e-3) @ R.T), ("exactly collinear", P_SHEARED, scaled(P_SHEARED, 1.1, 0.0))]


def cases():
    rng = np.random.default_rng(31)
    out = []
    for name, X, x in deformations():
        for al in ALPHAS:
            if al == 0.1 or name in ("at rest", "biaxial stretch 2", "sheared", "compressed to 0.3"):
                out.append(_case(f"{name}, alpha {al:g}", X, x, alpha=al))
    out.append(_case("StVK and rubber triangle sharing an edge", TWO, scaled(TWO, 1.3, 1.1), TWO_TRI, model=[0, 1], alpha=[0.7, 0.5]))
    out.append(_case("two rubber triangles, Dirichlet nodes of both types", TWO, scaled(TWO, 1.4, 0.8) + 0.02 * rng.standard_normal(TWO.shape), TWO_TRI, alpha=[0.0, 0.5],
                     dbc=[1, 0, 2, 0]))
    out.append(_case("one projected Dirichlet node", P_SHEARED, scaled(P_SHEARED, 0.6, 1.2), dbc=[0, 2, 0]))
    out.append(_case("strip, up triangle", STRIP_UP, STRIP_UP @ STRIP_MAP.T))
    out.append(_case("strip, down triangle", STRIP_DOWN, STRIP_DOWN @ STRIP_MAP.T))
    return out


CASE_KEYS = ("X", "x", "tri", "h", "YM", "PR", "rho", "model", "alpha", "dbc")


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
