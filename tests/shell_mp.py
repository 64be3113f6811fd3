"""mpmath restatement of the elastic shell energies (ipc_amd/csrc/shell_kernels.h), their gradients and PSD Hessians; a project extension, so there is no
oracle to compare with -- this file is the reference, pinned by tests/test_shell_mp.py (mp.diff, rigid motions, closed forms, hand-placed hinges).

Membrane, per triangle (rest X, current x, thickness h, E, nu, rest area A):  Dm = [X1 - X0, X2 - X0] in an orthonormal frame of the rest plane,
F = [x1 - x0, x2 - x0] Dm^-1, G = (F^T F - I) / 2, psi = mu |G|^2 + lambda_ps tr(G)^2 / 2, energy h A psi; Hessian 9 x 9, eigenvalues clamped at 0 (mp.eigsy).
Bending, per hinge (x0, x1 on the edge, x2, x3 opposite): theta = atan2((n1 x n2) . e / |e|, n1 . n2), e = x1 - x0, n1 = e x (x2 - x0), n2 = (x0 - x1) x (x3 - x1);
energy bendScale k_b w_e (theta - thetaBar)^2, w_e = 3 |eBar|^2 / (A1 + A2), k_b = mean E h^3 / (24 (1 - nu^2)); Hessian 2 bendScale k_b w_e grad theta grad theta^T.

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64 with numpy.linalg.eigh): the float64 instance is the
"NumPy restatement" whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/snh_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every rest and current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  q with every term of its formula replaced by its magnitude (|c| + 1 for c - 1, |theta| + |thetaBar|, products of absolute values, sums over the
         elements that share a node), the largest entry for the gradient and the Hessian: one number per case and quantity
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_shell_mp_golden.py --measure prints it),
         times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction, Jacobi rotations instead of LAPACK --, rounded up
         to a power of two.  test_shell_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_shell_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.058 (triangle stretched), gradient 0.22 (triangle stretched), Hessian 0.50 (triangle rotated)
NUMPY_WORST_RATIO = 0.50
M = 4.0  # 8 x 0.50 = 3.98 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    atan2 = staticmethod(mp.atan2)
    zero = mpf(0)

    @staticmethod
    def clamp(A, n):
        """eigenvalue clamp at 0 of the symmetric n x n list-of-lists A"""
        w, Q = mp.eigsy(mp.matrix(A))
        return [[sum(Q[i, k] * (w[k] if w[k] > 0 else 0) * Q[j, k] for k in range(n)) for j in range(n)] for i in range(n)]


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    atan2 = staticmethod(math.atan2)
    zero = 0.0

    @staticmethod
    def clamp(A, n):
        w, Q = np.linalg.eigh(np.array(A, dtype=np.float64))
        return ((Q * np.maximum(w, 0.0)) @ Q.T).tolist()


def _sub(a, b):
    return [a[i] - b[i] for i in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def lame(E, nu):
    return E / (2 * (1 + nu)), E * nu / (1 - nu * nu)


def rest_triangle(ops, X):
    """Dm^-1 (2 x 2) in the frame whose first axis runs along X1 - X0, and the rest area"""
    u, w = _sub(X[1], X[0]), _sub(X[2], X[0])
    n = _cross(u, w)
    l, twoA = ops.sqrt(_dot(u, u)), ops.sqrt(_dot(n, n))
    p, q = _dot(w, u) / l, twoA / l
    return [[1 / l, -p / (l * q)], [ops.zero, 1 / q]], twoA / 2


def membrane(ops, X, x, h, E, nu, hessian=True, project=True, magnitudes=False):
    """(energy, gradient[9], Hessian 9 x 9 or None) of one triangle; magnitudes: every term replaced by its magnitude (the `scale` of the tolerance)"""
    a = abs if magnitudes else (lambda v: v)
    B, A = rest_triangle(ops, X)
    mu, lam = lame(E, nu)
    cm, cl = h * A * mu, h * A * lam
    e = [_sub(x[1], x[0]), _sub(x[2], x[0])]
    if magnitudes:
        e = [[abs(x[1][i]) + abs(x[0][i]) for i in range(3)], [abs(x[2][i]) + abs(x[0][i]) for i in range(3)]]
        B = [[abs(v) for v in r] for r in B]
        cl = abs(cl)
    f = [[e[0][i] * B[0][al] + e[1][i] * B[1][al] for i in range(3)] for al in range(2)]
    one = -1 if not magnitudes else 1
    G11, G22, G12 = (_dot(f[0], f[0]) + one) / 2, (_dot(f[1], f[1]) + one) / 2, _dot(f[0], f[1]) / 2
    tr = G11 + G22
    S = [[2 * cm * G11 + cl * tr, 2 * cm * G12], [2 * cm * G12, 2 * cm * G22 + cl * tr]]
    energy = cm * (G11 * G11 + 2 * G12 * G12 + G22 * G22) + cl * tr * tr / 2
    P = [[S[al][0] * f[0][i] + S[al][1] * f[1][i] for i in range(3)] for al in range(2)]  # dW/df_alpha
    ge = [[P[0][i] * B[k][0] + P[1][i] * B[k][1] for i in range(3)] for k in range(2)]  # dW/de_k
    g = [(-ge[0][i] - ge[1][i]) if not magnitudes else (ge[0][i] + ge[1][i]) for i in range(3)] + ge[0] + ge[1]
    if not hessian:
        return energy, g, None
    c2 = 2 * cm + cl
    d = lambda i, j: 1 if i == j else 0
    Hf = [[None, None], [None, None]]  # d2W / df_alpha df_beta, 3 x 3 each
    Hf[0][0] = [[S[0][0] * d(i, j) + c2 * f[0][i] * f[0][j] + cm * f[1][i] * f[1][j] for j in range(3)] for i in range(3)]
    Hf[1][1] = [[S[1][1] * d(i, j) + c2 * f[1][i] * f[1][j] + cm * f[0][i] * f[0][j] for j in range(3)] for i in range(3)]
    Hf[0][1] = [[S[0][1] * d(i, j) + cl * f[0][i] * f[1][j] + cm * f[1][i] * f[0][j] for j in range(3)] for i in range(3)]
    Hf[1][0] = [[Hf[0][1][j][i] for j in range(3)] for i in range(3)]
    # f_alpha = sum_n w[n][alpha] x_n with w[0] = -(B[0] + B[1]), w[1] = B[0], w[2] = B[1]
    wgt = [[(-B[0][al] - B[1][al]) if not magnitudes else (B[0][al] + B[1][al]) for al in range(2)], B[0], B[1]]
    H = [[sum(wgt[k][al] * wgt[l][be] * Hf[al][be][i][j] for al in range(2) for be in range(2)) for l in range(3) for j in range(3)] for k in range(3) for i in range(3)]
    if project and not magnitudes:
        H = ops.clamp(H, 9)
    return energy, g, H


def hinge_angle(ops, x, gradient=False, magnitudes=False):
    """theta of the hinge x = (x0, x1, x2, x3) and optionally its gradient[12]"""
    e, a, b, c = _sub(x[1], x[0]), _sub(x[2], x[0]), _sub(x[0], x[1]), _sub(x[3], x[1])
    n1, n2 = _cross(e, a), _cross(b, c)
    le = ops.sqrt(_dot(e, e))
    theta = ops.atan2(_dot(_cross(n1, n2), e) / le, _dot(n1, n2))
    if not gradient:
        return theta, None
    m = abs if magnitudes else (lambda v: v)
    a1, a2 = [v / _dot(n1, n1) for v in n1], [v / _dot(n2, n2) for v in n2]
    d12, d13 = _dot(_sub(x[1], x[2]), e) / le, _dot(_sub(x[1], x[3]), e) / le
    d20, d30 = _dot(a, e) / le, _dot(_sub(x[3], x[0]), e) / le
    g = [m(d12 * a1[i]) + m(d13 * a2[i]) for i in range(3)] + [m(d20 * a1[i]) + m(d30 * a2[i]) for i in range(3)]
    g += [m(-le * a1[i]) for i in range(3)] + [m(-le * a2[i]) for i in range(3)]
    return theta, g


def hinge_constants(ops, X, hE):
    """X: rest positions of (x0, x1, x2, x3); hE: ((h, E, nu) of the triangle of x2, the same of x3) -> thetaBar, w_e, k_b"""
    thetaBar, _ = hinge_angle(ops, X)
    e = _sub(X[1], X[0])
    A1 = ops.sqrt(_dot(*[_cross(e, _sub(X[2], X[0]))] * 2)) / 2
    A2 = ops.sqrt(_dot(*[_cross(e, _sub(X[3], X[0]))] * 2)) / 2
    kb = sum(E * h ** 3 / (24 * (1 - nu * nu)) for h, E, nu in hE) / 2
    return thetaBar, 3 * _dot(e, e) / (A1 + A2), kb


def hinge(ops, X, x, hE, bendScale, magnitudes=False):
    """(energy, gradient[12], Gauss-Newton Hessian 12 x 12) of one hinge"""
    thetaBar, w, kb = hinge_constants(ops, X, hE)
    theta, g = hinge_angle(ops, x, True, magnitudes)
    k = bendScale * kb * w
    d = (abs(theta) + abs(thetaBar)) if magnitudes else theta - thetaBar
    return k * d * d, [2 * k * d * v for v in g], [[2 * k * gi * gj for gj in g] for gi in g]


def hinges_of(tri):
    """hinges of a consistently oriented triangle list, ascending by (smaller, larger) edge node: rows (x0, x1, x2, x3, triangle of x2, triangle of x3)"""
    half = {}
    for t, (a, b, c) in enumerate(np.asarray(tri).tolist()):
        for p, q, o in ((a, b, c), (b, c, a), (c, a, b)):
            half.setdefault((min(p, q), max(p, q)), []).append((p < q, o, t))
    out = []
    for (lo, hi) in sorted(half):
        hs = half[(lo, hi)]
        if len(hs) == 2:
            f, g = (hs[0], hs[1]) if hs[0][0] else (hs[1], hs[0])
            assert f[0] and not g[0], "inconsistent orientation"
            out.append((lo, hi, f[1], g[1], f[2], g[2]))
    return out


def patch_reference(ops, case, X=None, x=None, magnitudes=False):
    """E, g[3 n], dense H[3 n, 3 n] (projected membrane + Gauss-Newton hinges) of a patch of triangles, as lists of ops numbers"""
    X = case["X"] if X is None else X
    x = case["x"] if x is None else x
    n = len(X)
    Xn = [[ops.num(v) for v in r] for r in X]
    xn = [[ops.num(v) for v in r] for r in x]
    tri = np.asarray(case["tri"]).tolist()
    mat = [(ops.num(case["h"][t]), ops.num(case["YM"][t]), ops.num(case["PR"][t])) for t in range(len(tri))]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]

    def scatter(nodes, e, ge, He):
        nonlocal E
        E = E + e
        idx = [3 * v + i for v in nodes for i in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + ge[p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + He[p][q]

    for t, nodes in enumerate(tri):
        scatter(nodes, *membrane(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], *mat[t], magnitudes=magnitudes))
    for (v0, v1, v2, v3, ta, tb) in hinges_of(tri):
        nodes = (v0, v1, v2, v3)
        scatter(nodes, *hinge(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], (mat[ta], mat[tb]), ops.num(case["bendScale"]), magnitudes))
    return E, g, H


def _f(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, (float, mpf)) else float(v)


def perturbed(A, seed):
    A = np.asarray(A, dtype=np.float64)
    s = np.random.default_rng(seed).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case):
    """reference, sens and scale of E, g, H of one case (float64 arrays; the differences are taken in mpmath)"""
    r = patch_reference(MP, case)
    sens = [0.0, np.zeros(3 * len(case["X"])), np.zeros((3 * len(case["X"]),) * 2)]
    for s in range(SENS_SAMPLES):
        p = patch_reference(MP, case, perturbed(case["X"], 2 * s + 1), perturbed(case["x"], 2 * s + 2))
        sens[0] = max(sens[0], float(abs(p[0] - r[0])))
        sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
        sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
    m = patch_reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2]}


def numpy_restatement(case):
    E, g, H = patch_reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64)}


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _case(name, X, x, tri, h=0.01, YM=1e5, PR=0.3, dbc=None, bendScale=1.0):
    X, x, tri = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    nt = len(tri)
    return {"name": name, "X": X, "x": x, "tri": tri, "h": np.full(nt, h), "YM": np.full(nt, YM), "PR": np.full(nt, PR), "rho": np.full(nt, 1000.0),
            "dbc": np.zeros(len(X), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32), "bendScale": bendScale}


def fold(angle_deg, apex=(0.4, -0.9)):
    """the fourth node of a hinge on the edge (0,0,0)-(1,0,0) whose triangle (x0, x1, x2) lies in z = 0 with x2 at y > 0: signed dihedral angle angle_deg"""
    t = np.radians(angle_deg)
    return np.array([apex[0], apex[1] * np.cos(t), apex[1] * np.sin(t)])


HINGE_TRI = [[0, 1, 2], [1, 0, 3]]


def hinge_nodes(angle_deg, apex=(0.4, -0.9)):
    return np.array([[0, 0, 0], [1, 0, 0], [0.3, 0.8, 0], fold(angle_deg, apex)], dtype=np.float64)


def grid(n, m=None, spacing=0.1):
    """n x m nodes in the plane z = 0, two triangles per cell, consistently oriented (normal +z)"""
    m = n if m is None else m
    V = np.array([[i * spacing, j * spacing, 0.0] for j in range(m) for i in range(n)])
    tri = []
    for j in range(m - 1):
        for i in range(n - 1):
            a = j * n + i
            tri += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return V, np.array(tri, dtype=np.int32)


def cases():
    rng = np.random.default_rng(7)
    T = np.array([[0.1, 0.2, 0.3], [1.1, 0.3, 0.2], [0.4, 1.0, 0.5]])
    c = T.mean(axis=0)
    R = rot([1, 2, 3], 50)
    out = [_case("triangle at rest", T, T, [[0, 1, 2]]),
           _case("triangle stretched", T, c + (T - c) * [1.3, 1.1, 1.0], [[0, 1, 2]]),
           _case("triangle sheared", T, T + np.outer(T[:, 1], [0.4, 0, 0.1]), [[0, 1, 2]], dbc=[2, 0, 0]),
           _case("triangle compressed", T, c + (T - c) * 0.6, [[0, 1, 2]]),
           _case("triangle compressed, one Dirichlet node", T, c + (T - c) * 0.7, [[0, 1, 2]], dbc=[0, 1, 0]),
           _case("triangle rotated", T, c + (T - c) @ R.T, [[0, 1, 2]]),
           _case("triangle rotated and stretched", T, c + ((T - c) * [1.2, 0.8, 1.0]) @ R.T, [[0, 1, 2]], PR=0.45),
           _case("triangle 1:100 at rest", [[0, 0, 0], [1, 0, 0], [0.5, 0.01, 0]], [[0, 0, 0], [1, 0, 0], [0.5, 0.01, 0]], [[0, 1, 2]]),
           _case("triangle 1:100 deformed", [[0, 0, 0], [1, 0, 0], [0.5, 0.01, 0]], [[0, 0, 0.001], [1.02, 0, 0], [0.5, 0.012, -0.001]], [[0, 1, 2]])]
    for rest, angles in ((0, (0, 30, 90, -90, 170, -170)), (40, (40, -20, 170, -170))):
        for ang in angles:
            x = hinge_nodes(ang)
            if ang in (30, -20):
                x = x @ R.T + 0.2
            out.append(_case(f"hinge rest {rest} at {ang}", hinge_nodes(rest), x, HINGE_TRI, dbc=[0, 0, 2, 0] if ang == 90 else None))
    out.append(_case("hinge, two materials", hinge_nodes(10), hinge_nodes(60) * 1.05, HINGE_TRI))
    out[-1]["h"][1], out[-1]["YM"][1], out[-1]["PR"][1] = 0.02, 3e5, 0.2
    V, tri = grid(3)
    out.append(_case("3x3 grid perturbed", V, V + 0.01 * rng.standard_normal(V.shape), tri, dbc=[1, 0, 0, 0, 0, 0, 0, 0, 2]))
    return out


def pack():
    cs = cases()
    out = {"names": np.array([c["name"] for c in cs])}
    for i, c in enumerate(cs):
        r = evaluate(c)
        for k in ("X", "x", "tri", "h", "YM", "PR", "rho", "dbc"):
            out[f"c{i}_{k}"] = c[k]
        out[f"c{i}_bendScale"] = np.float64(c["bendScale"])
        for k, v in r.items():
            out[f"c{i}_{k}"] = np.asarray(v)
    return out


def load(path=GOLDEN):
    z = np.load(path)
    res = []
    for i, name in enumerate(z["names"]):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        c["name"] = str(name)
        c["bendScale"] = float(c["bendScale"])
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
