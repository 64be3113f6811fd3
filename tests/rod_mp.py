"""mpmath restatement of the elastic rod energies (ipc_amd/csrc/rod_kernels.h), their gradients and PSD Hessians; a project extension, so there is no
oracle to compare with -- this file is the reference, pinned by tests/test_rod_mp.py (mp.diff, mp.eigsy, rigid motions, closed forms, hand-placed angles).

Stretching, per segment (a, b) (rest length L, length l, radius r, E):  k_s = E pi r^2 / L, W_s = k_s (l - L)^2 / 2; Hessian [[B, -B], [-B, B]] with
B = k_s [t t^T + max(0, 1 - L / l) (I - t t^T)], t = (x_b - x_a) / l: the eigenvalue clamp at 0 in closed form.
Bending, per node b with exactly two segments (a, b), (b, c):  e0 = x_b - x_a, e1 = x_c - x_b, kb = 2 e0 x e1 / d, d = |e0||e1| + e0 . e1,
W_b = bendScale k_b |kb|^2 with |kb|^2 = 4 (|e0||e1| - e0 . e1) / d, k_b = E_m pi r_m^4 / 4 / (L0 + L1) (means of the two segments); +infinity where d <= 0;
gradient 2 bendScale k_b J^T kb, Hessian 2 bendScale k_b J^T J (Gauss-Newton), J = d kb / d (x_a, x_b, x_c).

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64): the float64 instance is the "NumPy restatement"
whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/shell_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every rest and current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  q with every term of its formula replaced by its magnitude (|l| + |L| for l - L, |p| + |q| for p - q, products of absolute values, sums over the
         elements that share a node), the largest entry for the gradient and the Hessian: one number per case and quantity
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_rod_mp_golden.py --measure prints it),
         times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction --, rounded up to a power of two.
         test_rod_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_rod_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.031 (three-armed junction), gradient 0.175 (closed six-node ring), Hessian 0.161 (closed six-node ring)
NUMPY_WORST_RATIO = 0.175
M = 2.0  # 8 x 0.175 = 1.4 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rod_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    zero = mpf(0)
    inf = mp.inf
    pi = mp.pi


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    zero = 0.0
    inf = math.inf
    pi = math.pi


def _sub(a, b):
    return [a[i] - b[i] for i in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _cross_abs(a, b):
    return [abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]), abs(a[0] * b[1]) + abs(a[1] * b[0])]


def _skew(u):
    return [[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]


def rest_length(ops, Xa, Xb):
    e = _sub(Xb, Xa)
    return ops.sqrt(_dot(e, e))


def stretch(ops, X, x, r, E, project=True, magnitudes=False):
    """(energy, gradient[6], Hessian 6 x 6) of one segment X = (Xa, Xb), x = (xa, xb); project=False: the full Hessian (c = 1 - L / l unclamped)"""
    L = rest_length(ops, X[0], X[1])
    ks = E * ops.pi * r * r / L
    e = _sub(x[1], x[0])
    l = ops.sqrt(_dot(e, e))
    c = 1 - L / l
    if project and c < 0:
        c = 0 * c
    if magnitudes:
        em = [abs(x[1][i]) + abs(x[0][i]) for i in range(3)]
        dl = ops.sqrt(_dot(em, em)) + L
        t = [v / l for v in em]
        c = 1 + L / l
        B = [[ks * (t[i] * t[j] + c * ((1 if i == j else 0) + t[i] * t[j])) for j in range(3)] for i in range(3)]
        g = [ks * dl * v for v in t] * 2
        return ks * dl * dl / 2, g, [[B[i % 3][j % 3] for j in range(6)] for i in range(6)]
    dl = l - L
    t = [v / l for v in e]
    B = [[ks * (t[i] * t[j] + c * ((1 if i == j else 0) - t[i] * t[j])) for j in range(3)] for i in range(3)]
    g = [-ks * dl * v for v in t] + [ks * dl * v for v in t]
    H = [[(1 if (i < 3) == (j < 3) else -1) * B[i % 3][j % 3] for j in range(6)] for i in range(6)]
    return ks * dl * dl / 2, g, H


def curvature(ops, x, jacobian=False, magnitudes=False):
    """(|kb|^2, kb[3], J 3 x 9 or None) of the polyline x = (xa, xb, xc); |kb|^2 = +inf where d <= 0 (then kb and J are None)"""
    e0, e1 = _sub(x[1], x[0]), _sub(x[2], x[1])
    s0, s1 = _dot(e0, e0), _dot(e1, e1)
    p, q = ops.sqrt(s0 * s1), _dot(e0, e1)
    d = p + q
    if not d > 0:
        return ops.inf, None, None
    if magnitudes:
        e0m = [abs(x[1][i]) + abs(x[0][i]) for i in range(3)]
        e1m = [abs(x[2][i]) + abs(x[1][i]) for i in range(3)]
        pm, qm = ops.sqrt(_dot(e0m, e0m) * _dot(e1m, e1m)), _dot(e0m, e1m)
        kb = [2 * v / d for v in _cross_abs(e0m, e1m)]
        w0 = [ops.sqrt(_dot(e1m, e1m) / s0) * e0m[i] + e1m[i] for i in range(3)]
        w1 = [ops.sqrt(_dot(e0m, e0m) / s1) * e1m[i] + e0m[i] for i in range(3)]
        K0, K1 = [[abs(v) for v in row] for row in _skew(e0m)], [[abs(v) for v in row] for row in _skew(e1m)]
        D0 = [[(2 * K1[m][c] + kb[m] * w0[c]) / d for c in range(3)] for m in range(3)]
        D1 = [[(2 * K0[m][c] + kb[m] * w1[c]) / d for c in range(3)] for m in range(3)]
        J = [D0[m] + [D0[m][c] + D1[m][c] for c in range(3)] + D1[m] for m in range(3)]
        return 4 * (pm + qm) / d, kb, J
    k2 = 4 * max(p - q, 0 * p) / d  # (Cauchy-Schwarz: p >= q; the clamp only removes a rounding of a straight node)
    kb = [2 * v / d for v in _cross(e0, e1)]
    if not jacobian:
        return k2, kb, None
    w0 = [ops.sqrt(s1 / s0) * e0[i] + e1[i] for i in range(3)]
    w1 = [ops.sqrt(s0 / s1) * e1[i] + e0[i] for i in range(3)]
    K0, K1 = _skew(e0), _skew(e1)
    D0 = [[(-2 * K1[m][c] - kb[m] * w0[c]) / d for c in range(3)] for m in range(3)]
    D1 = [[(2 * K0[m][c] - kb[m] * w1[c]) / d for c in range(3)] for m in range(3)]
    J = [[-v for v in D0[m]] + [D0[m][c] - D1[m][c] for c in range(3)] + D1[m] for m in range(3)]
    return k2, kb, J


def bend_stiffness(ops, X, rE):
    """X: rest positions of (a, b, c); rE: ((r, E) of segment (a, b), the same of (b, c)) -> k_b = E_m pi r_m^4 / 4 / (L0 + L1)"""
    rm, Em = (rE[0][0] + rE[1][0]) / 2, (rE[0][1] + rE[1][1]) / 2
    return Em * ops.pi * rm ** 4 / 4 / (rest_length(ops, X[0], X[1]) + rest_length(ops, X[1], X[2]))


def bend(ops, X, x, rE, bendScale, magnitudes=False):
    """(energy, gradient[9], Gauss-Newton Hessian 9 x 9) of one bending triple; (+inf, None, None) at an exact fold"""
    k = bendScale * bend_stiffness(ops, X, rE)
    k2, kb, J = curvature(ops, x, True, magnitudes)
    if kb is None:
        return ops.inf, None, None
    g = [2 * k * sum(J[m][c] * kb[m] for m in range(3)) for c in range(9)]
    H = [[2 * k * sum(J[m][a] * J[m][b] for m in range(3)) for b in range(9)] for a in range(9)]
    return k * k2, g, H


def triples_of(seg, nV):
    """bending triples of a segment list, ascending by the interior node b: rows (a, b, c, segment of (a, b), segment of (b, c)); a the far node of the
    incident segment with the smaller index.  Nodes with one segment (ends) or three and more (junctions) have none."""
    inc = [[] for _ in range(nV)]
    for s, (a, b) in enumerate(np.asarray(seg).reshape(-1, 2).tolist()):
        inc[a].append((s, b))
        inc[b].append((s, a))
    return [(inc[b][0][1], b, inc[b][1][1], inc[b][0][0], inc[b][1][0]) for b in range(nV) if len(inc[b]) == 2]


def chain_reference(ops, case, X=None, x=None, magnitudes=False, parts=False):
    """E, g[3 n], dense H[3 n, 3 n] (clamped stretching + Gauss-Newton bending) of a set of segments, as lists of ops numbers; parts: also the per-segment
    and per-triple energies"""
    X = case["X"] if X is None else X
    x = case["x"] if x is None else x
    n = len(X)
    Xn = [[ops.num(v) for v in r] for r in X]
    xn = [[ops.num(v) for v in r] for r in x]
    seg = np.asarray(case["seg"]).reshape(-1, 2).tolist()
    mat = [(ops.num(case["r"][s]), ops.num(case["YM"][s])) for s in range(len(seg))]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    per = ([], [])

    def scatter(nodes, e, ge, He):
        nonlocal E
        E = E + e
        idx = [3 * v + i for v in nodes for i in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + ge[p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + He[p][q]

    for s, nodes in enumerate(seg):
        r = stretch(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], *mat[s], magnitudes=magnitudes)
        per[0].append(r[0])
        scatter(nodes, *r)
    if float(case["bendScale"]) > 0:
        for (a, b, c, s0, s1) in triples_of(seg, n):
            nodes = (a, b, c)
            r = bend(ops, [Xn[v] for v in nodes], [xn[v] for v in nodes], (mat[s0], mat[s1]), ops.num(case["bendScale"]), magnitudes)
            per[1].append(r[0])
            if r[1] is None:  # an exact fold: +inf energy, no derivative (the kernels write no gradient and no block there either)
                E = E + r[0]
                continue
            scatter(nodes, *r)
    return (E, g, H, per) if parts else (E, g, H)


def _f(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, (float, mpf)) else float(v)


def perturbed(A, seed):
    A = np.asarray(A, dtype=np.float64)
    s = np.random.default_rng(seed).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case):
    """reference, sens and scale of E, g, H of one case (float64 arrays; the differences are taken in mpmath)"""
    r = chain_reference(MP, case)
    sens = [0.0, np.zeros(3 * len(case["X"])), np.zeros((3 * len(case["X"]),) * 2)]
    for s in range(SENS_SAMPLES):
        p = chain_reference(MP, case, perturbed(case["X"], 2 * s + 1), perturbed(case["x"], 2 * s + 2))
        sens[0] = max(sens[0], float(abs(p[0] - r[0])))
        sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
        sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
    m = chain_reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2]}


def numpy_restatement(case):
    E, g, H = chain_reference(NP, case)
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


def _case(name, X, x, seg, r=0.002, YM=1e7, dbc=None, bendScale=1.0):
    X, x, seg = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(seg, dtype=np.int32).reshape(-1, 2)
    ns = len(seg)
    return {"name": name, "X": X, "x": x, "seg": seg, "r": np.broadcast_to(np.asarray(r, dtype=np.float64), (ns,)).copy(), "YM": np.full(ns, YM),
            "rho": np.full(ns, 1000.0), "dbc": np.zeros(len(X), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32), "bendScale": bendScale}


def elbow(angle_deg, l0=0.1, l1=0.16):
    """three nodes a - b - c with |ab| = l0, |bc| = l1 and the turning angle angle_deg at b (0 = straight), in a tilted plane"""
    t = np.radians(angle_deg)
    P = np.array([[-l0, 0.0, 0.0], [0.0, 0.0, 0.0], [l1 * np.cos(t), l1 * np.sin(t), 0.0]])
    return P @ rot([1, 2, 3], 50).T + [0.3, 0.1, -0.2]


def chain(n, spacing=0.1, axis=(1.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0)):
    """n nodes on a straight line, n - 1 segments (i, i + 1)"""
    V = np.asarray(origin, dtype=np.float64) + np.outer(np.arange(n) * spacing, np.asarray(axis, dtype=np.float64))
    return V, np.column_stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int32)


def ring(n, R):
    """n nodes on a circle of radius R in the plane z = 0, n segments (i, i + 1 mod n): every node is interior"""
    a = 2 * np.pi * np.arange(n) / n
    return np.column_stack([R * np.cos(a), R * np.sin(a), np.zeros(n)]), np.column_stack([np.arange(n), (np.arange(n) + 1) % n]).astype(np.int32)


def cases():
    rng = np.random.default_rng(11)
    S = np.array([[0.1, 0.2, 0.3], [0.25, 0.3, 0.2]])
    c = S.mean(axis=0)
    R = rot([1, 2, 3], 50)
    out = [_case("segment at rest", S, S, [[0, 1]]),
           _case("segment stretched", S, c + (S - c) * 1.2, [[0, 1]]),
           _case("segment compressed", S, c + (S - c) * 0.7, [[0, 1]]),
           _case("segment rotated", S, c + (S - c) @ R.T, [[0, 1]])]
    X3 = elbow(0)
    for ang in (0, 90, 170):
        out.append(_case(f"three nodes at {ang}", X3, elbow(ang, 0.1 if ang == 0 else 0.11, 0.16), [[0, 1], [1, 2]], r=[0.002, 0.003]))
    V, seg = chain(5, axis=(0.6, 0.0, 0.8), origin=(0.2, 0.5, -0.1))
    out.append(_case("five-node polyline, Dirichlet nodes", V, V + 0.02 * rng.standard_normal(V.shape), seg, r=[0.002, 0.002, 0.003, 0.003], dbc=[1, 0, 0, 2, 0]))
    hub = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [-0.05, 0.09, 0.0], [-0.05, -0.08, 0.03], [0.2, 0.01, 0.0]])
    out.append(_case("three-armed junction", hub, hub + 0.01 * rng.standard_normal(hub.shape), [[0, 1], [0, 2], [0, 3], [1, 4]]))
    V, seg = ring(6, 0.1)
    out.append(_case("closed six-node ring", V, V * [1.1, 0.9, 1.0] + 0.01 * rng.standard_normal(V.shape), seg))
    return out


def pack():
    cs = cases()
    out = {"names": np.array([c["name"] for c in cs])}
    for i, c in enumerate(cs):
        r = evaluate(c)
        for k in ("X", "x", "seg", "r", "YM", "rho", "dbc"):
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
