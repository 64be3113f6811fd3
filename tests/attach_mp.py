"""mpmath restatement of the attachment energy (ipc_amd/csrc/attach_kernels.h), its gradient and PSD Hessian; a project extension, so there is no oracle
to compare with -- this file is the reference, pinned by tests/test_attach_mp.py (mp.diff, mp.eigsy, rigid motions, the closed forms of a stitch).

An attachment ties point A to point B, each a convex combination of one to three nodes.  merge() restates the host plan: the distinct nodes with signed
coefficients c_i = weight in A - weight in B, zeros dropped.  With stiffness k and rest length L:
  d = sum_i c_i x_i, l = |d|, W = k (l - L)^2 / 2, grad_i = k (l - L) c_i t, t = d / l, H_ij = c_i c_j B, B = k [t t^T + max(0, 1 - L / l) (I - t t^T)]
  (the eigenvalue clamp at 0 in closed form: the full Hessian is (c c^T) (x) B_full).  L == 0: W = k |d|^2 / 2, grad_i = k c_i d, B = k I, also at d = 0.
  L > 0 and l == 0: W = k L^2 / 2, no force, no block.
The merged coefficients, k and L are the kernels' INPUTS: they enter mpmath as the float64 numbers they are.

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64): the float64 instance is the "NumPy restatement"
whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/rod_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  q with every term of its formula replaced by its magnitude (sum |c_i| |x_i| for d, |l| + |L| for l - L, 1 + L / l for the clamp factor, products of
         absolute values, sums over the attachments that share a node), the largest entry for the gradient and the Hessian: one number per case and quantity
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_attach_mp_golden.py --measure prints
         it), times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction --, rounded up to a power of two.
         test_attach_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_attach_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.063 (node - triangle point), gradient 0.268 (node - edge point), Hessian 0.099 (node - edge point)
NUMPY_WORST_RATIO = 0.268
M = 4.0  # 8 x 0.268 = 2.14 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attach_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    zero = mpf(0)


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    zero = 0.0


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def merge(nodesA, weightsA, nodesB, weightsB):
    """the host plan's merge of one attachment (attach_plan.cpp), in float64 and in its order: ([node ids], [signed coefficients]) in the order of first
    appearance (A's slots, then B's), zero coefficients dropped; slots with id -1 are unused"""
    ids, c = [], []
    for nodes, w, sign in ((nodesA, weightsA, 1.0), (nodesB, weightsB, -1.0)):
        for v, wv in zip(nodes, w):
            if int(v) == -1:
                continue
            if int(v) not in ids:
                ids.append(int(v))
                c.append(0.0)
            c[ids.index(int(v))] += sign * float(wv)
    keep = [j for j in range(len(ids)) if c[j] != 0.0]
    return [ids[j] for j in keep], [c[j] for j in keep]


def stencils(case):
    return [merge(case["nA"][i], case["wA"][i], case["nB"][i], case["wB"][i]) for i in range(len(case["k"]))]


def spring(ops, c, x, k, L, project=True, magnitudes=False):
    """(energy, gradient[3 m], Hessian 3 m x 3 m, length, force) of one attachment: c the m signed coefficients, x the m node positions (ops numbers);
    project=False: the full Hessian (1 - L / l unclamped).  gradient and Hessian are None where L > 0 and l == 0 (no direction: nothing is written)."""
    m = len(c)
    d = [sum(c[i] * x[i][a] for i in range(m)) for a in range(3)]
    l = ops.sqrt(_dot(d, d))
    if magnitudes:
        ca = [abs(v) for v in c]
        dm = [sum(ca[i] * abs(x[i][a]) for i in range(m)) for a in range(3)]
        if L == 0:
            B = [[k * (1 if a == b else 0) for b in range(3)] for a in range(3)]
            g = [k * ca[i] * dm[a] for i in range(m) for a in range(3)]
            E = k * _dot(dm, dm) / 2
        else:
            dl = ops.sqrt(_dot(dm, dm)) + L
            E = k * dl * dl / 2
            if not l > 0:
                return E, None, None, l, k * (l + L)
            t = [v / l for v in dm]
            cf = 1 + L / l
            B = [[k * (t[a] * t[b] + cf * ((1 if a == b else 0) + t[a] * t[b])) for b in range(3)] for a in range(3)]
            g = [k * dl * ca[i] * t[a] for i in range(m) for a in range(3)]
        H = [[ca[i] * ca[j] * B[a][b] for j in range(m) for b in range(3)] for i in range(m) for a in range(3)]
        return E, g, H, l, k * (l + L)
    if L == 0:  # a stitch: no square root, no division
        B = [[k * (1 if a == b else 0) for b in range(3)] for a in range(3)]
        g = [k * c[i] * d[a] for i in range(m) for a in range(3)]
        E = k * _dot(d, d) / 2
    else:
        dl = l - L
        E = k * dl * dl / 2
        if not l > 0:
            return E, None, None, l, k * dl
        t = [v / l for v in d]
        cf = 1 - L / l
        if project and cf < 0:
            cf = 0 * cf
        B = [[k * (t[a] * t[b] + cf * ((1 if a == b else 0) - t[a] * t[b])) for b in range(3)] for a in range(3)]
        g = [k * dl * c[i] * t[a] for i in range(m) for a in range(3)]
    H = [[c[i] * c[j] * B[a][b] for j in range(m) for b in range(3)] for i in range(m) for a in range(3)]
    return E, g, H, l, k * (l - L)


def reference(ops, case, x=None, magnitudes=False, project=True, parts=False):
    """E, g[3 n], dense H[3 n, 3 n] of the attachments of a case, as lists of ops numbers; parts: also the per-attachment energies, lengths and forces"""
    x = case["x"] if x is None else x
    n = len(x)
    xn = [[ops.num(v) for v in r] for r in x]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    per = ([], [], [])
    for i, (ids, c) in enumerate(stencils(case)):
        r = spring(ops, [ops.num(v) for v in c], [xn[v] for v in ids], ops.num(case["k"][i]), ops.num(case["L"][i]), project, magnitudes)
        E = E + r[0]
        per[0].append(r[0])
        per[1].append(r[3])
        per[2].append(r[4])
        if r[1] is None:
            continue
        idx = [3 * v + a for v in ids for a in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + r[1][p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + r[2][p][q]
    return (E, g, H, per) if parts else (E, g, H)


def _f(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, (float, mpf)) else float(v)


def perturbed(A, seed):
    A = np.asarray(A, dtype=np.float64)
    s = np.random.default_rng(seed).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case):
    """reference, sens and scale of E, g, H of one case, the lengths and forces (float64 arrays; the differences are taken in mpmath)"""
    r = reference(MP, case, parts=True)
    n3 = 3 * len(case["x"])
    sens = [0.0, np.zeros(n3), np.zeros((n3, n3))]
    for s in range(SENS_SAMPLES):
        p = reference(MP, case, perturbed(case["x"], s + 1))
        sens[0] = max(sens[0], float(abs(p[0] - r[0])))
        sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
        sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
    m = reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2], "perE": _f(r[3][0]), "len": _f(r[3][1]), "force": _f(r[3][2])}


def numpy_restatement(case):
    E, g, H = reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64)}


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (coincident points with a rest length write nothing: exact zeros are expected) 0 for no
    error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def _pt(*pairs):
    """a point from (node, weight) pairs -> (3 ids padded with -1, 3 weights padded with 0)"""
    ids = [p[0] for p in pairs] + [-1] * (3 - len(pairs))
    w = [float(p[1]) for p in pairs] + [0.0] * (3 - len(pairs))
    return ids, w


def _case(name, x, att, dbc=None):
    """att: [(point A, point B, k, L)] with the points from _pt"""
    x = np.asarray(x, dtype=np.float64)
    return {"name": name, "x": x, "nA": np.array([a[0][0] for a in att], dtype=np.int32), "wA": np.array([a[0][1] for a in att], dtype=np.float64),
            "nB": np.array([a[1][0] for a in att], dtype=np.int32), "wB": np.array([a[1][1] for a in att], dtype=np.float64),
            "k": np.array([a[2] for a in att], dtype=np.float64), "L": np.array([a[3] for a in att], dtype=np.float64),
            "dbc": np.zeros(len(x), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32)}


def cases():
    rng = np.random.default_rng(23)
    u = np.array([0.6, 0.0, 0.8])  # a unit vector with exact squares' sum
    P = lambda n: 0.2 + 0.3 * rng.random((n, 3))
    a0 = np.array([0.1, 0.2, 0.3])
    tri = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.05], [0.05, 0.25, 0.0]])
    out = [_case("node - node, stitch", [a0, a0 + [0.03, -0.02, 0.05]], [(_pt((0, 1)), _pt((1, 1)), 500.0, 0.0)]),
           _case("node - node, stretched", [a0, a0 + 0.15 * u], [(_pt((0, 1)), _pt((1, 1)), 300.0, 0.1)]),
           _case("node - node, compressed", [a0, a0 + 0.07 * u], [(_pt((0, 1)), _pt((1, 1)), 300.0, 0.1)]),
           _case("coincident points with a rest length", [a0, a0], [(_pt((0, 1)), _pt((1, 1)), 300.0, 0.1)]),
           _case("coincident points, stitch", [a0, a0], [(_pt((0, 1)), _pt((1, 1)), 500.0, 0.0)]),
           _case("node - edge point", np.vstack([[[0.05, 0.1, 0.12]], tri[:2] + 0.3]), [(_pt((0, 1)), _pt((1, 0.3), (2, 0.7)), 200.0, 0.05)]),
           _case("node - triangle point", np.vstack([tri + 0.1, [[0.2, 0.2, 0.2]]]), [(_pt((3, 1)), _pt((0, 0.2), (1, 0.3), (2, 0.5)), 800.0, 0.0)]),
           _case("edge point - triangle point", np.vstack([P(2), tri + 0.4]), [(_pt((0, 0.25), (1, 0.75)), _pt((2, 0.5), (3, 0.125), (4, 0.375)), 150.0, 0.02)]),
           _case("triangle point - triangle point", np.vstack([tri + 0.1, tri[::-1] * 1.1 + [0.1, 0.1, 0.17]]),
                 [(_pt((0, 0.3), (1, 0.3), (2, 0.4)), _pt((3, 0.6), (4, 0.1), (5, 0.3)), 400.0, 0.0)]),
           _case("one node in both points", P(3), [(_pt((0, 0.5), (1, 0.5)), _pt((1, 0.25), (2, 0.75)), 250.0, 0.03)]),
           _case("node ids descending", P(4), [(_pt((3, 1)), _pt((2, 0.5), (0, 0.5)), 350.0, 0.04), (_pt((3, 0.5), (1, 0.5)), _pt((0, 1)), 120.0, 0.0)]),
           _case("Dirichlet nodes", P(4), [(_pt((0, 0.5), (1, 0.5)), _pt((2, 0.4), (3, 0.6)), 600.0, 0.05), (_pt((1, 1)), _pt((2, 1)), 90.0, 0.0)], dbc=[1, 0, 2, 0]),
           _case("coordinates offset by 1e3", np.array([a0, a0 + 0.12 * u, a0 + [0.01, 0.02, -0.03]]) + 1e3,
                 [(_pt((0, 1)), _pt((1, 1)), 300.0, 0.1), (_pt((0, 1)), _pt((2, 1)), 500.0, 0.0)])]
    return out


INPUTS = ("x", "nA", "wA", "nB", "wB", "k", "L", "dbc")


def pack():
    cs = cases()
    out = {"names": np.array([c["name"] for c in cs])}
    for i, c in enumerate(cs):
        r = evaluate(c)
        for k in INPUTS:
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
        ref[proj, :] = 0.0
        ref[:, proj] = 0.0
    return ref, tol
