"""mpmath restatement of the pressure-chamber energy (ipc_amd/csrc/chamber_kernels.h), its gradient and per-triangle PSD Hessian; a project extension, so
there is no oracle to compare with -- this file is the reference, pinned by tests/test_chamber_mp.py (mp.diff, mp.eigsy, rigid motions, closed surfaces).

A chamber is a closed, outward-oriented triangle list with the gauge pressure p and the reference point r.  With y_i = x_i - r, per triangle:
  W_t = -(p / 6) y0 . (y1 x y2);  dW/dx0 = -(p/6) y1 x y2, dW/dx1 = -(p/6) y2 x y0, dW/dx2 = -(p/6) y0 x y1;
  Hessian 9 x 9: zero diagonal blocks, H01 = (p/6) [y2]x, H02 = -(p/6) [y1]x, H12 = (p/6) [y0]x, projected to PSD per triangle.
p and r are the kernels' INPUTS: they enter mpmath as the float64 numbers they are.  r is the rest reference point of the host plan (ref_point below
restates its summation order to the bit); the cases' rest positions are their current ones.

Every formula below is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits, projection by mp.eigsy; NP: float64, projection by the cyclic
Jacobi iteration of jacobi9_device.h in its order and with its stopping rule): the float64 instance is the "NumPy restatement" whose recorded error sizes
the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as tests/attach_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns
  scale  q with every term of its formula replaced by its magnitude (|x - r| for y -- one subtraction, rounded once relative to its result --, products
         of absolute values, sums over the triangles that share a node), the largest entry for the gradient and the Hessian: one number per case and quantity.  For the projected Hessian of a triangle the
         magnitude of every entry is the Frobenius norm of the magnitudes of the unprojected block: the projection onto the PSD cone is 1-Lipschitz in
         that norm, so an error of the block passes through it no larger, and the eigen-iteration's own error is relative to that norm.
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_chamber_mp_golden.py --measure
         prints it), times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction, the hardware reciprocal and
         square-root estimates inside the rotations --, rounded up to a power of two.  test_chamber_mp.py::test_numpy_restatement_meets_the_tolerance
         pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_chamber_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.696 (two cubes in one chamber), gradient 0.502 (Dirichlet nodes), Hessian 1.463 (cube)
NUMPY_WORST_RATIO = 1.463
M = 16.0  # 8 x 1.463 = 11.7 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chamber_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H")


def _jacobi_psd(H):
    """V max(lambda, 0) V^T of a symmetric 9 x 9 list of floats by the cyclic Jacobi iteration of jacobi9_device.h (host branch): the rotations (P, Q)
    row by row, t = sgn(a) b / (|a| + sqrt(a^2 + b^2)) with a = (aqq - app) / 2 and b = apq, until off^2 <= 1e-28 diag^2"""
    n = len(H)
    W = [list(map(float, r)) for r in H]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(60):
        off = sum(2.0 * W[i][j] * W[i][j] for j in range(n) for i in range(j))
        dg = sum(W[i][i] * W[i][i] for i in range(n))
        if off <= 1e-28 * dg or off == 0.0:
            break
        for P in range(n - 1):
            for Q in range(P + 1, n):
                apq = W[P][Q]
                if apq == 0.0:
                    continue
                app, aqq = W[P][P], W[Q][Q]
                a = 0.5 * (aqq - app)
                t = (apq if a >= 0 else -apq) / (abs(a) + math.sqrt(a * a + apq * apq))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    if k != P and k != Q:
                        wp, wq = W[k][P], W[k][Q]
                        W[k][P] = W[P][k] = c * wp - s * wq
                        W[k][Q] = W[Q][k] = s * wp + c * wq
                    vp, vq = V[k][P], V[k][Q]
                    V[k][P], V[k][Q] = c * vp - s * vq, s * vp + c * vq
                W[P][P], W[Q][Q] = app - t * apq, aqq + t * apq
                W[P][Q] = W[Q][P] = 0.0
    ev = [W[i][i] if W[i][i] > 0.0 else 0.0 for i in range(n)]
    return [[sum(V[i][k] * ev[k] * V[j][k] for k in range(n)) for j in range(n)] for i in range(n)]


def _eigsy_psd(H):
    n = len(H)
    E, Q = mp.eigsy(mp.matrix(H))
    ev = [E[k] if E[k] > 0 else mpf(0) for k in range(n)]
    return [[sum(Q[i, k] * ev[k] * Q[j, k] for k in range(n)) for j in range(n)] for i in range(n)]


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    psd = staticmethod(_eigsy_psd)
    zero = mpf(0)


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    psd = staticmethod(_jacobi_psd)
    zero = 0.0


def _cross(a, b, mag=False):
    if mag:
        return [a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]]
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _skew(s, w, zero, mag=False):
    m = 1 if mag else -1
    return [[zero, m * s * w[2], s * w[1]], [s * w[2], zero, m * s * w[0]], [m * s * w[1], s * w[0], zero]]


def triangle(ops, x, r, p, project=True, magnitudes=False):
    """(energy, gradient[9], Hessian 9 x 9) of one triangle: x its three node positions, r the reference point, p the pressure (ops numbers)"""
    if magnitudes:
        y = [[abs(x[k][a] - r[a]) for a in range(3)] for k in range(3)]
        s = abs(p) / 6
    else:
        y = [[x[k][a] - r[a] for a in range(3)] for k in range(3)]
        s = p / 6
    c12, c20, c01 = _cross(y[1], y[2], magnitudes), _cross(y[2], y[0], magnitudes), _cross(y[0], y[1], magnitudes)
    sg = s if magnitudes else -s
    E = sg * _dot(y[0], c12)
    g = [sg * v for v in c12 + c20 + c01]
    H = [[ops.zero] * 9 for _ in range(9)]
    for (I, J), B in (((0, 1), _skew(s, y[2], ops.zero, magnitudes)), ((0, 2), _skew(s if magnitudes else -s, y[1], ops.zero, magnitudes)),
                      ((1, 2), _skew(s, y[0], ops.zero, magnitudes))):
        for a in range(3):
            for b in range(3):
                H[3 * I + a][3 * J + b] = B[a][b]
                H[3 * J + b][3 * I + a] = B[a][b]
    if magnitudes:
        f = ops.sqrt(sum(v * v for row in H for v in row))
        H = [[f] * 9 for _ in range(9)]
    elif project and p != 0:
        H = ops.psd(H)
    return E, g, H


def reference(ops, case, x=None, magnitudes=False, project=True, parts=False):
    """E, g[3 n], dense H[3 n, 3 n] of the chamber of a case, as lists of ops numbers; parts: also the per-triangle energies"""
    x = case["x"] if x is None else x
    n = len(x)
    xn = [[ops.num(v) for v in row] for row in x]
    r, p = [ops.num(v) for v in case["r"]], ops.num(case["p"])
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    per = []
    for t in case["tri"]:
        ids = [int(v) for v in t]
        e, gt, Ht = triangle(ops, [xn[v] for v in ids], r, p, project, magnitudes)
        E = E + e
        per.append(e)
        if float(case["p"]) == 0.0 and not magnitudes:
            continue
        idx = [3 * v + a for v in ids for a in range(3)]
        for i, P in enumerate(idx):
            g[P] = g[P] + gt[i]
            for j, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + Ht[i][j]
    return (E, g, H, per) if parts else (E, g, H)


def ref_point(x, tri):
    """the host plan's reference point (chamber_plan.h) in float64 and in its order: (sum_t ((x0 + x1) + x2)) / (3 m), one accumulator per axis"""
    S = [0.0, 0.0, 0.0]
    for t in tri:
        for a in range(3):
            S[a] += (float(x[t[0]][a]) + float(x[t[1]][a])) + float(x[t[2]][a])
    return np.array([S[a] / (3.0 * len(tri)) for a in range(3)])


def rest_volume(x, tri, r):
    """the host plan's rest volume in float64 and in its order"""
    V6 = 0.0
    for t in tri:
        y = [[float(x[v][a]) - float(r[a]) for a in range(3)] for v in t]
        V6 += (y[0][0] * (y[1][1] * y[2][2] - y[1][2] * y[2][1]) + y[0][1] * (y[1][2] * y[2][0] - y[1][0] * y[2][2])) + y[0][2] * (y[1][0] * y[2][1] - y[1][1] * y[2][0])
    return V6 / 6.0


def volume_area(case, x=None, r=None):
    """(V, A, sum_t |y0| |y1| |y2|, sum_t (|y0| + |y1| + |y2|)^2) of the chamber of a case in mpmath; V about r (default: the case's)"""
    x = case["x"] if x is None else x
    r = [mpf(float(v)) for v in (case["r"] if r is None else r)]
    V = A = m3 = m2 = mpf(0)
    for t in case["tri"]:
        y = [[mpf(float(x[int(v)][a])) - r[a] for a in range(3)] for v in t]
        V += _dot(y[0], _cross(y[1], y[2])) / 6
        nrm = _cross([y[1][a] - y[0][a] for a in range(3)], [y[2][a] - y[0][a] for a in range(3)])
        A += mp.sqrt(_dot(nrm, nrm)) / 2
        l = [mp.sqrt(_dot(v, v)) for v in y]
        m3 += l[0] * l[1] * l[2]
        m2 += (l[0] + l[1] + l[2]) ** 2
    return V, A, m3, m2


def triangle_eigenvalues(case):
    """per triangle the 9 eigenvalues of its unprojected Hessian (mpmath), as float64 rows"""
    out = []
    r, p = [mpf(float(v)) for v in case["r"]], mpf(float(case["p"]))
    for t in case["tri"]:
        H = triangle(MP, [[mpf(float(v)) for v in case["x"][int(i)]] for i in t], r, p, project=False)[2]
        out.append([float(v) for v in mp.eigsy(mp.matrix(H), eigvals_only=True)])
    return np.array(out)


def _f(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, (float, mpf)) else float(v)


def perturbed(A, seed):
    A = np.asarray(A, dtype=np.float64)
    s = np.random.default_rng(seed).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case):
    """reference, sens and scale of E, g, H of one case, the per-triangle energies, the volume and the area (float64; the differences are taken in mpmath)"""
    r = reference(MP, case, parts=True)
    n3 = 3 * len(case["x"])
    sens = [0.0, np.zeros(n3), np.zeros((n3, n3))]
    for s in range(SENS_SAMPLES):
        q = reference(MP, case, perturbed(case["x"], s + 1))
        sens[0] = max(sens[0], float(abs(q[0] - r[0])))
        sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(q[1], r[1])]))
        sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(q[2], r[2])]))
    m = reference(MP, case, magnitudes=True)
    scale = (float(m[0]), float(max(m[1])), float(max(max(row) for row in m[2])))
    V, A, m3, m2 = volume_area(case)
    return {"E": float(r[0]), "g": _f(r[1]), "H": _f(r[2]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2], "scale_E": scale[0], "scale_g": scale[1],
            "scale_H": scale[2], "perE": _f(r[3]), "vol": float(V), "area": float(A), "volMag": float(m3), "areaMag": float(m2)}


def numpy_restatement(case):
    E, g, H = reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64)}


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (p = 0 writes nothing: exact zeros are expected) 0 for no error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
CUBE_X = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
# outward by the right-hand rule
CUBE_TRI = np.array([[0, 3, 2], [0, 2, 1], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 7, 6], [3, 6, 2], [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]], dtype=np.int32)
TET_X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
TET_TRI = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def _case(name, x, tri, p, dbc=None):
    x = np.asarray(x, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int32)
    return {"name": name, "x": x, "tri": tri, "p": np.float64(p), "r": ref_point(x, tri),
            "dbc": np.zeros(len(x), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32)}


def cases():
    rng = np.random.default_rng(31)
    J = lambda n, s=0.05: s * (rng.random((n, 3)) - 0.5)  # a jitter: no face stays planar, no eigenvalue pair stays degenerate by symmetry
    cube = lambda size, lo: CUBE_X * size + np.asarray(lo, dtype=np.float64) + J(8, 0.05 * size)
    two = np.vstack([cube(0.2, [0.1, 0.1, 0.1]), cube(0.15, [0.44, 0.18, 0.16])])
    return [_case("tetrahedron", TET_X * 0.3 + [0.2, 0.1, 0.15] + J(4, 0.02), TET_TRI, 800.0),
            _case("cube", cube(0.25, [0.1, 0.2, 0.3]), CUBE_TRI, 1500.0),
            _case("cube far from the origin", cube(0.25, [0.1, 0.2, 0.3]) + [250.0, -250.0, 250.0], CUBE_TRI, 1500.0),
            _case("negative pressure", cube(0.2, [0.3, 0.1, 0.2]), CUBE_TRI, -2500.0),
            _case("zero pressure", cube(0.2, [0.2, 0.2, 0.1]), CUBE_TRI, 0.0),
            _case("Dirichlet nodes", cube(0.3, [0.1, 0.1, 0.2]), CUBE_TRI, 1200.0, dbc=[1, 0, 2, 0, 0, 0, 0, 0]),
            _case("two cubes in one chamber", two, np.vstack([CUBE_TRI, CUBE_TRI + 8]), 900.0)]


INPUTS = ("x", "tri", "p", "r", "dbc")


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
        for k in ("E", "sens_E", "scale_E", "scale_g", "scale_H", "p", "vol", "area", "volMag", "areaMag"):
            c[k] = float(c[k])
        res.append(c)
    return res


def expected(case, k, coef=1.0, projectDBC=True):
    """(reference, tolerance) of quantity k at `coef`; gradient entries, rows and columns of projected Dirichlet nodes dropped (type 1 always, 2 with projectDBC)"""
    ref, tol = coef * np.array(case[k], dtype=np.float64), np.array(tolerance(case, k, coef), dtype=np.float64)
    if k == "E":
        return float(ref), float(tol)
    if case["p"] == 0.0:
        tol = np.zeros_like(ref)  # nothing is written: exact zeros
    proj = np.repeat((case["dbc"] == 1) | ((case["dbc"] == 2) & bool(projectDBC)), 3)
    ref[proj] = 0.0
    if k == "H":
        ref[proj, :] = 0.0
        ref[:, proj] = 0.0
    return ref, tol
