"""mpmath restatement of the fibre energy of tetrahedral elements (ipc_amd/csrc/fiber_kernels.h), its gradient and its Hessian, unclamped and clamped; a
project extension, so there is no oracle to compare with -- this file is the reference, pinned by tests/test_fiber_mp.py (mp.diff, mp.eigsy, rigid rotations).

Per fibred tetrahedron with b = A_t a (A_t = restTriInv, a the unit rest direction), c = (-(b1 + b2 + b3), b1, b2, b3), rest volume vol:
  d = sum_i c_i x_i, l = |d|, t = d / l, W = vol psi(l), grad_i = vol psi' c_i t, H_ij = c_i c_j B, B = vol [max(0, psi'') t t^T + max(0, psi' / l) (I - t t^T)]
  law 0 (spring): psi = k (l - l0)^2 / 2, l0 = 1 - act; tension only: 0 for l <= l0.     law 1 (exp): psi = k / (2 k2) (exp(k2 (l^2 - 1)^2) - 1) for l > 1, else 0.
  l == 0: W = vol psi(0), no force, no block.
b, vol k, k2 and l0 are the kernels' INPUTS: they enter mpmath as the float64 numbers they are (rest_inputs() restates the host plan's b = A a in its
order of operations; the GPU tests take A and vol from the context instead).  c_0 is the exact -(b1 + b2 + b3) here.

Every formula is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64); the float64 instance is the "NumPy restatement".

Tolerance of a quantity q (energy, gradient, dense Hessian) of one element or one assembled case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  -- the form
of tests/attach_mp.py, and its M = 4 (the attachment is the closest term: the same d = sum c_i x_i, the same clamp, the same atomic scatter).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every current coordinate moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns.  It
         also carries a law that switches within an ulp (the tension-only threshold).
  scale  the first-order rounding magnitude of q: d is evaluated as sum b_i (x_i - x_0), so d_m = sum |b_i| |x_i - x_0| and u l_m, l_m = |d_m|, bounds the
         rounding of l; that error and u times the magnitude of every rounded intermediate travel through the law by the chain rule (law(..., lm): l_m + l0
         for l - l0; 2 l l_m + l^2 + 1 for I = l^2 - 1; 2 k2 |I| I_m + q for q = k2 I^2; e (1 + q_m) for e = exp(q): its own rounding plus that of its
         argument); gradient and blocks are products of these magnitudes with |c_i| (|c_0| = |b1| + |b2| + |b3|) and t_m = d_m / l, summed over the elements that
         share a node; the largest entry for the gradient and the Hessian.  Zero where the law is off: exact zeros are expected there.
None of it is tuned to a GPU result; test_fiber_mp.py::test_numpy_restatement_meets_the_tolerance checks the float64 restatement against it.
"""
import functools
import math

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
M = 4.0  # tests/attach_mp.py
SENS_SAMPLES = 4
DBL_MAX = 1.7976931348623157e308
SPRING, EXP = 0, 1


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    exp = staticmethod(mp.exp)
    expm1 = staticmethod(mp.expm1)
    zero = mpf(0)


def _np_exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    exp = staticmethod(_np_exp)
    expm1 = staticmethod(lambda v: math.expm1(v) if v < 709.0 else math.inf)
    zero = 0.0


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def law(ops, l, vk, k2, kind, tension_only, l0, lm=None):
    """(W, d1, d2) = vol (psi, psi', psi'')(l); zeros where the law is off.  With lm (the magnitude sum behind l, so that u lm bounds the rounding of l): the
    first-order error magnitudes of the three instead -- every rounded operation contributes u times the magnitude of its result, the error of l travels
    through the chain rule"""
    z = ops.zero
    if kind == EXP:
        if not l > 1:
            return z, z, z
        I = l * l - 1
        q = k2 * I * I
        e = ops.exp(q)
        if lm is None:
            return vk / (2 * k2) * ops.expm1(q), vk * 2 * l * I * e, vk * e * (2 * I + 4 * l * l + 8 * q * l * l)
        Im = 2 * l * lm + l * l + 1  # I = l^2 - 1
        qm = 2 * k2 * I * Im + q  # q = k2 I^2
        em = e * (1 + qm)
        return (vk / (2 * k2) * (e * qm + ops.expm1(q)), vk * 2 * (lm * I * e + l * Im * e + l * I * em),
                vk * (em * (2 * I + 4 * l * l + 8 * q * l * l) + e * (2 * Im + 8 * l * lm + 8 * qm * l * l + 16 * q * l * lm)))
    dl = l - l0
    if tension_only and not dl > 0:
        return z, z, z
    if lm is None:
        return vk * dl * dl / 2, vk * dl, vk + z
    dlm = lm + l0
    return vk * (abs(dl) * dlm + dl * dl / 2), vk * dlm, vk + z


def element(ops, b, x, vk, k2, kind, tension_only, l0, project=True, magnitudes=False):
    """(W, gradient[12] or None, Hessian 12 x 12 or None, l, d1) of one element: b the 3 coefficients, x the 4 node positions (ops numbers).  project=False: the
    full Hessian.  gradient and Hessian are None where l == 0 (no direction) and where the law is off (psi' = psi'' = 0): nothing is written.
    d = sum c_i x_i is evaluated as b1 (x1 - x0) + b2 (x2 - x0) + b3 (x3 - x0), as the kernels do (the same sum; exact under a translation)."""
    c = [-(b[0] + b[1] + b[2]), b[0], b[1], b[2]]
    d = [sum(b[i] * (x[i + 1][a] - x[0][a]) for i in range(3)) for a in range(3)]
    l = ops.sqrt(_dot(d, d))
    if magnitudes:
        ca = [abs(b[0]) + abs(b[1]) + abs(b[2]), abs(b[0]), abs(b[1]), abs(b[2])]
        dm = [sum(ca[i + 1] * abs(x[i + 1][a] - x[0][a]) for i in range(3)) for a in range(3)]
        lm = ops.sqrt(_dot(dm, dm))
        W, d1, d2 = law(ops, l, vk, k2, kind, tension_only, l0, lm)
        if not l > 0 or (d1 == 0 and d2 == 0):
            return W, None, None, l, d1
        t = [v / l for v in dm]
        kc = d1 / l + abs(law(ops, l, vk, k2, kind, tension_only, l0)[1]) * lm / (l * l)
        B = [[d2 * t[p] * t[q] + kc * ((1 if p == q else 0) + t[p] * t[q]) for q in range(3)] for p in range(3)]
        g = [d1 * ca[i] * t[p] for i in range(4) for p in range(3)]
        H = [[ca[i] * ca[j] * B[p][q] for j in range(4) for q in range(3)] for i in range(4) for p in range(3)]
        return W, g, H, l, d1
    W, d1, d2 = law(ops, l, vk, k2, kind, tension_only, l0)
    if not l > 0 or (d1 == 0 and d2 == 0):
        return W, None, None, l, d1
    t = [v / l for v in d]
    kc, kt = d1 / l, d2
    if project:
        kc = kc if kc > 0 else 0 * kc
        kt = kt if kt > 0 else 0 * kt
    B = [[kt * t[p] * t[q] + kc * ((1 if p == q else 0) - t[p] * t[q]) for q in range(3)] for p in range(3)]
    g = [d1 * c[i] * t[p] for i in range(4) for p in range(3)]
    H = [[c[i] * c[j] * B[p][q] for j in range(4) for q in range(3)] for i in range(4) for p in range(3)]
    return W, g, H, l, d1


def reference(ops, case, x=None, magnitudes=False, project=True):
    """(E, g[3 n], dense H[3 n][3 n], per-element W, per-element l) of the fibred elements of a case (the `elems` records), lists of ops numbers"""
    x = case["x"] if x is None else x
    n = len(x)
    xn = [[ops.num(v) for v in r] for r in x]
    E = ops.zero
    g = [ops.zero] * (3 * n)
    H = [[ops.zero] * (3 * n) for _ in range(3 * n)]
    perW, perL = [], []
    for el in case["elems"]:
        r = element(ops, [ops.num(v) for v in el["b"]], [xn[v] for v in el["nodes"]], ops.num(el["vk"]), ops.num(el["k2"]), el["law"], el["tension_only"],
                    ops.num(el["l0"]), project, magnitudes)
        E = E + r[0]
        perW.append(r[0])
        perL.append(r[3])
        if r[1] is None:
            continue
        idx = [3 * int(v) + a for v in el["nodes"] for a in range(3)]
        for p, P in enumerate(idx):
            g[P] = g[P] + r[1][p]
            for q, Q in enumerate(idx):
                H[P][Q] = H[P][Q] + r[2][p][q]
    return E, g, H, perW, perL


def _f(v):
    def one(q):
        return float(q) if abs(q) <= DBL_MAX else (math.inf if q > 0 else -math.inf)
    if isinstance(v, (float, mpf)):
        return one(v)
    a = np.array(v, dtype=object)
    return np.vectorize(one, otypes=[np.float64])(a) if a.size else np.zeros(a.shape)


def perturbed(A, seed):
    A = np.asarray(A, dtype=np.float64)
    s = np.random.default_rng(seed).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case):
    """reference, sens and scale of E, g, H of one case, the per-element energies and stretches (float64; the differences are taken in mpmath)"""
    r = reference(MP, case)
    n3 = 3 * len(case["x"])
    sens = [0.0, np.zeros(n3), np.zeros((n3, n3)), np.zeros(len(case["elems"])), np.zeros(len(case["elems"]))]
    for s in range(SENS_SAMPLES):
        p = reference(MP, case, perturbed(case["x"], s + 1))
        sens[0] = max(sens[0], _f(abs(p[0] - r[0])))
        sens[1] = np.maximum(sens[1], _f([abs(a - b) for a, b in zip(p[1], r[1])]))
        sens[2] = np.maximum(sens[2], _f([[abs(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(p[2], r[2])]))
        sens[3] = np.maximum(sens[3], _f([abs(a - b) for a, b in zip(p[3], r[3])]))
        sens[4] = np.maximum(sens[4], _f([abs(a - b) for a, b in zip(p[4], r[4])]))
    m = reference(MP, case, magnitudes=True)
    return {"E": _f(r[0]), "g": _f(r[1]), "H": _f(r[2]), "perW": _f(r[3]), "len": _f(r[4]), "sens_E": sens[0], "sens_g": sens[1], "sens_H": sens[2],
            "sens_perW": sens[3], "sens_len": sens[4], "scale_E": _f(m[0]), "scale_g": _f(max(m[1])), "scale_H": _f(max(max(row) for row in m[2])), "scale_perW": _f(m[3])}


def numpy_restatement(case):
    E, g, H, perW, _ = reference(NP, case)
    return {"E": float(E), "g": np.array(g, dtype=np.float64), "H": np.array(H, dtype=np.float64), "perW": np.array(perW, dtype=np.float64)}


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (the law is off, or l == 0: exact zeros are expected) 0 for no error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * np.asarray(ref["scale_" + k]))


def expected(case, ref, k, coef=1.0, projectDBC=True):
    """(reference, tolerance) of quantity k at `coef`; gradient entries, rows and columns of projected Dirichlet nodes dropped (type 1 always, 2 with projectDBC)"""
    val, tol = coef * np.array(ref[k], dtype=np.float64), np.array(tolerance(ref, k, coef), dtype=np.float64)
    if k in ("E", "perW"):
        return val, tol
    dbc = np.asarray(case.get("dbc", np.zeros(len(case["x"]), dtype=np.int32)))
    proj = np.repeat((dbc == 1) | ((dbc == 2) & bool(projectDBC)), 3)
    val[proj] = 0.0
    if k == "H":
        val[proj, :] = 0.0
        val[:, proj] = 0.0
    return val, tol


# ---- the rest-shape inputs, as the host plan computes them ------------------------------------------------------------------------------------------
def b_from(A9, a):
    """b = A a in the plan's order of operations (fiber_plan.cpp: ((0 + A_r0 a_0) + A_r1 a_1) + A_r2 a_2, no contraction); A9 column-major"""
    A9, a = [float(v) for v in A9], [float(v) for v in a]
    return np.array([((0.0 + A9[r] * a[0]) + A9[r + 3] * a[1]) + A9[r + 6] * a[2] for r in range(3)])


def unit(a):
    """the plan's normalisation: scaled by the largest magnitude first"""
    a = [float(v) for v in a]
    s = max(abs(v) for v in a)
    x, y, z = a[0] / s, a[1] / s, a[2] / s
    n = math.sqrt(x * x + y * y + z * z)
    return np.array([x / n, y / n, z / n])


def rest_inputs(X, tet):
    """(A9 column-major, vol) of one rest tetrahedron in float64 (numpy's inverse: an INPUT of the reference, as the context's restTriInv is on the GPU)"""
    X = np.asarray(X, dtype=np.float64)
    Dm = np.column_stack([X[tet[1]] - X[tet[0]], X[tet[2]] - X[tet[0]], X[tet[3]] - X[tet[0]]])
    return np.linalg.inv(Dm).flatten(order="F"), abs(np.linalg.det(Dm)) / 6.0


def elem_record(A9, vol, nodes, a, k, kind=SPRING, k2=0.0, tension_only=False, act=0.0):
    return {"b": b_from(A9, unit(a)), "vk": float(vol) * float(k), "k2": float(k2) if kind == EXP else 0.0, "law": kind,
            "tension_only": bool(tension_only) and kind == SPRING, "l0": 1.0 - float(act), "nodes": [int(v) for v in nodes]}


# ---- cases: one tetrahedron each -----------------------------------------------------------------------------------------------------------------
def _R(axis, deg):
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return c * np.eye(3) + s * K + (1 - c) * np.outer(ax, ax)


OBLIQUE = _R([1.0, 2.0, -0.5], 37.0)
REG = np.array([[0.0, 0.0, 0.0], [0.1, 0.01, 0.0], [0.02, 0.12, 0.01], [0.01, 0.03, 0.09]])
SLIVER = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.03, 0.04, 1e-5]])
# a corner of a cube with side 1/8: A = 8 I exactly, so b = (8, 0, 0) for a = e_x and d = 8 (x1 - x0) is EXACTLY zero on the tetrahedron flattened along x
CORNER = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.0, 0.125, 0.0], [0.0, 0.0, 0.125]])


def deformed(X, a, l, s, R=None, shift=(0.0, 0.0, 0.0)):
    """x = X F^T + shift with F = R (l a a^T + s (I - a a^T)): the fibre stretch is l, the transverse stretch s"""
    a = unit(a)
    P = np.outer(a, a)
    F = (np.eye(3) if R is None else R) @ (l * P + s * (np.eye(3) - P))
    return np.asarray(X) @ F.T + np.asarray(shift)


def _case(name, X, x, a, k, kind=SPRING, k2=0.0, tension_only=False, act=0.0, energy=0, overflow=False):
    return {"name": name, "X": np.asarray(X, dtype=np.float64), "T": np.array([[0, 1, 2, 3]], dtype=np.int32), "x": np.asarray(x, dtype=np.float64), "a": np.asarray(a, dtype=np.float64),
            "k": float(k), "law": kind, "k2": float(k2), "tension_only": tension_only, "act": float(act), "energy": energy, "overflow": overflow}


def with_elems(case, A9=None, vol=None):
    """the case with its `elems` record: from numpy's rest inputs, or from the context's restTriInv / volume (the GPU tests)"""
    if A9 is None:
        A9, vol = rest_inputs(case["X"], case["T"][0])
    out = dict(case)
    out["elems"] = [elem_record(A9, vol, case["T"][0], case["a"], case["k"], case["law"], case["k2"], case["tension_only"], case["act"])]
    return out


def cases():
    ax, ob = np.array([1.0, 0.0, 0.0]), np.array([0.3, -0.5, 0.8])
    sh = (0.2, -0.1, 0.3)
    out = []
    for act in (-0.2, 0.0, 0.3):
        l0 = 1.0 - act
        out.append(_case(f"spring, l = l0 to rounding, act {act}", REG, deformed(REG, ob, l0, 1.0, OBLIQUE, sh), ob, 3e4, act=act))
        for to in (False, True):
            for side in (-1.0, 1.0):
                out.append(_case(f"spring, l = l0 (1 {'+' if side > 0 else '-'} 1e-6), act {act}, tensiononly {to}", REG,
                                 deformed(REG, ob, l0 * (1.0 + side * 1e-6), 1.05, OBLIQUE, sh), ob, 3e4, tension_only=to, act=act))
    out += [_case("spring, stretched 1.4 along x", REG, deformed(REG, ax, 1.4, 0.9, None, sh), ax, 5e4),
            _case("spring, compressed 0.6, oblique", REG, deformed(REG, ob, 0.6, 1.2, OBLIQUE, sh), ob, 5e4),
            _case("spring, compressed 0.6, tension only", REG, deformed(REG, ob, 0.6, 1.2, OBLIQUE, sh), ob, 5e4, tension_only=True),
            _case("spring, active 0.3 at rest", REG, REG + np.array(sh), ob, 5e4, act=0.3),
            _case("exp, l = 0.8 < 1", REG, deformed(REG, ob, 0.8, 1.1, OBLIQUE, sh), ob, 2e4, EXP, 5.0),
            _case("exp, l = 1.2", REG, deformed(REG, ob, 1.2, 0.95, OBLIQUE, sh), ob, 2e4, EXP, 5.0),
            _case("exp, l = 3, finite exponent", REG, deformed(REG, ob, 3.0, 0.7, OBLIQUE, sh), ob, 2e4, EXP, 0.5),
            _case("exp, the exponent overflows", REG, deformed(REG, ob, 6.0, 0.7, OBLIQUE, sh), ob, 2e4, EXP, 1.0, overflow=True),
            _case("l = 0: a flat tetrahedron normal to the fibre (SNH)", CORNER, deformed(CORNER, ax, 0.0, 1.0, None, (0.25, -0.5, 0.125)), ax, 5e4, act=0.3, energy=2),
            _case("l = 0, tension only (SNH)", CORNER, deformed(CORNER, ax, 0.0, 1.0, None, (0.25, -0.5, 0.125)), ax, 5e4, tension_only=True, energy=2),
            _case("sliver rest shape, large |A|", SLIVER, deformed(SLIVER, ob, 1.1, 1.0, OBLIQUE, sh), ob, 4e4),
            _case("sliver rest shape, exp", SLIVER, deformed(SLIVER, ob, 1.3, 1.0, OBLIQUE, sh), ob, 4e4, EXP, 2.0),
            _case("coordinates offset by 1e3, spring", REG, deformed(REG, ob, 1.25, 1.0, OBLIQUE, (1e3, -1e3, 1e3)), ob, 5e4, act=0.3)]
    return out


@functools.lru_cache(maxsize=None)
def evaluated():
    """[(case with elems, evaluate(case))] of cases(), computed once per process"""
    return [(c, evaluate(c)) for c in (with_elems(c) for c in cases())]
