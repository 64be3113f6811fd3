"""mpmath restatement of the round collider (ipc_amd/csrc/round_collider_kernels.h): signed distance, barrier energy, gradient, the PSD Hessian in closed
form, the step bound, and the lagged friction terms.  A project extension, so there is no oracle to compare with -- this file is the reference, pinned
by tests/test_round_collider_mp.py (mp.diff, mp.eigsy, mp.findroot).

A collider is a dict: p0, p1 (3 floats each), R, hollow.  A sphere has p0 == p1.  q(x) is the closest point of the segment, r = |x - q|, m = (x - q) / r,
side = +1 / -1 (solid / hollow), s = side (r - R), n = side m.  Region "side": 0 < (x - p0) . a < len strictly; "cap" otherwise.
  E = kappa b(s^2, dHat),  b(d) = -(d - dHat)^2 ln(d / dHat)            over the vertices with dbc == 0 and s^2 < dHat
  g = kappa b' 2 s n
  H = kappa [max(0, 4 b'' s^2 + 2 b') n n^T + max(0, 2 b' s side / r) T],  T = I - m m^T (cap) or I - m m^T - a a^T (side)
  step bound: the first t > 0 with s(x + t p) = (1 - slackness) s(x), the ray against the collider of radius R + side (1 - slackness) s(x)

Every formula is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64): the float64 instance is the "NumPy restatement" whose
recorded error sizes the tolerance.

Tolerance of a quantity q of one vertex (as tests/rod_mp.py):  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53
  sens   |q_mp(inputs~) - q_mp(inputs)| entrywise with every coordinate of the vertex (and of its direction, for a step bound), the end points and the
         radius moved by ONE ulp, signs fixed by a seed; the largest of SENS_SAMPLES patterns (a sphere's two end points move together)
  scale  q with every term of its formula replaced by its magnitude (d + dHat for d - dHat, r + R for r - R, ...); for a step bound t = C / (sqrt(disc) - B)
         it is |t| (Cmag / |C| + (B^2 + A Cmag) / disc): the relative rounding of C and of the discriminant, which is what a grazing ray amplifies
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over cases(), rounded up to a power of two
         (test_round_collider_mp.py::test_numpy_restatement_meets_the_tolerance pins it).
"""
import math

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
SENS_SAMPLES = 4
# measured (python tests/round_collider_mp.py): worst err / (sens + u scale) of the float64 restatement over cases() and rays():
# E 0.842, gradient 0.330, Hessian 0.752, step bound 0.206
NUMPY_WORST_RATIO = 0.842
M = 1.0  # 0.842 rounded up to a power of two


class MP:
    @staticmethod
    def num(v):
        return v if isinstance(v, mpf) else mpf(float(v))
    sqrt = staticmethod(mp.sqrt)
    log = staticmethod(mp.log)


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    log = staticmethod(math.log)


def collider(p0, p1, R, hollow=False):
    return {"p0": [float(v) for v in p0], "p1": [float(v) for v in p1], "R": float(R), "hollow": bool(hollow)}


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def evaluate(ops, c, x):
    """s, r, m, a, side region, side"""
    p0, p1, x = [ops.num(v) for v in c["p0"]], [ops.num(v) for v in c["p1"]], [ops.num(v) for v in x]
    R, side = ops.num(c["R"]), (-1 if c["hollow"] else 1)
    d = [x[i] - p0[i] for i in range(3)]
    if c["p0"] == c["p1"]:
        a, L, u = [ops.num(0)] * 3, ops.num(0), ops.num(0)
    else:
        e = [p1[i] - p0[i] for i in range(3)]
        L = ops.sqrt(_dot(e, e))
        a = [e[i] / L for i in range(3)]
        u = _dot(d, a)
    t = min(max(u, ops.num(0)), L)
    w = [d[i] - t * a[i] for i in range(3)]
    r = ops.sqrt(_dot(w, w))
    m = [w[i] / r for i in range(3)] if r > 0 else [ops.num(0)] * 3
    return side * (r - R), r, m, a, bool(u > 0 and u < L), side


def barrier(ops, d, dHat):
    t2, lg = d - dHat, ops.log(d / dHat)
    return -t2 * t2 * lg, t2 * lg * -2 - (t2 * t2) / d, (lg * -2 - t2 * 4 / d) + 1 / (d * d) * (t2 * t2)


def barrier_magnitudes(ops, d, dHat):
    t2, lg = d + dHat, abs(ops.log(d / dHat))
    return t2 * t2 * lg, t2 * lg * 2 + (t2 * t2) / d, (lg * 2 + t2 * 4 / d) + 1 / (d * d) * (t2 * t2)


def active(c, x, dbc, dHat):
    """the constraint set's rule, in mpmath on the float inputs"""
    s = evaluate(MP, c, x)[0]
    return dbc == 0 and s * s < mpf(dHat)


def vertex_terms(ops, c, x, dHat, kappa, magnitudes=False):
    """E, g[3], H[3][3] (the PSD projection in closed form) of one vertex, taken as active; magnitudes: the three scales instead"""
    s, r, m, a, sideRegion, side = evaluate(ops, c, x)
    dHat, kappa = ops.num(dHat), ops.num(kappa)
    d = s * s
    if magnitudes:
        b, gb, Hb = barrier_magnitudes(ops, d, dHat)
        sm = r + ops.num(c["R"])
        return kappa * b, kappa * gb * 2 * sm, kappa * ((4 * Hb * d + 2 * gb) + 2 * gb * sm / r)
    b, gb, Hb = barrier(ops, d, dHat)
    E = kappa * b
    g = [kappa * gb * 2 * s * side * m[i] for i in range(3)]
    c1, c2 = 4 * Hb * d + 2 * gb, (2 * gb * s * side / r if r > 0 else ops.num(0))
    c1, c2 = (c1 if c1 > 0 else ops.num(0)), (c2 if c2 > 0 else ops.num(0))
    ax = 1 if sideRegion else 0
    H = [[kappa * (c1 * (m[i] * m[j]) + c2 * ((1 if i == j else 0) - m[i] * m[j] - ax * (a[i] * a[j]))) for j in range(3)] for i in range(3)]
    return E, g, H


def energy_mp(c, x, dHat, kappa):
    """kappa b(s(x)^2) as a function mp.diff can differentiate (x: three mpf)"""
    s = evaluate(MP, c, x)[0]
    return mpf(kappa) * barrier(MP, s * s, mpf(dHat))[0]


def exact_hessian_mp(c, x, dHat, kappa):
    f = lambda *y: energy_mp(c, list(y), dHat, kappa)
    H = mp.zeros(3, 3)
    for i in range(3):
        for j in range(3):
            o = [0, 0, 0]
            o[i] += 1
            o[j] += 1
            H[i, j] = mp.diff(f, tuple(mpf(v) for v in x), tuple(o))
    return H


def gradient_mp_diff(c, x, dHat, kappa):
    f = lambda *y: energy_mp(c, list(y), dHat, kappa)
    return [mp.diff(f, tuple(mpf(v) for v in x), tuple(1 if k == i else 0 for k in range(3))) for i in range(3)]


def psd_project_mp(H):
    E, Q = mp.eigsy(H)
    D = mp.diag([e if e > 0 else mpf(0) for e in E])
    return Q * D * Q.T


# ---- step bound ---------------------------------------------------------------------------------------------------------------------------------
def _ball_entry(ops, d, p, rad, info=None):
    A, B = _dot(p, p), _dot(d, p)
    C = _dot(d, d) - rad * rad
    if not C > 0 or not B < 0:
        return None
    disc = B * B - A * C
    if not disc >= 0:
        return None
    t = C / (ops.sqrt(disc) - B)
    if info is not None:
        Cm = _dot(d, d) + rad * rad
        info.append((t, abs(t) * (Cm / abs(C) + (B * B + A * Cm) / disc) if disc > 0 else ops.num(math.inf)))
    return t


def step_bound(ops, c, x, p, slackness, with_scale=False):
    """the first t > 0 with s(x + t p) = (1 - slackness) s(x), None where the ray never gets there; with_scale: (t, scale)"""
    s0 = evaluate(ops, c, x)[0]
    if not s0 > 0:
        return (None, None) if with_scale else None
    side = -1 if c["hollow"] else 1
    rad = ops.num(c["R"]) + side * ((1 - ops.num(slackness)) * s0)
    x, p = [ops.num(v) for v in x], [ops.num(v) for v in p]
    p0, p1 = [ops.num(v) for v in c["p0"]], [ops.num(v) for v in c["p1"]]
    d = [x[i] - p0[i] for i in range(3)]
    if side < 0:
        A, B, C = _dot(p, p), _dot(d, p), _dot(d, d) - rad * rad
        if not A > 0 or not C < 0:
            return (None, None) if with_scale else None
        disc = B * B - A * C
        sq = ops.sqrt(disc)
        t = (sq - B) / A if B <= 0 else -C / (B + sq)
        Cm = _dot(d, d) + rad * rad
        return (t, abs(t) * (Cm / abs(C) + (B * B + A * Cm) / disc)) if with_scale else t
    info = []
    _ball_entry(ops, d, p, rad, info)
    if c["p0"] != c["p1"]:
        e = [x[i] - p1[i] for i in range(3)]
        _ball_entry(ops, e, p, rad, info)
        ax = [p1[i] - p0[i] for i in range(3)]
        L = ops.sqrt(_dot(ax, ax))
        a = [ax[i] / L for i in range(3)]
        du, pu = _dot(d, a), _dot(p, a)
        dp, pp = [d[i] - du * a[i] for i in range(3)], [p[i] - pu * a[i] for i in range(3)]
        cyl = []
        t = _ball_entry(ops, dp, pp, rad, cyl)
        if t is not None and 0 <= du + t * pu <= L:
            info += cyl
    if not info:
        return (None, None) if with_scale else None
    best = min(info, key=lambda q: q[0])
    return best if with_scale else best[0]


def gap_along_ray_mp(c, x, p, t):
    return evaluate(MP, c, [mpf(x[i]) + t * mpf(p[i]) for i in range(3)])[0]


# ---- lagged friction ----------------------------------------------------------------------------------------------------------------------------
def lag(ops, c, x, dHat, kappa):
    """lambda and the unit normal of one active vertex at lag time"""
    s, r, m, a, sideRegion, side = evaluate(ops, c, x)
    gb = barrier(ops, s * s, ops.num(dHat))[1]
    return gb * (-ops.num(kappa) * 2 * s), [side * v for v in m]


def friction_terms(ops, n, lam, x, xt, mu, eps2, magnitudes=False):
    """E, g[3], H[3][3] of one lagged entry: the half-space's terms with the lagged normal n"""
    n, x, xt = [ops.num(v) for v in n], [ops.num(v) for v in x], [ops.num(v) for v in xt]
    lam, mu, eps2 = ops.num(lam), ops.num(mu), ops.num(eps2)
    vd = [x[i] - xt[i] for i in range(3)]
    dn = _dot(vd, n)
    vp = [vd[i] - dn * n[i] for i in range(3)]
    m2, eps, ml = _dot(vp, vp), ops.sqrt(eps2), mu * lam
    if magnitudes:
        vm = [abs(x[i]) + abs(xt[i]) for i in range(3)]
        vpm = [vm[i] + _dot(vm, [abs(v) for v in n]) * abs(n[i]) for i in range(3)]
        mm = ops.sqrt(_dot(vpm, vpm))
        if m2 > eps2:
            return abs(ml) * (mm + eps / 2), abs(ml) * mm / ops.sqrt(m2), abs(ml) * (mm * mm / m2 + 2) / ops.sqrt(m2)
        return abs(ml) * mm * mm / eps / 2, abs(ml) * mm / eps, abs(ml) * 2 / eps
    if m2 > eps2:
        mag = ops.sqrt(m2)
        E = ml * (mag - eps / 2)
        g = [ml / mag * vp[i] for i in range(3)]
        H = [[vp[i] * (-ml / m2 / mag) * vp[j] + ((1 if i == j else 0) - n[i] * n[j]) * (ml / mag) for j in range(3)] for i in range(3)]
    else:
        E = ml * m2 / eps / 2
        g = [ml / eps * vp[i] for i in range(3)]
        H = [[((1 if i == j else 0) - n[i] * n[j]) * (ml / eps) for j in range(3)] for i in range(3)]
    return E, g, H


# ---- tolerance ----------------------------------------------------------------------------------------------------------------------------------
def _nudge(v, rng):
    v = np.asarray(v, dtype=np.float64)
    s = rng.integers(0, 2, size=v.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))


def perturbed(c, x, seed, p=None):
    rng = np.random.default_rng(seed)
    p0 = _nudge(c["p0"], rng)
    p1 = p0 if c["p0"] == c["p1"] else _nudge(c["p1"], rng)
    c2 = collider(p0, p1, float(_nudge(c["R"], rng)), c["hollow"])
    x2 = _nudge(x, rng)
    return (c2, x2) if p is None else (c2, x2, _nudge(p, rng))


def _flat(q):
    E, g, H = q
    return [E] + list(g) + [H[i][j] for i in range(3) for j in range(3)]


def expected_vertex(c, x, dHat, kappa):
    """reference and tolerance / M of E, g, H of one active vertex: two arrays of 13 floats (E, g[3], H row-major)"""
    ref = _flat(vertex_terms(MP, c, x, dHat, kappa))
    sens = [mpf(0)] * 13
    for k in range(SENS_SAMPLES):
        c2, x2 = perturbed(c, x, k + 1)
        q = _flat(vertex_terms(MP, c2, x2, dHat, kappa))
        sens = [max(a, abs(b - r)) for a, b, r in zip(sens, q, ref)]
    sE, sg, sH = vertex_terms(MP, c, x, dHat, kappa, magnitudes=True)
    scale = [sE] + [sg] * 3 + [sH] * 9
    return np.array([float(v) for v in ref]), np.array([float(a + mpf(U) * b) for a, b in zip(sens, scale)])


def expected_friction(c, xlag, dHat, kappa, x, xt, mu, eps2):
    """the same for the friction terms of one entry lagged at xlag (lambda and the normal from there) and evaluated at x against x^t; lambda enters
    every term linearly, so its own rounding multiplies the scale by lambda's magnitude form over |lambda|"""
    def terms(c_, xl_, x_, xt_):
        lam, n = lag(MP, c_, xl_, dHat, kappa)
        return lam, _flat(friction_terms(MP, n, lam, x_, xt_, mu, eps2))
    lam, ref = terms(c, xlag, x, xt)
    sens = [mpf(0)] * 13
    for k in range(SENS_SAMPLES):
        c2, xl2 = perturbed(c, xlag, 100 + k)
        rng = np.random.default_rng(150 + k)
        q = terms(c2, xl2, _nudge(x, rng), _nudge(xt, rng))[1]
        sens = [max(a, abs(b - r)) for a, b, r in zip(sens, q, ref)]
    n = lag(MP, c, xlag, dHat, kappa)[1]
    sE, sg, sH = friction_terms(MP, n, lam, x, xt, mu, eps2, magnitudes=True)
    lamScale = vertex_terms(MP, c, xlag, dHat, kappa, magnitudes=True)[1] / abs(lam)
    scale = [sE * lamScale] + [sg * lamScale] * 3 + [sH * lamScale] * 9
    return np.array([float(v) for v in ref]), np.array([float(a + mpf(U) * b) for a, b in zip(sens, scale)])


def expected_step(c, x, p, slackness):
    """(t, tolerance / M) of one ray, (None, None) where it does not bound the step"""
    t, scale = step_bound(MP, c, x, p, slackness, with_scale=True)
    if t is None:
        return None, None
    sens = mpf(0)
    for k in range(SENS_SAMPLES):
        c2, x2, p2 = perturbed(c, x, 200 + k, p)
        t2 = step_bound(MP, c2, x2, p2, slackness)
        if t2 is not None:
            sens = max(sens, abs(t2 - t))
    return float(t), float(sens + mpf(U) * scale)


def ratio(err, tol):
    """err / tol entrywise, 0 where both are 0, inf where only the tolerance is"""
    err, tol = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol, dtype=np.float64)
    out = np.zeros_like(err)
    nz = tol > 0
    out[nz] = err[nz] / tol[nz]
    out[~nz & (err > 0)] = np.inf
    return out


# ---- cases: what test_gpu_round_collider_mp.py places on its five-tet cubes ----------------------------------------------------------------------
DHAT = 0.01  # squared: the barrier starts at a gap of 0.1
KAPPA = 3.5e3
GAPS = (0.02, 0.05, 0.09, 0.0999999, 0.1000001, 0.3)  # the fourth just inside dHat, the fifth just outside
DIRS = [(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.6, 0.0, 0.8), (-0.36, 0.48, -0.8), (0.3, -0.5, 0.2), (-0.7, 0.1, 0.4), (0.2, 0.9, -0.3)]


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _sphere_points(c):
    ctr, R, side = np.array(c["p0"]), c["R"], (-1.0 if c["hollow"] else 1.0)
    P = [ctr + (R + side * g) * _unit(DIRS[(i + k) % len(DIRS)]) for i in range(len(DIRS)) for k, g in enumerate(GAPS)]
    return np.array(P[:40])


def _capsule_points(c):
    p0, p1, R = np.array(c["p0"]), np.array(c["p1"]), c["R"]
    a = _unit(p1 - p0)
    L = float(np.linalg.norm(p1 - p0))
    w0 = _unit(np.cross(a, [0.3, -0.2, 0.9]))
    w1 = np.cross(a, w0)
    P = []
    for k, g in enumerate(GAPS):  # side region, around the axis
        ang = 0.7 * k + 0.2
        P.append(p0 + (0.15 + 0.13 * k) * L * a + (R + g) * (math.cos(ang) * w0 + math.sin(ang) * w1))
    for k, g in enumerate(GAPS):  # the two caps
        u = _unit(a + 0.8 * math.cos(1.1 * k) * w0 + 0.8 * math.sin(1.1 * k) * w1)
        P.append(p1 + (R + g) * u)
        P.append(p0 + (R + g) * (u - 2 * (u @ a) * a))
    for g in GAPS[:4]:  # exactly on the end planes t = 0 and t = 1 (exact where the capsule is axis-aligned and dyadic), and on the axis extension
        P.append(p0 + (R + g) * w0)
        P.append(p1 + (R + g) * w1)
        P.append(p1 + (R + g) * a)
        P.append(p0 - (R + g) * a)
    P += [p0 + 0.5 * L * a + (R + 0.0625) * w0, p0 + 0.25 * L * a - (R + 0.03125) * w1]
    P += [p0 + (0.1 + 0.2 * k) * L * a - (R + g) * _unit(w0 + (k - 1.5) * w1) for k, g in enumerate(GAPS[:4])]
    return np.array(P[:40])


def cases():
    """name -> (collider, 40 points, dbc[40]): the last point inside dHat is a Dirichlet node"""
    out = {}
    shapes = {"solid_sphere": collider((0.25, -0.5, 0.125), (0.25, -0.5, 0.125), 0.75),
              "hollow_sphere": collider((0.25, -0.5, 0.125), (0.25, -0.5, 0.125), 1.5, hollow=True),
              "capsule_aligned": collider((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.5),
              "capsule_skew": collider((0.1, -0.2, 0.3), (0.9, 0.5, -0.1), 0.35)}
    for name, c in shapes.items():
        P = _sphere_points(c) if c["p0"] == c["p1"] else _capsule_points(c)
        if name == "capsule_aligned":  # w0, w1 come out as -e_z-ish / e_y-ish combinations: snap the end-plane points to exact dyadic coordinates
            P[30] = [0.0, 0.5 + 0.0625, 0.0]
            P[31] = [1.0, 0.0, -(0.5 + 0.03125)]
        dbc = np.zeros(40, dtype=np.int32)
        dbc[2] = 1  # a gap of 0.09 (spheres) / 0.09 (capsules, side region): inside dHat, yet never in the set
        out[name] = (c, P, dbc)
    return out


def _graze_offset(R, along, slackness=0.9):
    """impact parameter b of a ray that starts `along` before its closest approach: b = (1 - 1e-6) x the inflated radius R + (1 - slackness)(sqrt(b^2 + along^2) - R)"""
    b = R
    for _ in range(60):
        b = (R + (1 - slackness) * (math.sqrt(b * b + along * along) - R)) * (1 - 1e-6)
    return b


def rays(name):
    """(vertex position, direction, label) per shape: hits, a near-graze, a miss and one pointing away"""
    c = cases()[name][0]
    p0, p1, R = np.array(c["p0"]), np.array(c["p1"]), c["R"]
    if c["hollow"]:
        x = p0 + np.array([0.3, -0.2, 0.4])
        return [(x, np.array([1.0, 0.5, -0.25]), "outwards"), (x, np.array([-2.0, 0.1, 0.3]), "across"), (x, np.array([1e-3, 0.0, 0.0]), "short"),
                (p0 + np.array([0.0, 1.3, 0.0]), np.array([0.0, 1.0, 0.0]), "radial"), (x, np.zeros(3), "still")]
    if c["p0"] == c["p1"]:
        x = p0 + np.array([R + 0.4, 0.1, -0.2])
        graze = np.array([-1.0, 0.0, 0.0])
        xg = p0 + np.array([R + 0.5, _graze_offset(R, R + 0.5), 0.0])  # passes the inflated ball just inside its rim
        return [(x, np.array([-1.0, 0.0, 0.1]), "hit"), (xg, graze, "graze"), (x, np.array([0.0, 1.0, 0.0]), "miss"), (x, np.array([1.0, 0.2, 0.0]), "away"),
                (x, np.array([-0.01, 0.0, 0.0]), "short")]
    a = _unit(p1 - p0)
    L = float(np.linalg.norm(p1 - p0))
    w = _unit(np.cross(a, [0.3, -0.2, 0.9]))
    xs = p0 + 0.4 * L * a + (R + 0.3) * w
    xc = p1 + (R + 0.3) * _unit(a + 0.5 * w)
    return [(xs, -w, "side hit"), (xs, -w + 0.9 * a, "side oblique"), (xc, -_unit(a + 0.5 * w), "cap hit"), (xc, -a - 0.1 * w, "cap oblique"),
            (xs + 2.0 * L * a, -w, "miss"), (xs, w + 0.3 * a, "away"), (p0 - (R + 0.4) * a, a, "along the axis"),
            (p0 + 0.5 * L * a + _graze_offset(R, 1.0) * w + 1.0 * np.cross(a, w), -np.cross(a, w) * 2.0, "graze")]


def numpy_worst_ratio():
    worst = {"E": 0.0, "g": 0.0, "H": 0.0, "t": 0.0}
    for name, (c, P, dbc) in cases().items():
        for x in P:
            if not active(c, x, 0, DHAT):
                continue
            ref, tol = expected_vertex(c, x, DHAT, KAPPA)
            r = ratio(np.array([float(v) for v in _flat(vertex_terms(NP, c, x, DHAT, KAPPA))]) - ref, tol)
            worst["E"], worst["g"], worst["H"] = max(worst["E"], r[0]), max(worst["g"], r[1:4].max()), max(worst["H"], r[4:].max())
        for x, p, label in rays(name):
            t, tol = expected_step(c, x, p, 0.9)
            tn = step_bound(NP, c, x, p, 0.9)
            assert (t is None) == (tn is None), (name, label)
            if t is not None:
                worst["t"] = max(worst["t"], float(ratio(tn - t, tol)))
    return worst


if __name__ == "__main__":
    print(numpy_worst_ratio())
