"""Reference of the shells' plastic flow (ipc_amd/csrc/shell_plastic_kernels.h) in plain mpmath -- the membrane flow of one triangle, the flow of one hinge and
the state query --, its hand-placed cases, the tolerances and a float64 NumPy restatement that shows the tolerances are attainable.

A helper module after plastic_mp.py, whose DPS, U and M it takes; used by test_shell_plastic_mp.py, test_gpu_shell_plastic_mp.py and
test_gpu_shell_plastic_step.py.  Nothing here shares code or arithmetic with ipc_amd/: every quantity is built in mp from the exact doubles handed to the GPU.

  triangle   F = [x1 - x0, x2 - x0] B (3 x 2),  C = F^T F = Q diag(l) Q^T (mp.eigsy: repeated stretches need no special case),  e_i = ln(l_i) / 2,
             e3 = -c (e1 + e2),  c = k5 / (2 k4) from the two StVK constants,  d = (e1, e2, e3) - mean,  n = |d|
             det C = |(x1 - x0) x (x2 - x0)|^2 det(B)^2 <= 0 (exact in mp: a collapsed triangle): skipped.   y = yield + harden alpha.   n <= y: nothing.
             Delta = r (n - y) / (1 + harden),  r = -expm1(-creep dt)  (1 at creep = inf),  G = Q diag(exp(-Delta e_i / n)) Q^T,  B' = B G,  alpha' = alpha + Delta
  hinge      theta = atan2((n1 x n2) . e / |e|, n1 . n2),  k = theta - thetaBar (not unwrapped),  eps = g |k|;  a zero n1, n2 or e: skipped.
             y = bendYield + harden alphaB.   eps <= y: nothing.   Delta as above,  thetaBar' = thetaBar + sign(k) Delta / g,  alphaB' = alphaB + Delta

B is a 2 x 2 array B[i][j]; the C ABI's four doubles per triangle are b00 b10 b01 b11 (column-major).

Tolerances.  Each is the reference's own sensitivity to a one-ulp perturbation of its inputs plus M U times the scale of the quantity, M = plastic_mp.M = 128,
U = 2^-53:  tol = sens + M U scale.
  sens   |f_mp(inputs~) - f_mp(inputs)| with every coordinate and every entry of B (or thetaBar and g) multiplied by 1 +- U, signs fixed by a seed; the largest of
         SENS_SAMPLES = 4 sign patterns (one pattern can cancel)
  scale  B': max(|B|_max, |B'|_max) -- B' = B G is a sum of two products of entries of B with entries of G, and the rotation mixes the entries;
         alpha': alpha + n + max |e_i| -- the magnitudes of the terms it is summed from;   n (state): n + max |e_i|;   the area ratio: itself;
         thetaBar': |thetaBar| + |theta| + |k| -- it is thetaBar plus a fraction of k = theta - thetaBar;   alphaB', eps: alphaB + eps + y;
         thetaBar - thetaBar0: |thetaBar| + |thetaBar0|
Both flows are continuous across their yield surfaces (Delta -> 0), so a reference and a kernel that decide n <= y differently within rounding still agree
within tol; only "not a bit is written" and the counters need the decision itself, and those are asserted where it is DECIDED: |n - y| > DECIDE = 2^-40
(plastic_mp.DECIDE; n and eps are good to a few U relative to max(1, |e|), far below it)."""
import numpy as np
from mpmath import mp, mpf

import plastic_mp as pmp

DPS, U, M = pmp.DPS, pmp.U, pmp.M
SENS_SAMPLES, DECIDE = pmp.SENS_SAMPLES, pmp.DECIDE
INF = float("inf")
_at_dps = pmp._at_dps


def to2(b4):
    """the C ABI's four doubles of one triangle (b00 b10 b01 b11) -> B[i][j]"""
    return np.asarray(b4, dtype=np.float64).reshape(2, 2).T.copy()


def to4(B):
    return np.asarray(B, dtype=np.float64).T.reshape(4).copy()


def rest_B(Xr):
    """Dm^-1 of a rest triangle in doubles, in the frame of shell_plan.h (first axis along X1 - X0): the CPU tests' stand-in for what the library computes"""
    Xr = np.asarray(Xr, dtype=np.float64)
    a, b = Xr[1] - Xr[0], Xr[2] - Xr[0]
    t1 = a / np.linalg.norm(a)
    nn = np.cross(a, b)
    t2 = np.cross(nn / np.linalg.norm(nn), t1)
    Dm = np.array([[a @ t1, b @ t1], [a @ t2, b @ t2]])
    return np.linalg.inv(Dm)


def plane_stress_c(nu):
    """c = lambda_ps / (2 mu) = nu / (1 - nu) as the quotient of two doubles k5 / (2 k4) with k4 = mu, k5 = lambda_ps at E = 1: (k4, k5)"""
    return 1.0 / (2.0 * (1.0 + nu)), nu / (1.0 - nu * nu)


def _f(v):
    return v if isinstance(v, mpf) else mpf(float(v))


def _m(A):
    return [[_f(v) for v in r] for r in A]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(p * q for p, q in zip(a, b))


# ---- the triangle ---------------------------------------------------------------------------------------------------------------------------------
@_at_dps
def tri_strain(X, B, k4, k5):
    """(e (e1 >= e2), Q (mp.matrix, columns to e1, e2), d (3), n) or None where the triangle is collapsed"""
    P, Bm = _m(X), _m(B)
    u1, u2 = [P[1][i] - P[0][i] for i in range(3)], [P[2][i] - P[0][i] for i in range(3)]
    w = _cross(u1, u2)
    detB = Bm[0][0] * Bm[1][1] - Bm[0][1] * Bm[1][0]
    if not _dot(w, w) * detB * detB > 0:
        return None
    f = [[u1[i] * Bm[0][j] + u2[i] * Bm[1][j] for i in range(3)] for j in range(2)]
    C = mp.matrix(2, 2)
    for i in range(2):
        for j in range(2):
            C[i, j] = _dot(f[i], f[j])
    ev, Q = mp.eigsy(C)  # ascending
    e = [mp.log(ev[1]) / 2, mp.log(ev[0]) / 2]
    Q2 = mp.matrix(2, 2)
    for i in range(2):
        Q2[i, 0], Q2[i, 1] = Q[i, 1], Q[i, 0]
    c = _f(k5) / (2 * _f(k4))
    e3 = -c * (e[0] + e[1])
    m = (e[0] + e[1] + e3) / 3
    d = [e[0] - m, e[1] - m, e3 - m]
    return e, Q2, d, mp.sqrt(sum(v * v for v in d))


@_at_dps
def flow_tri(X, B, k4, k5, yld, creep, harden, alpha, dt):
    """(B', alpha', n, yielded, f): B' a 2 x 2 list of mpf; n is None where the triangle is skipped and where the flow is off; f = Delta / n (0 without flow)"""
    Bm, alpha = _m(B), _f(alpha)
    if not float(yld) < INF:
        return Bm, alpha, None, False, mpf(0)
    st = tri_strain(X, Bm, k4, k5)
    if st is None:
        return Bm, alpha, None, False, mpf(0)
    e, Q, _, n = st
    K = _f(harden)
    y = _f(yld) + K * alpha
    if n <= y:
        return Bm, alpha, n, False, mpf(0)
    r = mpf(1) if float(creep) == INF else -mp.expm1(-_f(creep) * _f(dt))
    Delta = r * (n - y) / (1 + K)
    f = Delta / n
    g = [mp.exp(-f * v) for v in e]
    G = [[sum(Q[i, k] * g[k] * Q[j, k] for k in range(2)) for j in range(2)] for i in range(2)]
    B1 = [[sum(Bm[i][k] * G[k][j] for k in range(2)) for j in range(2)] for i in range(2)]
    return B1, alpha + Delta, n, True, f


def _signs(seed, n):
    return np.where(np.random.default_rng(seed).integers(0, 2, size=n).astype(bool), 1, -1)


@_at_dps
def tri_reference(case, B=None, k=None, seed=0):
    """the membrane flow of one case from the doubles (X, B, k4, k5, parameters), with the tolerances: dict B1 (2 x 2), alpha1, n, y (doubles; n NaN where
    skipped or off), yielded, skipped, decided, tolB (2 x 2), tolAlpha, tolN, ratio (det B / det B1: what the area ratio changes by), tolRatio"""
    B = np.asarray(case["B"] if B is None else B, dtype=np.float64)
    k4, k5 = case["k"] if k is None else k
    X = np.asarray(case["X"], dtype=np.float64)
    par = (case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
    B1, al1, n, yielded, _ = flow_tri(X, B, k4, k5, *par)
    det = lambda Z: Z[0][0] * Z[1][1] - Z[0][1] * Z[1][0]
    ratio = det(_m(B)) / det(B1)
    st = tri_strain(X, B, k4, k5)
    u = mpf(U)
    sensB, sensAl, sensN, sensR = np.zeros((2, 2)), 0.0, 0.0, 0.0
    for s_ in range(SENS_SAMPLES):
        s = _signs(9000 + 100 * seed + s_, 13)
        Xp = [[_f(X[a][i]) * (1 + int(s[3 * a + i]) * u) for i in range(3)] for a in range(3)]
        Bp = [[_f(B[i][j]) * (1 + int(s[9 + 2 * i + j]) * u) for j in range(2)] for i in range(2)]
        C1, bl1, _, _, _ = flow_tri(Xp, Bp, k4, k5, *par)
        sensB = np.maximum(sensB, np.array([[float(abs(C1[i][j] - B1[i][j])) for j in range(2)] for i in range(2)]))
        sensAl = max(sensAl, float(abs(bl1 - al1)))
        sensR = max(sensR, float(abs(det(Bp) / det(C1) - ratio)))
        sp = tri_strain(Xp, Bp, k4, k5)
        if st is not None and sp is not None:
            sensN = max(sensN, float(abs(sp[3] - st[3])))
    y = float(case["yield"]) + float(case["harden"]) * float(case["alpha"])
    emax = float(max(abs(v) for v in st[0])) if st is not None else 0.0
    nAll = float(st[3]) if st is not None else float("nan")  # (the state query gives n also where the flow is off)
    nf = float(n) if n is not None else float("nan")
    B1f = np.array([[float(v) for v in r] for r in B1])
    return dict(B1=B1f, alpha1=float(al1), n=nf, nState=nAll, y=y, yielded=yielded, skipped=st is None and float(case["yield"]) < INF,
                decided=n is None or abs(nf - y) > DECIDE, tolB=sensB + M * U * max(np.abs(B).max(), np.abs(B1f).max()),
                tolAlpha=sensAl + M * U * (float(case["alpha"]) + (nf if n is not None else 0.0) + emax), tolN=sensN + M * U * ((nAll if st is not None else 0.0) + emax),
                ratio=float(ratio), tolRatio=sensR + M * U * abs(float(ratio)))


def flow_tri_np(X, B, k4, k5, yld, creep, harden, alpha, dt):
    """(B', alpha', n, yielded) in plain doubles by a route of its own (numpy's eigh of C)"""
    X, B = np.asarray(X, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if not yld < INF:
        return B.copy(), alpha, float("nan"), False
    E = np.stack([X[1] - X[0], X[2] - X[0]], axis=1)
    w = np.cross(E[:, 0], E[:, 1])
    if not (w @ w) * np.linalg.det(B) ** 2 > 0.0:
        return B.copy(), alpha, float("nan"), False
    F = E @ B
    lam, Q = np.linalg.eigh(F.T @ F)
    e = 0.5 * np.log(lam)
    e3 = -(k5 / (2.0 * k4)) * (e[0] + e[1])
    d = np.array([e[0], e[1], e3]) - ((e[0] + e[1]) + e3) / 3.0
    n = float(np.sqrt(d @ d))
    y = yld + harden * alpha
    if not n > y:
        return B.copy(), alpha, n, False
    Delta = -np.expm1(-creep * dt) * (n - y) / (1.0 + harden)
    G = (Q * np.exp(-Delta / n * e)) @ Q.T
    return B @ G, alpha + Delta, n, True


# ---- the hinge ------------------------------------------------------------------------------------------------------------------------------------
@_at_dps
def hinge_theta(X):
    """theta of the hinge (x0, x1 | x2, x3), or None where n1, n2 or e has zero length"""
    P = _m(X)
    e = [P[1][i] - P[0][i] for i in range(3)]
    n1 = _cross(e, [P[2][i] - P[0][i] for i in range(3)])
    n2 = _cross([-v for v in e], [P[3][i] - P[1][i] for i in range(3)])
    if not (_dot(e, e) > 0 and _dot(n1, n1) > 0 and _dot(n2, n2) > 0):
        return None
    return mp.atan2(_dot(_cross(n1, n2), e) / mp.sqrt(_dot(e, e)), _dot(n1, n2))


@_at_dps
def flow_hinge(X, thetaBar, g, yld, creep, harden, alphaB, dt):
    """(thetaBar', alphaB', eps, yielded, theta): eps and theta None where the hinge is skipped or does not flow"""
    tb, al, g = _f(thetaBar), _f(alphaB), _f(g)
    if not float(yld) < INF:
        return tb, al, None, False, None
    theta = hinge_theta(X)
    if theta is None:
        return tb, al, None, False, None
    k = theta - tb
    eps = g * abs(k)
    K = _f(harden)
    y = _f(yld) + K * al
    if eps <= y:
        return tb, al, eps, False, theta
    r = mpf(1) if float(creep) == INF else -mp.expm1(-_f(creep) * _f(dt))
    Delta = r * (eps - y) / (1 + K)
    return tb + mp.sign(k) * Delta / g, al + Delta, eps, True, theta


@_at_dps
def hinge_reference(case, thetaBar=None, g=None, seed=0):
    """the flow of one hinge case, with the tolerances: dict thetaBar1, alphaB1, eps, y, theta (doubles; NaN where skipped or off), yielded, skipped, decided,
    tolTheta, tolAlpha, tolEps"""
    tb = float(case["thetaBar"] if thetaBar is None else thetaBar)
    g = float(case["g"] if g is None else g)
    X = np.asarray(case["X"], dtype=np.float64)
    par = (case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
    t1, a1, eps, yielded, theta = flow_hinge(X, tb, g, *par)
    u = mpf(U)
    sT, sA, sE = 0.0, 0.0, 0.0
    for s_ in range(SENS_SAMPLES):
        s = _signs(9500 + 100 * seed + s_, 14)
        Xp = [[_f(X[a][i]) * (1 + int(s[3 * a + i]) * u) for i in range(3)] for a in range(4)]
        t2, a2, e2, _, _ = flow_hinge(Xp, _f(tb) * (1 + int(s[12]) * u), _f(g) * (1 + int(s[13]) * u), *par)
        sT, sA = max(sT, float(abs(t2 - t1))), max(sA, float(abs(a2 - a1)))
        if eps is not None and e2 is not None:
            sE = max(sE, float(abs(e2 - eps)))
    y = float(case["yield"]) + float(case["harden"]) * float(case["alpha"])
    nan = float("nan")
    ef, thf = (float(eps), float(theta)) if eps is not None else (nan, nan)
    mag = float(case["alpha"]) + (ef + y if eps is not None else 0.0)
    return dict(thetaBar1=float(t1), alphaB1=float(a1), eps=ef, y=y, theta=thf, yielded=yielded, skipped=eps is None and float(case["yield"]) < INF,
                decided=eps is None or abs(ef - y) > DECIDE, tolTheta=sT + M * U * (abs(tb) + (2 * abs(thf) + abs(tb) if eps is not None else 0.0)),
                tolAlpha=sA + M * U * mag, tolEps=sE + M * U * mag)


def flow_hinge_np(X, thetaBar, g, yld, creep, harden, alphaB, dt):
    """(thetaBar', alphaB', eps, yielded) in plain doubles"""
    X = np.asarray(X, dtype=np.float64)
    if not yld < INF:
        return thetaBar, alphaB, float("nan"), False
    e = X[1] - X[0]
    n1, n2 = np.cross(e, X[2] - X[0]), np.cross(-e, X[3] - X[1])
    if not (e @ e > 0 and n1 @ n1 > 0 and n2 @ n2 > 0):
        return thetaBar, alphaB, float("nan"), False
    theta = np.arctan2(np.cross(n1, n2) @ e / np.sqrt(e @ e), n1 @ n2)
    k = theta - thetaBar
    eps = g * abs(k)
    y = yld + harden * alphaB
    if not eps > y:
        return thetaBar, alphaB, eps, False
    Delta = -np.expm1(-creep * dt) * (eps - y) / (1.0 + harden)
    return thetaBar + np.copysign(Delta / g, k), alphaB + Delta, eps, True


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
REST_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.75, 0.0]])  # no right angle, no equal sides
UNIT_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # B = I exactly


def _rot(seed):
    q = np.random.default_rng(seed).normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def tri_case(name, F2, rest=REST_TRI, rot=None, nu=0.3, yld=0.05, creep=INF, harden=0.0, alpha=0.0, dt=0.01, thickness=0.01):
    """a triangle whose rest shape `rest` (in the plane z = 0) is deformed in its plane by the 2 x 2 matrix F2 and then rotated"""
    F = np.eye(3)
    F[:2, :2] = np.asarray(F2, dtype=np.float64) if np.ndim(F2) == 2 else np.diag(F2)
    if rot is not None:
        F = _rot(rot) @ F
        name += ", rotated"
    return dict(name=name, Xr=rest.copy(), X=rest @ F.T, B=rest_B(rest), k=plane_stress_c(nu), nu=float(nu), thickness=float(thickness), **{"yield": float(yld)},
                creep=float(creep), harden=float(harden), alpha=float(alpha), dt=float(dt))


@_at_dps
def tri_cases():
    out = []

    def add(name, F2, **kw):
        out.append(tri_case(name, F2, **kw))
        out.append(tri_case(name, F2, rot=300 + len(out), **kw))
    for nu in (0.0, 0.3, 0.49):
        add(f"uniaxial stretch, nu {nu:g}", (1.3, 1.0), nu=nu)
        add(f"biaxial stretch, nu {nu:g}", (1.25, 0.9), nu=nu)
    add("equal stretch (l1 == l2)", (1.2, 1.2))
    add("equal stretch, unit triangle (b == 0 and a == c)", (1.2, 1.2), rest=UNIT_TRI)
    add("pure shear", [[1.0, 0.4], [0.0, 1.0]])
    add("pure shear, unit triangle", [[1.0, 0.4], [0.0, 1.0]], rest=UNIT_TRI)
    add("unit triangle stretched along its second axis (b == 0, a < c)", (0.9, 1.3), rest=UNIT_TRI)
    out.append(tri_case("rest, yield 0 (n = 0 = y exactly: on the yield surface)", (1.0, 1.0), rest=UNIT_TRI, yld=0.0))
    out.append(tri_case("rest, yield 0", (1.0, 1.0), rot=77, yld=0.0))  # rigidly rotated: n = 0 up to rounding
    add("below yield", (1.02, 0.99))
    add("finite creep", (1.3, 0.95), creep=5.0, dt=0.01)
    add("finite creep, long step", (1.3, 0.95), creep=5.0, dt=0.1)
    add("hardening from alpha 0.1", (1.3, 0.95), harden=0.5, alpha=0.1)
    add("hardening keeps it elastic", (1.1, 0.98), harden=2.0, alpha=0.1)
    add("creep and hardening", (0.8, 1.25), creep=20.0, dt=0.025, harden=0.25, alpha=0.03)
    add("switched off", (1.3, 0.95), yld=INF)
    # collapsed: all three nodes in one point, and x2 on the line x0 x1 (parallel edges in their doubles)
    c0 = tri_case("collapsed to a point", (1.0, 1.0))
    c0["X"] = np.tile(c0["X"][0], (3, 1))
    c1 = tri_case("collapsed to a line", (1.0, 1.0))
    c1["X"] = np.array([[0.5, 0.25, 1.0], [1.5, 0.75, 0.5], [2.5, 1.25, 0.0]])
    out += [c0, c1]
    # decided, just: y = n (1 + 4 DECIDE) -- from below, bits kept
    nn = tri_strain(tri_case("", (1.3, 1.0))["X"], rest_B(REST_TRI), *plane_stress_c(0.3))[3]
    out.append(tri_case("on the yield surface from below", (1.3, 1.0), yld=float(nn * (1 + 4 * mpf(DECIDE)))))
    # n just below and just above y, one ulp apart in the stretch: y lies between the two norms (continuity; the decision is not asserted)
    lo, hi = 1.3, float(np.nextafter(1.3, 2.0))
    nl, nh = (tri_strain(UNIT_TRI @ np.diag((s, 1.0, 1.0)), np.eye(2), *plane_stress_c(0.3))[3] for s in (lo, hi))
    y = float((nl + nh) / 2)
    out.append(tri_case("one ulp below the yield surface", (lo, 1.0), rest=UNIT_TRI, yld=y))
    out.append(tri_case("one ulp above the yield surface", (hi, 1.0), rest=UNIT_TRI, yld=y))
    return out


def hinge_rest(angle=0.0):
    """two triangles over the edge x0 = (0, 0, 0), x1 = (0, 1, 0): x2 at +x, x3 at -x lifted by the dihedral angle; nodes x0, x1, x2, x3"""
    return np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.8, 0.3, 0.0], [-0.7 * np.cos(angle), 0.6, 0.7 * np.sin(angle)]])


HINGE_TRI = np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)


def hinge_case(name, fold, rest_angle=0.0, rot=None, yld=0.002, creep=INF, harden=0.0, alpha=0.0, dt=0.01, thickness=0.01, g=None, degenerate=False):
    """rest at `rest_angle`, current positions folded to `fold`.  g defaults to the plan's formula in doubles for this rest shape"""
    Xr, X = hinge_rest(rest_angle), hinge_rest(fold)
    if degenerate:
        X[3] = X[1] + 0.5 * (X[0] - X[1])  # x3 on the edge: n2 = 0 exactly
    if rot is not None:
        X = X @ _rot(rot).T
        name += ", rotated"
    area = lambda P, t: 0.5 * np.linalg.norm(np.cross(P[t[1]] - P[t[0]], P[t[2]] - P[t[0]]))
    w = 3.0 * 1.0 / (area(Xr, HINGE_TRI[0]) + area(Xr, HINGE_TRI[1]))
    th0 = hinge_theta(Xr)
    return dict(name=name, Xr=Xr, X=X, thetaBar=float(th0), g=float(thickness * w / 2.0) if g is None else g, thickness=float(thickness), **{"yield": float(yld)},
                creep=float(creep), harden=float(harden), alpha=float(alpha), dt=float(dt))


@_at_dps
def hinge_cases():
    out = []
    for fold in (0.3, -0.3, 3.0, -3.0):
        out.append(hinge_case(f"flat rest folded to {fold:g}", fold))
        out.append(hinge_case(f"flat rest folded to {fold:g}", fold, rot=500 + len(out)))
    out.append(hinge_case("curved rest 0.5 folded past it to 0.9", 0.9, rest_angle=0.5))
    out.append(hinge_case("curved rest 0.5 folded back through flat to -0.2 (k changes sign)", -0.2, rest_angle=0.5, rot=41))
    out.append(hinge_case("below yield", 0.05, yld=0.01))
    out.append(hinge_case("finite creep", 0.3, creep=5.0, dt=0.02, rot=42))
    out.append(hinge_case("hardening from alphaB 0.001", 0.3, harden=0.5, alpha=0.001))
    out.append(hinge_case("creep and hardening", -0.6, creep=20.0, dt=0.025, harden=2.0, alpha=0.0005, rot=43))
    out.append(hinge_case("switched off", 0.3, yld=INF))
    out.append(hinge_case("degenerate wing", 0.3, degenerate=True))
    out.append(hinge_case("flat at yield 0 (eps = 0 = y)", 0.0, yld=0.0))
    return out
