"""Per-element reference of the plastic flow (ipc_amd/csrc/plastic_kernels.h) in plain mpmath, its hand-placed cases, the tolerance and a float64 NumPy
restatement that shows the tolerance is attainable.

A helper module (like snh_mp.py, whose M and U it takes), used by test_plastic_mp.py, test_gpu_plastic_mp.py and test_gpu_plastic_step.py.  Nothing here shares
code or arithmetic with ipc_amd/: every quantity is built in mp (mp.dps = 100) from the exact doubles handed to the GPU.

  F = Ds(x) A,  C = F^T F = Q diag(lambda) Q^T (mp.eigsy: no SVD, so repeated stretches need no special case),  e_i = ln(lambda_i) / 2,  d = e - mean(e),  n = |d|
  det F <= 0: skipped.   y = yield + harden alpha.   n <= y: nothing.   Delta = r (n - y) / (1 + harden),  r = -expm1(-creep dt)  (1 at creep = inf)
  G = Q diag(exp(-Delta d_i / n)) Q^T,  A' = A G,  alpha' = alpha + Delta

A is a 3 x 3 array A[i][j]; the C ABI's nine doubles per element are A[i][j] at 3 j + i (column-major): a9.reshape(3, 3).T.

Tolerance of A' (entry by entry):  tol = M (sens + u |A|_max),  M = snh_mp.M = 128,  u = 2^-53.
  sens   |A'_mp(x~, A~) - A'_mp(x, A)| with each of the twelve coordinates and nine entries of A multiplied by 1 +- u, the signs fixed by a seed; the largest of
         SENS_SAMPLES = 4 sign patterns (as snh_mp: one pattern can cancel)
  scale  |A|_max: A' = A G is a sum of three products of entries of A with entries of a matrix whose norm is exp(Delta |d|_inf / n) <= e^Delta, and the
         rotations mix the entries
Tolerance of alpha': M (sens(alpha') + u (alpha + n + max |e_i|)) -- the magnitudes of the terms it is summed from.
The flow is continuous across the yield surface (Delta -> 0), so a reference and a kernel that decide n <= y differently within rounding still agree within
tol; only the statement "not a bit is written" and the counters need the decision itself, and those are asserted where it is DECIDED: |n - y| > DECIDE.
  DECIDE = 2^-40: n comes from three logarithms of singular values, each good to a few u relative to max(1, |e|) <= 8 in every case here, far below 2^-40.
"""
import numpy as np
from mpmath import mp, mpf

import elastic_mp as emp

DPS = 100
mp.dps = DPS

U = 2.0 ** -53
M = 128.0  # snh_mp.M (test_plastic_mp.py holds the two together; snh_mp itself is imported where it is used, so that importing this module does not move it
#            ahead of the mp modules that set another precision)
SENS_SAMPLES = 4
DECIDE = 2.0 ** -40
INF = float("inf")
DENSITY = emp.DENSITY
YM, PR = 1e5, 0.4


def _at_dps(fn):
    """run fn at DPS digits whatever precision the module imported last has left behind (the mp helper modules of this folder set 50 or 100 globally)"""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


def to3(a9):
    """the C ABI's nine doubles of one element -> A[i][j]"""
    return np.asarray(a9, dtype=np.float64).reshape(3, 3).T.copy()


def to9(A):
    return np.asarray(A, dtype=np.float64).T.reshape(9).copy()


def rest_A(Xr):
    """restTriInv of a rest shape in doubles (closed-form inverse): the CPU tests' stand-in for what the library computes from the mesh"""
    D = (np.asarray(Xr, dtype=np.float64)[1:] - np.asarray(Xr, dtype=np.float64)[0]).T
    return np.array([np.cross(D[:, (j + 1) % 3], D[:, (j + 2) % 3]) for j in range(3)]) / np.linalg.det(D)


def _m(A):
    return [[v if isinstance(v, mpf) else mpf(float(v)) for v in r] for r in A]


@_at_dps
def deformation(X, A):
    """F = Ds(x) A in mp; X: 4 x 3 (doubles or mp), A: 3 x 3"""
    P = [[v if isinstance(v, mpf) else mpf(float(v)) for v in p] for p in X]
    return emp._mul(emp._edges(P), _m(A))


@_at_dps
def hencky(F):
    """(e, Q): e_i = ln(lambda_i) / 2 and the eigenvectors (columns of Q) of C = F^T F"""
    C = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            C[i, j] = sum(F[k][i] * F[k][j] for k in range(3))
    ev, Q = mp.eigsy(C)
    return [mp.log(ev[k]) / 2 for k in range(3)], Q


@_at_dps
def strain_norm(X, A):
    """n, or None where det F <= 0"""
    F = deformation(X, A)
    if emp._det(F) <= 0:
        return None
    e, _ = hencky(F)
    m = sum(e) / 3
    return mp.sqrt(sum((v - m) ** 2 for v in e))


@_at_dps
def flow(X, A, yld, creep, harden, alpha, dt):
    """(A', alpha', n, yielded): A' a 3 x 3 list of mpf; n is None where the element is skipped (det F <= 0) and where plasticity is off"""
    Am, alpha = _m(A), (alpha if isinstance(alpha, mpf) else mpf(float(alpha)))
    if not float(yld) < INF:
        return Am, alpha, None, False
    F = deformation(X, Am)
    if emp._det(F) <= 0:
        return Am, alpha, None, False
    e, Q = hencky(F)
    m = sum(e) / 3
    d = [v - m for v in e]
    n = mp.sqrt(sum(v * v for v in d))
    K = mpf(float(harden))
    y = mpf(float(yld)) + K * alpha
    if n <= y:
        return Am, alpha, n, False
    r = mpf(1) if float(creep) == INF else -mp.expm1(-mpf(float(creep)) * mpf(float(dt)))
    Delta = r * (n - y) / (1 + K)
    g = [mp.exp(-Delta * v / n) for v in d]
    G = [[sum(Q[i, k] * g[k] * Q[j, k] for k in range(3)) for j in range(3)] for i in range(3)]
    return emp._mul(Am, G), alpha + Delta, n, True


@_at_dps
def flow_G(X, A, yld, creep, harden, alpha, dt):
    """G alone (identity where nothing flows): for the properties of the reference"""
    A1 = flow(X, A, yld, creep, harden, alpha, dt)[0]
    return emp._mul(emp._inv(_m(A)), A1)


def _signs(seed, n):
    return np.where(np.random.default_rng(seed).integers(0, 2, size=n).astype(bool), 1, -1)


@_at_dps
def reference(case, A=None, seed=0):
    """the flow of one case from the doubles (X, A, parameters), with the tolerances: dict A1, alpha1 (doubles), n, y (doubles; n NaN where skipped or off),
    yielded, decided, tolA (3 x 3), tolAlpha, and the mp values A1_mp, alpha1_mp"""
    A = np.asarray(case["A"] if A is None else A, dtype=np.float64)
    X = np.asarray(case["X"], dtype=np.float64)
    par = (case["yield"], case["creep"], case["harden"], case["alpha"], case["dt"])
    A1, al1, n, yielded = flow(X, A, *par)
    u = mpf(U)
    sensA, sensAl = np.zeros((3, 3)), 0.0
    for k in range(SENS_SAMPLES):
        s = _signs(7000 + 100 * seed + k, 21)
        Xp = [[mpf(float(X[a][i])) * (1 + int(s[3 * a + i]) * u) for i in range(3)] for a in range(4)]
        Ap = [[mpf(float(A[i][j])) * (1 + int(s[12 + 3 * i + j]) * u) for j in range(3)] for i in range(3)]
        B1, bl1, _, _ = flow(Xp, Ap, *par)
        sensA = np.maximum(sensA, np.array([[float(abs(B1[i][j] - A1[i][j])) for j in range(3)] for i in range(3)]))
        sensAl = max(sensAl, float(abs(bl1 - al1)))
    y = float(case["yield"]) + float(case["harden"]) * float(case["alpha"])
    emax = 0.0
    if n is not None:
        emax = float(max(abs(v) for v in hencky(deformation(X, A))[0]))
    nf = float(n) if n is not None else float("nan")
    return dict(A1=np.array([[float(v) for v in r] for r in A1]), alpha1=float(al1), n=nf, y=y, yielded=yielded, skipped=n is None and float(case["yield"]) < INF,
                decided=n is None or abs(nf - y) > DECIDE, tolA=M * (sensA + U * np.abs(A).max()), tolAlpha=M * (sensAl + U * (float(case["alpha"]) + (nf if n is not None else 0.0) + emax)),
                A1_mp=A1, alpha1_mp=al1)


# ---- the float64 restatement: the route of the kernel (SVD of F, logarithms, V diag V^T, A G) in numpy, none of its code ------------------------------------
def flow_np(X, A, yld, creep, harden, alpha, dt):
    """(A', alpha', n, yielded) in plain doubles"""
    X, A = np.asarray(X, dtype=np.float64), np.asarray(A, dtype=np.float64)
    if not yld < INF:
        return A.copy(), alpha, float("nan"), False
    F = (X[1:] - X[0]).T @ A
    if not np.linalg.det(F) > 0.0:
        return A.copy(), alpha, float("nan"), False
    _, s, Vt = np.linalg.svd(F)
    e = np.log(s)
    d = e - ((e[0] + e[1]) + e[2]) / 3.0
    n = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    y = yld + harden * alpha
    if not n > y:
        return A.copy(), alpha, n, False
    r = -np.expm1(-creep * dt)
    Delta = r * (n - y) / (1.0 + harden)
    G = (Vt.T * np.exp(-Delta / n * d)) @ Vt
    return A @ G, alpha + Delta, n, True


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _case(name, F, rest_kind="unit", rot=None, yld=0.05, creep=INF, harden=0.0, alpha=0.0, dt=0.01):
    Xr, _ = emp.rest_shape(rest_kind)
    F = np.asarray(F, dtype=np.float64)
    if F.ndim == 1:
        F = np.diag(F)
    if rot is not None:
        F = emp._rot(rot) @ F
        name += ", rotated"
    X = Xr @ F.T
    return dict(name=name, Xr=Xr, X=X, A=rest_A(Xr), **{"yield": float(yld)}, creep=float(creep), harden=float(harden), alpha=float(alpha), dt=float(dt))


@_at_dps
def cases():
    out = []

    def add(name, F, **kw):
        out.append(_case(name, F, **kw))
        out.append(_case(name, F, rot=200 + len(out), **kw))
    add("general stretch", (1.3, 0.95, 0.8))
    add("general stretch, sliver rest shape", (1.3, 0.95, 0.8), rest_kind="sliver")
    add("uniaxial stretch (two equal stretches)", (1.4, 1.0, 1.0))
    add("uniaxial compression (the larger two equal)", (1.0, 1.0, 0.7))
    add("pure dilation", (1.2, 1.2, 1.2))
    add("pure dilation, yield 0", (1.2, 1.2, 1.2), yld=0.0)
    add("rest, yield 0", (1.0, 1.0, 1.0), yld=0.0)
    add("simple shear", [[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    add("below yield", (1.03, 1.0, 0.98))
    add("inverted", (1.2, 0.9, -0.5))
    add("inverted, sliver rest shape", (1.2, 0.9, -0.5), rest_kind="sliver")
    add("finite creep, dt 0.01", (1.3, 0.95, 0.8), creep=5.0, dt=0.01)
    add("finite creep, dt 0.1", (1.3, 0.95, 0.8), creep=5.0, dt=0.1)
    add("hardening from alpha 0.1", (1.3, 0.95, 0.8), harden=0.5, alpha=0.1)
    add("hardening keeps it elastic", (1.1, 1.0, 0.95), harden=2.0, alpha=0.1)
    add("creep and hardening", (0.8, 1.25, 1.1), creep=20.0, dt=0.025, harden=0.25, alpha=0.03)
    add("switched off", (1.3, 0.95, 0.8), yld=INF)
    # n just below and just above y, one ulp apart in the stretch: y lies between the two norms
    lo, hi = 1.3, float(np.nextafter(1.3, 2.0))
    nl, nh = (strain_norm(emp.UNIT @ np.diag((s, 1.0, 1.0)), np.eye(3)) for s in (lo, hi))
    y = float((nl + nh) / 2)
    assert nl < mpf(y) < nh
    out.append(_case("one ulp below the yield surface", (lo, 1.0, 1.0), yld=y))
    out.append(_case("one ulp above the yield surface", (hi, 1.0, 1.0), yld=y))
    return out


# ---- the energy after a flow (test_gpu_plastic_mp.py): the stable neo-Hookean energy of snh_mp at F = Ds(x) A' -----------------------------------------------
@_at_dps
def snh_energy(X, A, vol):
    """(E, Escale) in mp: vol psi(F) and the sum of the magnitudes of its terms (as snh_mp.element_reference)"""
    import snh_mp as smp
    muL, lamL = emp.lame(YM, PR)
    mu, lam, alpha, _ = smp.params(muL, lamL)
    F = deformation(X, A)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    E = vol * smp.psi(F, muL, lamL)
    Es = abs(vol) * (mu / 2 * (IC + 3) + lam / 2 * (smp._perm_abs(F) + alpha) ** 2 + mu / 2 * abs(mp.log(IC + 1)) + 9 * mu * mu / (32 * lam) + mu / 2 * mp.log(4))
    return E, Es


@_at_dps
def energy_reference(X, ref, vol, seed=0):
    """(E, tol) of the element after the flow of `ref` (reference()): snh_mp's tolerance M (sens + u scale) at A', plus what tolA propagates -- the change of E
    when each entry of A' moves by its own tolerance, summed"""
    A1 = ref["A1_mp"]
    vol = mpf(float(vol))
    E, Es = snh_energy(X, A1, vol)
    u, sens = mpf(U), mpf(0)
    for k in range(SENS_SAMPLES):
        s = _signs(8000 + 100 * seed + k, 21)
        Xp = [[mpf(float(X[a][i])) * (1 + int(s[3 * a + i]) * u) for i in range(3)] for a in range(4)]
        Ap = [[A1[i][j] * (1 + int(s[12 + 3 * i + j]) * u) for j in range(3)] for i in range(3)]
        sens = max(sens, abs(snh_energy(Xp, Ap, vol)[0] - E))
    prop = mpf(0)
    for i in range(3):
        for j in range(3):
            Ap = [list(r) for r in A1]
            Ap[i][j] += mpf(float(ref["tolA"][i][j]))
            prop += abs(snh_energy(X, Ap, vol)[0] - E)
    return float(E), float(M * (sens + u * Es) + prop)
