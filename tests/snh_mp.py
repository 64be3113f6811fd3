"""Per-element reference of the stable neo-Hookean energy (Smith, de Goes, Kim 2018; energy type 2, `SNH`) in plain mpmath, its hand-placed cases and a
float64 NumPy restatement that fixes the tolerance margin.

A helper module (like elastic_mp.py, whose mesh / carrier helpers it reuses), used by test_snh_mp.py, test_gpu_snh_mp.py, test_gpu_snh_stress.py,
test_gpu_snh_step.py and tools/make_snh_mp_golden.py.  Nothing here shares code or arithmetic with ipc_amd/: every quantity is built in mp (mp.dps = 100) from the
exact doubles handed to the GPU.

  mu_L, lam_L  the Lame parameters of the element (elastic_mp.lame);  mu = 4/3 mu_L   lam = lam_L + 5/6 mu_L   alpha = 1 + 3 mu / (4 lam)
  I_C = |F|_F^2   J = det F   c = I_C / (I_C + 1)   k = lam (J - alpha)
  psi = mu/2 (I_C - 3) + lam/2 (J - alpha)^2 - mu/2 log(I_C + 1) - psi0,   psi0 = 9 mu^2 / (32 lam) - mu/2 log 4
  P   = mu c F + k cof F
  d2psi/dF2 = mu c 1 + 2 mu / (I_C + 1)^2 f f^T + lam g g^T + k dcof/dF      f = vec F, g = vec cof F, dcof_ij/dF_rl = eps_irs eps_jlm F_sm   (d2psi)
  sigma space (s the signed singular values, n_i the product of the other two, m the third index of a pair):
      dE_i = mu c s_i + k n_i    A_ii = mu c + 2 mu s_i^2 / (I_C+1)^2 + lam n_i^2    A_ij = 2 mu s_i s_j / (I_C+1)^2 + lam n_i n_j + k s_m
      B_ij = [[mu c, -k s_m], [-k s_m, mu c]],  eigenvalues mu c -+ k s_m on (1, +-1) / sqrt 2
  Cauchy stress  sigma = P F^T / J = mu c F F^T / J + k I
test_snh_mp.py pins each closed form on differentiation of psi (mp.diff) and on each other.

THE PROJECTION.  The sigma-space blocks of this energy are projected by clamping EIGENVALUES (A through the 3 x 3 eigen-solve, the 2 x 2 blocks in closed form),
and the blocks are the matrix of d2psi/dF2 in an orthonormal basis: the projected element matrix IS the eigenvalue clamp of the 9 x 9, a continuous function of F
that does not depend on the basis the SVD picks.  So the reference is mp.eigsy on the analytic 9 x 9 -- no SVD in it -- and every case, equal singular values and
rest included, is compared entry by entry (elastic_mp needs its `ambiguous` class for NH / FCR; here there is none).  project_sigma() builds the same matrix the
kernel's way (SVD, blocks) and test_snh_mp.py asserts that the two agree.

Tolerance of a quantity q of one element:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53.
  sens   |q_mp(x~) - q_mp(x)| with every input coordinate (rest and current positions) moved by ONE ulp, the signs fixed by a seed; the largest of
         SENS_SAMPLES = 4 sign patterns (a single pattern can cancel: the first placement of "rest sliver, inverted" had sens(E) = 0 where other patterns give 1e-12)
  scale  the largest entry of q with every term of its formula replaced by its magnitude (sum of magnitudes: mu c |F| + lam (|J|_abs + alpha) |cof|_abs for P, and
         so on; |J|_abs, |cof|_abs the sums of the absolute products), mapped through |dN/dX| and times vol like q itself.  For E the sum of the magnitudes of
         the terms of psi.  One number per element and quantity: the rotations U, V mix the entries of a block.
  M      measured: the worst err / (sens + u scale) of the float64 NumPy restatement below (numpy_restatement: numpy.linalg.svd / eigh, not the GPU) over every
         stored case, times 8, rounded up to a power of two.  tools/make_snh_mp_golden.py --measure prints the ratios;
         test_snh_mp.py::test_numpy_restatement_meets_the_tolerance pins M.
"""
import os

import numpy as np
from mpmath import mp, mpf

import elastic_mp as emp

mp.dps = 100

SNH = 2
U = 2.0 ** -53
# measured (tools/make_snh_mp_golden.py --measure): worst err / (sens + u scale) of the NumPy restatement  E 1.05 (rest sliver), gradient 1.85 (rest sliver,
# inverted), Hessian 8.63 (block tet 24), stress 1.57 (Dirichlet type 1 on 3 nodes); medians 0.050, 0.10, 1.03, 0.10
NUMPY_WORST_RATIO = 8.63
M = 128.0  # 8 x 8.63 = 69 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snh_mp_cases.npz")
DENSITY = emp.DENSITY
SENS_SAMPLES = 4
PAIRS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))  # (i, j, m)
UNIT = emp.UNIT


# ---- the material in mp ----------------------------------------------------------------------------------------------------------------------
def params(muL, lamL):
    mu = mpf(4) / 3 * muL
    lam = lamL + mpf(5) / 6 * muL
    alpha = 1 + 3 * mu / (4 * lam)
    psi0 = 9 * mu * mu / (32 * lam) - mu / 2 * mp.log(4)
    return mu, lam, alpha, psi0


def cof(F):
    return [[F[(i + 1) % 3][(j + 1) % 3] * F[(i + 2) % 3][(j + 2) % 3] - F[(i + 1) % 3][(j + 2) % 3] * F[(i + 2) % 3][(j + 1) % 3] for j in range(3)] for i in range(3)]


def _abs3(F):
    return [[abs(v) for v in r] for r in F]


def _perm_abs(F):
    """sum of the absolute products of det F"""
    G = _abs3(F)
    return sum(G[0][j] * (G[1][(j + 1) % 3] * G[2][(j + 2) % 3] + G[1][(j + 2) % 3] * G[2][(j + 1) % 3]) for j in range(3))


def _cof_abs(F):
    G = _abs3(F)
    return [[G[(i + 1) % 3][(j + 1) % 3] * G[(i + 2) % 3][(j + 2) % 3] + G[(i + 1) % 3][(j + 2) % 3] * G[(i + 2) % 3][(j + 1) % 3] for j in range(3)] for i in range(3)]


def psi(F, muL, lamL):
    if muL == 0 and lamL == 0:
        return mpf(0)
    mu, lam, alpha, psi0 = params(muL, lamL)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    return mu / 2 * (IC - 3) + lam / 2 * (emp._det(F) - alpha) ** 2 - mu / 2 * mp.log(IC + 1) - psi0


def psi_sigma(s, muL, lamL):
    return psi([[s[0], 0, 0], [0, s[1], 0], [0, 0, s[2]]], muL, lamL)


def piola(F, muL, lamL):
    mu, lam, alpha, _ = params(muL, lamL)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    c, k, C = IC / (IC + 1), lam * (emp._det(F) - alpha), cof(F)
    return [[mu * c * F[i][j] + k * C[i][j] for j in range(3)] for i in range(3)]


def _eps(i, j, k):
    return (i - j) * (j - k) * (k - i) // 2


def d2psi(F, muL, lamL, magnitudes=False):
    """the unprojected 9 x 9, index 3 i + j for F[i][j]; magnitudes: every term replaced by its magnitude"""
    mu, lam, alpha, _ = params(muL, lamL)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    c = IC / (IC + 1)
    if magnitudes:
        k, C, G = lam * (_perm_abs(F) + alpha), _cof_abs(F), _abs3(F)
    else:
        k, C, G = lam * (emp._det(F) - alpha), cof(F), F
    H = mp.matrix(9, 9)
    for i in range(3):
        for j in range(3):
            for r in range(3):
                for l in range(3):
                    d = sum((abs(_eps(i, r, s) * _eps(j, l, m)) if magnitudes else _eps(i, r, s) * _eps(j, l, m)) * G[s][m] for s in range(3) for m in range(3))
                    H[3 * i + j, 3 * r + l] = (mu * c if (i, j) == (r, l) else 0) + 2 * mu / (IC + 1) ** 2 * G[i][j] * G[r][l] + lam * C[i][j] * C[r][l] + k * d
    return H


def sigma_forms(s, muL, lamL):
    """dE (3), A (3 x 3), and per pair (i, j, m) the two eigenvalues (mu c - k s_m, mu c + k s_m) of B_ij"""
    mu, lam, alpha, _ = params(muL, lamL)
    IC = s[0] ** 2 + s[1] ** 2 + s[2] ** 2
    c, k = IC / (IC + 1), lam * (s[0] * s[1] * s[2] - alpha)
    n = [s[1] * s[2], s[2] * s[0], s[0] * s[1]]
    dE = [mu * c * s[i] + k * n[i] for i in range(3)]
    A = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            A[i, j] = 2 * mu * s[i] * s[j] / (IC + 1) ** 2 + lam * n[i] * n[j] + (mu * c if i == j else k * s[3 - i - j])
    return dE, A, [(mu * c - k * s[m], mu * c + k * s[m]) for _, _, m in PAIRS]


def eig_clamp(A, n):
    ev, Q = mp.eigsy(A)
    P = mp.matrix(n, n)
    for k in range(n):
        if ev[k] > 0:
            for i in range(n):
                for j in range(n):
                    P[i, j] += ev[k] * Q[i, k] * Q[j, k]
    return P, [ev[k] for k in range(n)]


def sigma_basis(F):
    """(T, s): column 3 i + j of T = vec(U e_i e_j^T V^T), U, V rotations, the sign on the smallest singular value"""
    Uu, s, V = emp.svd_rotations(F)
    T = mp.matrix(9, 9)
    for i in range(3):
        for j in range(3):
            for r in range(3):
                for c in range(3):
                    T[3 * r + c, 3 * i + j] = Uu[r][i] * V[c][j]
    return T, s


def sigma_matrix(s, muL, lamL, project):
    """the 9 x 9 in the basis of sigma_basis from the closed forms; project: A eigen-clamped, the two eigenvalues of every B clamped at 0"""
    _, A, B = sigma_forms(s, muL, lamL)
    if project:
        A, _ = eig_clamp(A, 3)
    Ms = mp.matrix(9, 9)
    for a in range(3):
        for b in range(3):
            Ms[4 * a, 4 * b] = A[a, b]
    for n, (i, j, m) in enumerate(PAIRS):
        l1, l2 = B[n]
        if project:
            l1, l2 = max(l1, mpf(0)), max(l2, mpf(0))
        p, q = 3 * i + j, 3 * j + i
        Ms[p, p] = Ms[q, q] = (l1 + l2) / 2
        Ms[p, q] = Ms[q, p] = (l1 - l2) / 2
    return Ms


def project_sigma(F, muL, lamL):
    """the projected 9 x 9 built the kernel's way"""
    T, s = sigma_basis(F)
    return T * sigma_matrix(s, muL, lamL, True) * T.T


def cauchy(F, muL, lamL):
    """sxx, syy, szz, sxy, syz, sxz"""
    mu, lam, alpha, _ = params(muL, lamL)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    J = emp._det(F)
    c, k = IC / (IC + 1), lam * (J - alpha)
    S = lambda i, j: mu * c * sum(F[i][q] * F[j][q] for q in range(3)) / J + (k if i == j else 0)
    return [S(0, 0), S(1, 1), S(2, 2), S(0, 1), S(1, 2), S(0, 2)]


def von_mises(s):
    return mp.sqrt(((s[0] - s[1]) ** 2 + (s[1] - s[2]) ** 2 + (s[2] - s[0]) ** 2) / 2 + 3 * (s[3] ** 2 + s[4] ** 2 + s[5] ** 2))


# ---- one element -----------------------------------------------------------------------------------------------------------------------------
def _f(v):
    return np.array([float(x) for x in v])


def _shape(A):
    return [[-(A[0][j] + A[1][j] + A[2][j]) for j in range(3)]] + [[A[k][j] for j in range(3)] for k in range(3)]


def _to12(P9, Bv, w):
    H = [[mpf(0)] * 12 for _ in range(12)]
    for a in range(4):
        for c in range(4):
            for i in range(3):
                for r in range(3):
                    H[3 * a + i][3 * c + r] = w * sum(P9[3 * i + j, 3 * r + l] * Bv[a][j] * Bv[c][l] for j in range(3) for l in range(3))
    return H


def deformation(Xr, X):
    A, vol = emp.rest(Xr)
    return emp._mul(emp._edges(emp._pts(X)), A), A, vol


def element_reference(case, Xr=None, X=None):
    """at coef = 1: E, g (12), H (12 x 12, projected) before any Dirichlet drop, the stress record, as doubles, with the scales and what the case entered"""
    Xr = case["Xr"] if Xr is None else Xr
    X = case["X"] if X is None else X
    muL, lamL = emp.lame(case["YM"], case["PR"])
    F, A, vol = deformation(Xr, X)
    J = emp._det(F)
    if muL == 0 and lamL == 0:
        return dict(E=0.0, g=np.zeros(12), H=np.zeros((12, 12)), S=np.zeros(8) + np.array([0.0] * 7 + [float(J)]), Escale=0.0, gscale=0.0, Hscale=0.0, Sscale=0.0, Jabs=float(_perm_abs(F)), negA=0,
                    clamped=np.zeros(3, bool), psd=True, s=_f(emp.signed_singular_values(F)))
    mu, lam, alpha, psi0 = params(muL, lamL)
    Bv = _shape(A)
    Ba = _abs3(Bv)
    IC = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    c = IC / (IC + 1)
    E = vol * psi(F, muL, lamL)
    Escale = vol * (mu / 2 * (IC + 3) + lam / 2 * (_perm_abs(F) + alpha) ** 2 + mu / 2 * abs(mp.log(IC + 1)) + 9 * mu * mu / (32 * lam) + mu / 2 * mp.log(4))
    P = piola(F, muL, lamL)
    Ca, Fa, ka = _cof_abs(F), _abs3(F), lam * (_perm_abs(F) + alpha)
    g = [vol * sum(P[i][j] * Bv[a][j] for j in range(3)) for a in range(4) for i in range(3)]
    gscale = max(vol * sum((mu * c * Fa[i][j] + ka * Ca[i][j]) * Ba[a][j] for j in range(3)) for a in range(4) for i in range(3))
    H9 = d2psi(F, muL, lamL)
    P9, ev = eig_clamp(H9, 9)
    H = _to12(P9, Bv, vol)
    Hscale = max(max(r) for r in _to12(d2psi(F, muL, lamL, magnitudes=True), Ba, vol))
    s = emp.signed_singular_values(F)
    _, A3, Bev = sigma_forms(s, muL, lamL)
    negA = sum(1 for v in mp.eigsy(A3, eigvals_only=True) if v < 0)
    clamped = [min(b) < 0 for b in Bev]
    if J != 0:
        sg = cauchy(F, muL, lamL)
        S = _f(sg + [von_mises(sg), J])
        Sscale = float(max(mu * c * sum(Fa[i][q] * Fa[j][q] for q in range(3)) / abs(J) + (ka if i == j else 0) for i in range(3) for j in range(3)))
    else:
        S, Sscale = np.full(8, np.nan), 0.0
    return dict(E=float(E), g=_f(g), H=np.array([_f(r) for r in H]), S=S, Escale=float(Escale), gscale=float(gscale), Hscale=float(Hscale), Sscale=Sscale, Jabs=float(_perm_abs(F)),
                negA=int(negA), clamped=np.array(clamped), psd=bool(min(ev) >= 0), s=_f(s))


def perturbed(X, seed):
    """every coordinate moved by one ulp, the signs fixed by `seed` (zeros stay: they have no ulp to speak of)"""
    X = np.asarray(X, dtype=np.float64)
    up = np.random.default_rng(seed).integers(0, 2, size=X.shape).astype(bool)
    return np.where(X == 0.0, X, np.nextafter(X, np.where(up, np.inf, -np.inf)))


def evaluate_element(case, seed):
    r = element_reference(case)
    sens = {k: np.zeros_like(np.asarray(r[k], dtype=np.float64)) for k in ("E", "g", "H", "S")}
    for n in range(SENS_SAMPLES):  # the largest of a few sign patterns: in one pattern the 24 contributions can cancel
        p = element_reference(case, perturbed(case["Xr"], seed + 1000 * n), perturbed(case["X"], seed + 1000 * n + 1))
        sens = {k: np.maximum(sens[k], np.abs(np.asarray(p[k]) - np.asarray(r[k]))) for k in sens}
    return r, sens


# ---- the float64 restatement that fixes M (numpy.linalg, one element at a time; the route of the kernels, none of their code) ----------------------
def numpy_restatement(case):
    Xr, X = np.asarray(case["Xr"], dtype=np.float64), np.asarray(case["X"], dtype=np.float64)
    YM, PR = float(case["YM"]), float(case["PR"])
    det = lambda B: B[0, 0] * (B[1, 1] * B[2, 2] - B[1, 2] * B[2, 1]) - B[0, 1] * (B[1, 0] * B[2, 2] - B[1, 2] * B[2, 0]) + B[0, 2] * (B[1, 0] * B[2, 1] - B[1, 1] * B[2, 0])
    D = (Xr[1:] - Xr[0]).T
    A = np.array([np.cross(D[:, (j + 1) % 3], D[:, (j + 2) % 3]) for j in range(3)]) / det(D)  # the closed-form inverse: cofactors over the determinant
    vol = det(D) / 6
    F = (X[1:] - X[0]).T @ A
    J = det(F)
    if YM == 0.0:
        return dict(E=0.0, g=np.zeros(12), H=np.zeros((12, 12)), S=np.array([0.0] * 7 + [J]))
    muL, lamL = YM / (2 * (1 + PR)), YM * PR / ((1 + PR) * (1 - 2 * PR))
    mu, lam = 4.0 / 3.0 * muL, lamL + 5.0 / 6.0 * muL
    alpha = 1 + 0.75 * mu / lam
    IC = (F * F).sum()
    c, k = IC / (IC + 1), lam * (J - alpha)
    E = vol * (mu / 2 * (IC - 3) + lam / 2 * (J - alpha) ** 2 - mu / 2 * np.log(IC + 1) - (9 * mu * mu / (32 * lam) - mu / 2 * np.log(4.0)))
    C = np.array([np.cross(F[:, (j + 1) % 3], F[:, (j + 2) % 3]) for j in range(3)]).T
    P = mu * c * F + k * C
    Bv = np.vstack([-A.sum(axis=0), A])
    g = (vol * Bv @ P.T).reshape(-1)
    Uu, sv, Vt = np.linalg.svd(F)
    V = Vt.T
    if np.linalg.det(V) < 0:
        V[:, 2], Uu[:, 2] = -V[:, 2], -Uu[:, 2]
    if np.linalg.det(Uu) < 0:
        Uu[:, 2], sv[2] = -Uu[:, 2], -sv[2]
    n = np.array([sv[1] * sv[2], sv[2] * sv[0], sv[0] * sv[1]])
    A3 = 2 * mu / (IC + 1) ** 2 * np.outer(sv, sv) + lam * np.outer(n, n)
    for i in range(3):
        for j in range(3):
            A3[i, j] += mu * c if i == j else k * sv[3 - i - j]
    w, Q = np.linalg.eigh(A3)
    A3 = (Q * np.maximum(w, 0.0)) @ Q.T
    Ms = np.zeros((9, 9))
    Ms[np.ix_([0, 4, 8], [0, 4, 8])] = A3
    for i, j, m in PAIRS:
        l1, l2 = max(mu * c - k * sv[m], 0.0), max(mu * c + k * sv[m], 0.0)
        p, q = 3 * i + j, 3 * j + i
        Ms[p, p] = Ms[q, q] = (l1 + l2) / 2
        Ms[p, q] = Ms[q, p] = (l1 - l2) / 2
    T = np.einsum("ri,cj->rcij", Uu, V).reshape(9, 9)
    P9 = (T @ Ms @ T.T).reshape(3, 3, 3, 3)
    H = vol * np.einsum("ijrl,aj,cl->aicr", P9, Bv, Bv).reshape(12, 12)
    with np.errstate(divide="ignore", invalid="ignore"):
        sg = mu * c * (F @ F.T) / J + k * np.eye(3)
    s6 = np.array([sg[0, 0], sg[1, 1], sg[2, 2], (sg[0, 1] + sg[1, 0]) / 2, (sg[1, 2] + sg[2, 1]) / 2, (sg[0, 2] + sg[2, 0]) / 2])
    vm = np.sqrt(((s6[0] - s6[1]) ** 2 + (s6[1] - s6[2]) ** 2 + (s6[2] - s6[0]) ** 2) / 2 + 3 * (s6[3:] ** 2).sum())
    return dict(E=E, g=g, H=H, S=np.concatenate([s6, [vm, J]]))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def rest_shape(kind):
    if kind == "edge 1e-2":
        return (UNIT + 0.25) @ emp._rot(1).T * 1e-2, 1e-2
    return emp.rest_shape(kind)


def _elem(name, s, rest_kind="unit", YM=1e5, PR=0.4, rots=(None, None), dtype=(0, 0, 0, 0), F=None):
    Xr, size = rest_shape(rest_kind)
    if F is None:
        F = np.diag(np.asarray(s, dtype=np.float64))
        if rots[0] is not None:
            F = emp._rot(rots[0]) @ F
        if rots[1] is not None:
            F = F @ emp._rot(rots[1]).T
    return dict(name="SNH " + name, energy=SNH, Xr=Xr, X=Xr @ np.asarray(F).T, YM=float(YM), PR=float(PR), size=float(size), dtype=np.array(dtype))


def branches(s, PR):
    """float64, for the search only: (number of negative eigenvalues of A, [block (i, j) has a negative eigenvalue], margins) at YM = 1"""
    muL, lamL = 1.0 / (2 * (1 + PR)), PR / ((1 + PR) * (1 - 2 * PR))
    dE, A, B = sigma_forms([mpf(float(v)) for v in s], mpf(muL), mpf(lamL))
    ev = np.linalg.eigvalsh(np.array([[float(A[i, j]) for j in range(3)] for i in range(3)]))
    Bf = np.array([[float(b[0]), float(b[1])] for b in B])
    safe = np.abs(ev).min() > 0.02 * np.abs(ev).max() and np.all(np.abs(Bf).min(axis=1) > 0.02 * np.abs(Bf).max(axis=1))
    return int((ev < 0).sum()), [bool(b.min() < 0) for b in Bf], bool(safe)


def search_sigma(want, PR, seed):
    """singular values whose sigma-space blocks do what `want(negA, clamped)` asks, a factor 50 away from every threshold (used to FIND a case only: what it enters
    is established in mp and stored)"""
    rng = np.random.default_rng(seed)
    for _ in range(5000):
        s = np.sort(np.exp(rng.uniform(np.log(0.2), np.log(4.0), 3)))[::-1].copy()
        if rng.integers(0, 2):
            s[2] = -s[2]
        if min(abs(abs(s[i]) - abs(s[j])) for i, j, _ in PAIRS) < 0.05:
            continue
        nA, cl, safe = branches(s, PR)
        if safe and want(nA, cl):
            return s
    raise AssertionError("no singular values found")


def element_cases():
    out = []
    add = lambda name, s, **kw: out.append(_elem(name, s, **kw))
    add("rest", (1, 1, 1))
    add("pure rotation", (1, 1, 1), rots=(11, None))
    add("general stretch, rotation a", (1.4, 0.9, 0.6), rots=(19, 20))
    add("general stretch, rotation b", (1.4, 0.9, 0.6), rots=(21, 22))
    add("s_2 < 0, one flipped axis", (1.2, 0.9, -0.5), rots=(78, 79))
    add("s_2 < 0, unrotated", (1.2, 0.9, -0.5))
    add("reflection of rest", (1, 1, -1))
    add("reflection of rest, rotated", (1, 1, -1), rots=(80, 81))
    add("flat, J = 0", (1.2, 0.9, 0.0))
    add("flat, J = 0, rotated", (1.2, 0.9, 0.0), rots=(82, 83))
    add("all four nodes at one point, F = 0", (0, 0, 0))
    add("two equal singular values", (2, 2, 0.7), rots=(9, 10))
    add("two equal singular values, the smaller pair", (1.5, 0.8, 0.8), rots=(13, 14))
    add("three equal singular values 0.5", (0.5, 0.5, 0.5), rots=(12, None))
    add("three equal singular values 2", (2, 2, 2), rots=(8, None))
    add("compression to 1e-3", (1.1, 0.9, 1e-3), rots=(72, 73))
    add("compression to 1e-3, all directions", (1e-3, 1e-3, 1e-3), rots=(76, None))
    add("stretch to 1e2", (1e2, 1.1, 0.9), rots=(21, 22))
    add("A indefinite (Jacobi path of make_pd3)", search_sigma(lambda n, cl: n >= 1, 0.4, 40), rots=(24, 28))
    add("A indefinite, PR 0.499", search_sigma(lambda n, cl: n >= 1, 0.499, 41), PR=0.499, rots=(25, 29))
    add("A definite (fast exit of make_pd3)", search_sigma(lambda n, cl: n == 0, 0.4, 42), rots=(26, 30))
    add("a 2 x 2 block clamped", search_sigma(lambda n, cl: any(cl), 0.4, 43), rots=(33, 34))
    add("all three 2 x 2 blocks clamped", search_sigma(lambda n, cl: all(cl), 0.4, 44), rots=(35, 36))
    add("no 2 x 2 block clamped", search_sigma(lambda n, cl: not any(cl), 0.4, 45), rots=(31, 32))
    add("nothing projected", search_sigma(lambda n, cl: n == 0 and not any(cl), 0.4, 46), rots=(37, 38))
    for rk in ("sliver", "edge 1e-2", "edge 1e2", "permuted"):
        add(f"rest {rk}", (1.3, 0.9, 0.75), rest_kind=rk, rots=(39, 40))
    add("rest sliver, inverted", (1.3, 0.9, -0.75), rest_kind="sliver", rots=(39, 40))
    n = 0
    for typ in (1, 2):
        for cnt in (1, 3):
            nodes = [(n + k) % 4 for k in range(cnt)]
            add(f"Dirichlet type {typ} on {cnt} node(s)", ((1.3, 0.85, 0.7), (0.9, 0.8, -0.6))[n % 2], dtype=tuple(typ if k in nodes else 0 for k in range(4)), rots=(45 + n, 60 + n))
            n += 1
    add("Dirichlet types 1 and 2 mixed", (1.25, 1.0, 0.7), dtype=(1, 0, 2, 0), rots=(70, 71))
    add("zero stiffness", (1.2, 0.9, 0.8), YM=0.0, rots=(43, 44))
    add("second material, PR 0.499 YM 1e9", (1.2, 1.05, 0.85), PR=0.499, YM=1e9, rots=(41, 42))
    add("second material, PR 0 YM 1e3", (1.2, 1.05, -0.85), PR=0.0, YM=1e3, rots=(41, 42))
    for k in range(4):
        add(f"general {k}", ((1.1, 1.0, 0.8), (0.9, 0.7, 0.6), (1.6, 1.2, 0.5), (1.3, 0.6, -0.4))[k], rots=(90 + k, 94 + k))
    return out


def block_cases():
    """the 48-tet block of elastic_mp (same rest shape, same state), its elements under SNH"""
    V, F, X = emp.block_mesh()
    return [dict(name=f"SNH block tet {t}", energy=SNH, Xr=V[f].copy(), X=X[f].copy(), YM=1e5, PR=0.4, size=0.5, dtype=np.zeros(4, dtype=int)) for t, f in enumerate(F)]


# ---- the stored file -------------------------------------------------------------------------------------------------------------------------
E_IN = ("energy", "Xr", "X", "YM", "PR", "size", "dtype")
E_REF = ("E", "g", "H", "S", "Escale", "gscale", "Hscale", "Sscale", "Jabs", "negA", "clamped", "psd", "s")
QUANT = ("E", "g", "H", "S")


def _eval(job):
    case, seed = job
    return evaluate_element(case, seed)


def pack(map_fn=map):
    out = {}
    for pre, cases, seed0 in (("e_", element_cases(), 0), ("b_", block_cases(), 2000)):
        res = list(map_fn(_eval, [(c, 9000 + 2 * (seed0 + i)) for i, c in enumerate(cases)]))
        for k in E_IN:
            out[pre + k] = np.array([c[k] for c in cases])
        out[pre + "name"] = np.array([c["name"] for c in cases])
        for k in E_REF:
            f = emp._triu if k == "H" else np.asarray
            out[pre + "ref_" + k] = np.array([f(r[0][k]) for r in res])
        for k in QUANT:
            f = emp._triu if k == "H" else np.asarray
            out[pre + "sens_" + k] = np.array([f(r[1][k]) for r in res])
    return out


def load(path=GOLDEN, prefix="e_"):
    Z = np.load(path)
    keys = [k[len(prefix):] for k in Z.files if k.startswith(prefix)]
    out = []
    for i in range(len(Z[prefix + "name"])):
        c = {k: Z[prefix + k][i] for k in keys}
        c["name"], c["index"], c["energy"] = str(c["name"]), i, int(c["energy"])
        for k in ("ref_H", "sens_H"):
            c[k] = emp.untriu(c[k])
        out.append(c)
    return out


# ---- Dirichlet drop, tolerances, ratios ----------------------------------------------------------------------------------------------------------
dropped_nodes = emp.dropped_nodes


def expected(case, k, coef=1.0, projectDBC=True, newton=False):
    """(reference, sens) of quantity k at `coef`, the Dirichlet entries dropped (the stress carries no coefficient)"""
    ref, sens = coef * np.array(case["ref_" + k], dtype=np.float64), coef * np.array(case["sens_" + k], dtype=np.float64)
    if k in ("g", "H"):
        for n in dropped_nodes(case, projectDBC, newton)[0 if k == "g" else 1]:
            for a in (ref, sens):
                a[3 * n:3 * n + 3] = 0.0
                if k == "H":
                    a[:, 3 * n:3 * n + 3] = 0.0
    return ref, sens


def denominator(case, k, coef=1.0, projectDBC=True, newton=False):
    """sens + u scale per entry; 0 where the entry is dropped (it must then be exactly 0)"""
    den = expected(case, k, coef, projectDBC, newton)[1] + U * coef * float(case["ref_" + k + "scale"])
    if k == "S":
        den[6] = den[:6].max() * 4 + float(case["sens_S"][6])  # von Mises: a root of squares of differences of the six entries
        den[7] = float(case["sens_S"][7]) + U * float(case["ref_Jabs"])  # J: the sum of the absolute products of det F
    if k in ("g", "H"):
        for n in dropped_nodes(case, projectDBC, newton)[0 if k == "g" else 1]:
            den[3 * n:3 * n + 3] = 0.0
            if k == "H":
                den[:, 3 * n:3 * n + 3] = 0.0
    return den


def tol(case, k, coef=1.0, projectDBC=True, newton=False):
    return M * denominator(case, k, coef, projectDBC, newton)


def ratio(case, k, got, coef=1.0, projectDBC=True, newton=False):
    """worst |got - ref| / (sens + u scale) over the entries of quantity k; an entry without sens and scale (a dropped Dirichlet row, a zero-stiffness element) must
    come out exactly 0"""
    ref = expected(case, k, coef, projectDBC, newton)[0]
    den = denominator(case, k, coef, projectDBC, newton)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))))


def stress_checked(case):
    """the stress of a case is compared where it exists: P F^T / J has no value at J = 0 (flat elements, F = 0; a flat element that a rotation leaves at
    J ~ 1e-17 has one, of size 1e22 and with no digit that survives an ulp of the input)"""
    return bool(np.all(np.isfinite(case["ref_S"])) and abs(float(case["ref_S"][7])) > 1e-12 * float(case["ref_Jabs"]) or case["YM"] == 0.0)


def numpy_ratios(path=GOLDEN):
    """{quantity: (worst ratio, case, median)} of numpy_restatement over every stored case"""
    rec = {k: [] for k in QUANT}
    for pre in ("e_", "b_"):
        for c in load(path, pre):
            r = numpy_restatement(c)
            for n in dropped_nodes(c, False)[1]:  # type 1 nodes: their rows and columns of the matrix are dropped whatever projectDBC says
                r["H"][3 * n:3 * n + 3, :] = 0.0
                r["H"][:, 3 * n:3 * n + 3] = 0.0
            for k in QUANT:
                if k == "S" and not stress_checked(c):
                    continue
                rec[k].append((ratio(c, k, r[k], projectDBC=False), c["name"]))
    return {k: max(v) + (float(np.median([x for x, _ in v])),) for k, v in rec.items()}


# ---- carrier mesh (elastic_mp's: tet t owns nodes 4t..4t+3) -----------------------------------------------------------------------------------------
carrier = emp.carrier
configure = emp.configure
mass_mp = emp.mass_mp
