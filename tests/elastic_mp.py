"""Per-element reference of the elastic energies (neo-Hookean, fixed corotated) and of the inversion step bound in plain mpmath, the hand-placed
cases and their carrier mesh.

A helper module (like stencil_mp.py), used by test_elastic_mp.py, test_gpu_elastic_mp.py and tools/make_elastic_mp_golden.py.  Nothing here shares code
or arithmetic with ipc_amd/ or oracle/: every derived quantity is built in mp (mp.dps = 100) from the exact doubles handed to the GPU.

  A = [X1-X0, X2-X0, X3-X0]^-1    vol = det / 6    mu = YM / (2 (1 + PR))    lam = YM PR / ((1 + PR)(1 - 2 PR))    F = [x1-x0, x2-x0, x3-x0] A
  NH   psi = mu/2 (tr F^T F - 3) - mu ln J + lam/2 (ln J)^2                                   (the form of nh_psi and of the reference's NeoHookeanEnergy)
  FCR  psi = mu sum (s_i - 1)^2 + lam/2 (J - 1)^2 = mu (|F|^2 - 2 sum s_i + 3) + lam/2 (J - 1)^2,  s the singular values, the smallest signed by det F
  energy    E = coef vol psi                  gradient   central differences of E over the 12 coordinates, step 1e-20 x the element's size
  Hessian   central differences of psi(F) give the 9 x 9 d2psi/dF2; it is projected PER ELEMENT and then mapped to 12 x 12 with the shape-function
            gradients (b_{k+1}[j] = A(k, j), b_0 = -sum) and scaled by coef vol; rows and columns of projected Dirichlet nodes are dropped afterwards
  Dirichlet (Mesh.hpp:135-144, Energy.cpp:284-288) the gradient drops every Dirichlet node under projectDBC and none without it; the Hessian drops type 1
            always and type 2 under projectDBC.  Dropped entries are exactly 0.0.

THE PROJECTION.  In the basis U e_i e_j^T V^T (U, V from mp.svd_r, made rotations, the sign on the smallest singular value) the 9 x 9 falls into the 3 x 3
block A3 over (00, 11, 22) and three 2 x 2 blocks over (kk', k'k) -- the module asserts that every other entry vanishes.  A3 is projected with mp.eigsy,
negative eigenvalues clamped.  The 2 x 2 blocks are NOT eigen-projected by the project nor by the code it restates: IglUtils::makePD2d returns, for a block
[[a, b], [b, d]] with eigenvalues L2 < 0 < L1,  v v^T / L1  with v = (L1 - d, b), where the eigen-projection is L1 v v^T / |v|^2 -- for the blocks that occur
(a == d) that is the eigen-projection times 2 b^2 / L1^2.  Parity with that routine is the project's contract, so the reference applies the same RULE in mp
(to second derivatives that still come from differences of psi); where no 2 x 2 block has a negative eigenvalue this equals mp.eigsy on the 9 x 9, which
the module asserts for every such case (`gap`), and the gap of the other cases is stored (up to 0.5 of the block: every compressed element has a negative
twist eigenvalue).  The rule is discontinuous at L2 = 0, which is where every element AT REST OR PURELY ROTATED sits (twist eigenvalue (dE_k + dE_k') /
(s_k + s_k') = 0): there round-off decides the branch, so for blocks with |L2| <= 1e-12 L1 the jump between the two outcomes is added to sens_H.  Those
cases are checked through THE BASIS below, against either outcome.
THE BASIS.  The rule is not invariant under a change of the SVD basis either: with two equal singular values the symmetric mode of their 2 x 2 block and the
mode e_kk - e_k'k' of A3 share an eigenvalue and any rotation in the plane mixes them, but a clamped block rescales the first and not the second.  The
kernel's Jacobi sweep, the oracle's and mp.svd_r pick different bases, so for a case with two singular values within 1e-6 relative AND a clamped block -- and
for the threshold cases -- the ENTRIES of the projected Hessian are arbitrary (`ambiguous`).  What does not depend on the basis is checked instead
(hessian_ratio): the nine eigenvalues of the projected 9 x 9 (the rule assigns one value per mode of an orthonormal basis, whichever basis), read out of the
12 x 12 of a unit rest tet without arithmetic, against the stored spectrum at M (sens + u scale), a threshold block taking either of its two outcomes;
symmetry; the null space of translations.  Every other case is checked entry by entry, and test_elastic_mp.py asserts that no stored tolerance exceeds 1e-6
of its block, so that a check that passes everything cannot come back.
Branches of makePD2d that no placed case can enter: `b2 == 0` needs BL == rc bit for bit; `L1 <= 0` needs x < 1 - s_k s_k' and x > 1 + s_k s_k' (x = lam ln J /
mu) under NH, impossible; it is entered by the FCR case "both block eigenvalues negative".

THE CLAMP.  The kernel divides by 2 max(s_k + s_k', 1e-6) (nh_device.h, Energy.cpp:467-491).  Every case keeps |s_k + s_k'| >= 1e-3 except the two named FCR
cases (s_1 + s_2 = 1e-9 and 2e-7; a negative sum cannot occur: the sign sits on the singular value of smallest magnitude): for them the twist eigenvalue of
the block is replaced by (dpsi/ds_k + dpsi/ds_k') / 1e-6, dpsi/ds by differences of the sigma form of psi, before the rule above.  There the block is
[[a, b], [b, a]] with a ~ -b ~ -5e10 and L1 = a + |b| ~ 1e5: makePD2d forms L1 by that cancellation and divides b^2 by it, so ANY double restatement loses
5e10 / 1e5 u relative, which no perturbation of the inputs shows.  The oracle and the kernel miss alike; the measured ratio of the oracle on these two
Hessians is CLAMP_H_RATIO and they (only they, only H) are held to M_CLAMP_H = 8 x that.

STEP BOUND.  det([v0 + t q0, v1 + t q1, v2 + t q2]) - 0.2 det([v0, v1, v2]) = a t^3 + b t^2 + c t + d (filterStepSize's slackness; the C ABI does not expose
it).  Layer (a) is the algorithm's decision structure in mp: |a| <= 1e-6 falls to the quadratic, there |b| <= 1e-6 to -d/c, the quadratic takes
(-c - sqrt)/(2b) and the other root if that is negative, the cubic takes the smallest positive root with |Im| < 1e-6; the call returns the root when
0 < root < tMax, else tMax.  Layer (b), for cases at unit scale, is the smallest root in (0, tMax) of the full cubic from mp.polyroots.  Cases keep a factor
100 from every threshold of (a) and double roots apart by > 1e-3 relative; there (a) and (b) agree and the module asserts it.  The case at element scale 1e-2
(a = -4e-9: the quadratic path drops a t^3) has layer (a) only.

Carrier mesh: N isolated tets, tet t owns nodes 4t..4t+3, each with its case's own rest shape.  They may overlap in space -- nothing here sees contact -- so no
case is translated and a copy of a case has bit-identical coordinates.  The mesh is created with YM = 0 (every element without stiffness) and each stiff
tet gets its material through set_component_material, which is how the zero-stiffness cases keep mu = lam = 0.

Tolerance of a quantity q of one element:  tol(q) = M (sens(q) + u scale),  u = 2^-53, scale = the largest magnitude in that element's own gradient / block
(before Dirichlet rows are dropped), max(|E|, 3/2 mu vol) for the energy (psi is a sum of terms of size mu/2 tr F^T F >= 3/2 mu that cancel at rest: no double
evaluation of it is better than u times that, and at a rotation E itself is round-off), the bound itself for a step bound; sens(q) = |q_mp(x~) - q_mp(x)| with every input coordinate (rest
and current positions, the search direction) moved by a fixed random +-4 ulp.  M was measured on the CPU against the oracle (Mesh.elastic_energy(per_elem),
elastic_gradient, elastic_hessian_elem, filter_step_size) over all cases of tests/golden/elastic_mp_cases.npz:
    worst err / (sens + u scale) of the oracle = ORACLE_WORST_RATIO below,  M = 8 x that rounded up to a power of two.
tools/make_elastic_mp_golden.py --measure prints the ratios per quantity; test_elastic_mp.py::test_oracle_meets_the_tolerance pins M.  REPLACED lists the cases
whose first placement the oracle missed by more than 100 x the median.
"""
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 100

NH, FCR = 0, 1
ENERGY_NAMES = ("NH", "FCR")
U = 2.0 ** -53
SS_CLAMP = 1.0e-6
SLACKNESS = 0.2
ROOT_TOL = 1.0e-6
ORACLE_WORST_RATIO = 20.0  # measured: E 5.69, gradient 20 (rest edge 1e2), Hessian 17.7, step bound 0.883; medians 0.21, 0.44, 1.17, 0
M = 256.0  # 8 x 20 = 160 rounded up to a power of two
CLAMP_H_RATIO = 5.66e4  # measured: the oracle's ratio on the Hessian of the two cases inside the clamp (both miss alike, see THE CLAMP)
M_CLAMP_H = 2.0 ** 19  # 8 x 5.66e4 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic_mp_cases.npz")
DENSITY = 1000.0
PAIRS = ((0, 1), (1, 2), (2, 0))

REPLACED = {}  # name -> number of re-placements (another rotation seed)


# ---- mp primitives ---------------------------------------------------------------------------------------------------------------------------
def _pts(X):
    return [[mpf(float(v)) for v in p] for p in np.asarray(X, dtype=np.float64).reshape(-1, 3)]


def _det(D):
    return (D[0][0] * (D[1][1] * D[2][2] - D[1][2] * D[2][1]) - D[0][1] * (D[1][0] * D[2][2] - D[1][2] * D[2][0])
            + D[0][2] * (D[1][0] * D[2][1] - D[1][1] * D[2][0]))


def _edges(P):
    """3 x 3, column k = P[k+1] - P[0]"""
    return [[P[k + 1][i] - P[0][i] for k in range(3)] for i in range(3)]


def _inv(D):
    d = _det(D)
    c = lambda i, j: D[(i + 1) % 3][(j + 1) % 3] * D[(i + 2) % 3][(j + 2) % 3] - D[(i + 1) % 3][(j + 2) % 3] * D[(i + 2) % 3][(j + 1) % 3]
    return [[c(j, i) / d for j in range(3)] for i in range(3)]


def _mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def lame(YM, PR):
    YM, PR = mpf(float(YM)), mpf(float(PR))
    return YM / (2 * (1 + PR)), YM * PR / ((1 + PR) * (1 - 2 * PR))


def rest(Xr):
    """(A, vol) of the rest shape"""
    D = _edges(_pts(Xr))
    return _inv(D), _det(D) / 6


def signed_singular_values(F):
    """descending in magnitude, the smallest signed by det F (eigenvalues of F^T F: no vectors involved)"""
    C = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            C[i, j] = sum(F[k][i] * F[k][j] for k in range(3))
    ev = mp.eigsy(C, eigvals_only=True)
    s = sorted((mp.sqrt(max(ev[k], mpf(0))) for k in range(3)), reverse=True)
    if _det(F) < 0:
        s[2] = -s[2]
    return s


def psi_sigma(energy, s, mu, lam):
    J = s[0] * s[1] * s[2]
    if energy == NH:
        return mu / 2 * (s[0] ** 2 + s[1] ** 2 + s[2] ** 2 - 3) - mu * mp.log(J) + lam / 2 * mp.log(J) ** 2
    return mu * sum((x - 1) ** 2 for x in s) + lam / 2 * (J - 1) ** 2


def psi(energy, F, mu, lam):
    if mu == 0 and lam == 0:
        return mpf(0)
    I1 = sum(F[i][j] ** 2 for i in range(3) for j in range(3))
    J = _det(F)
    if energy == NH:
        lJ = mp.log(J)
        return mu / 2 * (I1 - 3) - mu * lJ + lam / 2 * lJ ** 2
    return mu * (I1 - 2 * sum(signed_singular_values(F)) + 3) + lam / 2 * (J - 1) ** 2


def svd_rotations(F):
    """U, s, V with F = U diag(s) V^T, U and V rotations, |s| descending, only s[2] may be negative"""
    Fm = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            Fm[i, j] = F[i][j]
    Um, S, Vt = mp.svd_r(Fm)
    Uu = [[Um[i, j] for j in range(3)] for i in range(3)]
    V = [[Vt[j, i] for j in range(3)] for i in range(3)]
    s = [S[k] for k in range(3)]
    if _det(V) < 0:
        for i in range(3):
            V[i][2], Uu[i][2] = -V[i][2], -Uu[i][2]
    if _det(Uu) < 0:
        for i in range(3):
            Uu[i][2] = -Uu[i][2]
        s[2] = -s[2]
    return Uu, s, V


def pd2d(a, b, d, force_negative=False):
    """the rule of IglUtils::makePD2d; force_negative: the outcome an L2 rounded just below zero would give"""
    b2 = b * b
    T2 = (a + d) / 2
    root = mp.sqrt(T2 * T2 - (a * d - b2))
    L2, L1 = T2 - root, T2 + root
    if not (L2 < 0 or force_negative):
        return a, b, d
    if L1 <= 0:
        return mpf(0), mpf(0), mpf(0)
    if b2 == 0:
        return L1, mpf(0), mpf(0)
    return (L1 - d) / L1 * (L1 - d), b * (L1 - d) / L1, b2 / L1


def _eig_clamp(A, n):
    ev, Q = mp.eigsy(A)
    P = mp.matrix(n, n)
    for k in range(n):
        if ev[k] > 0:
            for i in range(n):
                for j in range(n):
                    P[i, j] += ev[k] * Q[i, k] * Q[j, k]
    return P, sum(1 for k in range(n) if ev[k] < 0)


def d2psi(energy, F, mu, lam, h):
    """9 x 9 (index 3 i + j for F[i][j]) by central differences"""
    def at(*sh):
        G = [list(r) for r in F]
        for k, sgn in sh:
            G[k // 3][k % 3] += sgn * h
        return psi(energy, G, mu, lam)
    H = mp.matrix(9, 9)
    p0 = at()
    up = [at((k, 1)) for k in range(9)]
    dn = [at((k, -1)) for k in range(9)]
    for k in range(9):
        H[k, k] = (up[k] - 2 * p0 + dn[k]) / (h * h)
        for l in range(k + 1, 9):
            H[k, l] = H[l, k] = (at((k, 1), (l, 1)) - at((k, 1), (l, -1)) - at((k, -1), (l, 1)) + at((k, -1), (l, -1))) / (4 * h * h)
    return H


def project_element(energy, F, mu, lam, h):
    """(projected 9 x 9, the same with every on-threshold 2 x 2 block taking the other outcome, the plain eigsy projection, info)"""
    H = d2psi(energy, F, mu, lam, h)
    Uu, s, V = svd_rotations(F)
    T = mp.matrix(9, 9)  # column 3 i + j = vec(U e_i e_j^T V^T)
    for i in range(3):
        for j in range(3):
            for r in range(3):
                for c in range(3):
                    T[3 * r + c, 3 * i + j] = Uu[r][i] * V[c][j]
    Ms = T.T * H * T
    top = max(abs(Ms[i, j]) for i in range(9) for j in range(9))
    kept = {(0, 0), (0, 4), (0, 8), (4, 0), (4, 4), (4, 8), (8, 0), (8, 4), (8, 8)}
    out, alt = mp.matrix(9, 9), mp.matrix(9, 9)
    A3 = mp.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            A3[a, b] = Ms[4 * a, 4 * b]
    P3, negA3 = _eig_clamp(A3, 3)
    for a in range(3):
        for b in range(3):
            out[4 * a, 4 * b] = alt[4 * a, 4 * b] = P3[a, b]
    evA = mp.eigsy(A3, eigvals_only=True)
    info = dict(negA3=negA3, branch=[0, 0, 0], threshold=[False] * 3, s=s, specA=sorted(max(evA[k], mpf(0)) for k in range(3)), specB=[], specBalt=[])
    for n, (k, kp) in enumerate(PAIRS):
        p, q = 3 * k + kp, 3 * kp + k
        kept |= {(p, p), (p, q), (q, p), (q, q)}
        a, b, d = Ms[p, p], Ms[p, q], Ms[q, q]
        assert abs(a - d) <= mpf("1e-30") * top, "block diagonal"
        ss = s[k] + s[kp]
        if ss < SS_CLAMP:  # the kernel's clamp: twist eigenvalue (a - b) = (dE_k + dE_k') / max(ss, 1e-6)
            hs = mpf("1e-25")
            dE = []
            for i in (k, kp):
                sp, sm = list(s), list(s)
                sp[i] += hs
                sm[i] -= hs
                dE.append((psi_sigma(energy, sp, mu, lam) - psi_sigma(energy, sm, mu, lam)) / (2 * hs))
            sym, tw = a + b, (dE[0] + dE[1]) / mpf(SS_CLAMP)
            a = d = (sym + tw) / 2
            b = (sym - tw) / 2
        L1, L2 = (a + d) / 2 + abs(b), (a + d) / 2 - abs(b)
        info["branch"][n] = 0 if L2 >= 0 else (1 if L1 <= 0 else (2 if b == 0 else 3))
        info["threshold"][n] = bool(abs(L2) <= mpf("1e-12") * max(abs(L1), mpf("1e-300")))
        main = (a, b, d) if info["threshold"][n] else pd2d(a, b, d)  # on the threshold the exact value is L2 = 0: not clamped
        other = pd2d(a, b, d, True) if info["threshold"][n] else main
        for dst, (a2, b2_, d2), key in ((out, main, "specB"), (alt, other, "specBalt")):
            dst[p, p], dst[p, q], dst[q, p], dst[q, q] = a2, b2_, b2_, d2
            r2 = mp.sqrt(((a2 - d2) / 2) ** 2 + b2_ ** 2)
            info[key].append([(a2 + d2) / 2 - r2, (a2 + d2) / 2 + r2])
    for i in range(9):
        for j in range(9):
            if (i, j) not in kept:
                assert abs(Ms[i, j]) <= mpf("1e-30") * top, ("sigma-space structure", i, j, Ms[i, j] / top)
    plain, _ = _eig_clamp(H, 9)
    return T * out * T.T, T * alt * T.T, plain, info


def _to12(P9, Bv, w):
    """H[(a, i), (c, r)] = w sum_jl P9[(i, j), (r, l)] b_a[j] b_c[l]"""
    H = [[mpf(0)] * 12 for _ in range(12)]
    for a in range(4):
        for c in range(4):
            for i in range(3):
                for r in range(3):
                    H[3 * a + i][3 * c + r] = w * sum(P9[3 * i + j, 3 * r + l] * Bv[a][j] * Bv[c][l] for j in range(3) for l in range(3))
    return H


def _f(v):
    return np.array([float(x) for x in v])


def element_reference(case, Xr=None, X=None):
    """at coef = 1: E, g (12), H (12 x 12) before any Dirichlet drop, as doubles, with the scales and what the case entered"""
    Xr = case["Xr"] if Xr is None else Xr
    X = case["X"] if X is None else X
    energy = int(case["energy"])
    mu, lam = lame(case["YM"], case["PR"])
    A, vol = rest(Xr)
    y = [c for p in _pts(X) for c in p]
    size = mpf(float(case["size"]))

    def F_of(z):
        return _mul(_edges([z[0:3], z[3:6], z[6:9], z[9:12]]), A)

    def E_of(z):
        return vol * psi(energy, F_of(z), mu, lam)
    E0 = E_of(y)
    h = mpf("1e-20") * size
    g = []
    for i in range(12):
        zp, zm = list(y), list(y)
        zp[i] += h
        zm[i] -= h
        g.append((E_of(zp) - E_of(zm)) / (2 * h))
    floor = mpf("1e-30") * vol * (mu + lam) / size  # below the differences' own noise: exactly zero in exact arithmetic (an element at rest)
    g = [v if abs(v) > floor else mpf(0) for v in g]
    F = F_of(y)
    Bv = [[-(A[0][j] + A[1][j] + A[2][j]) for j in range(3)]] + [[A[k][j] for j in range(3)] for k in range(3)]
    if mu == 0 and lam == 0:
        Z = np.zeros((12, 12))
        return dict(E=0.0, g=np.zeros(12), H=Z, Halt=Z, Escale=0.0, gscale=0.0, Hscale=0.0, gap=0.0, negA3=0, branch=np.zeros(3, int), threshold=np.zeros(3, bool),
                    s=_f(signed_singular_values(F)), specA=np.zeros(3), specB=np.zeros((3, 2)), specBalt=np.zeros((3, 2)), ambiguous=False)
    P9, P9alt, plain, info = project_element(energy, F, mu, lam, mpf("1e-30"))  # (F is dimensionless; 1e-30 keeps truncation and cancellation below 1e-35 down to s = 1e-9)
    H, Halt, Hp = _to12(P9, Bv, vol), _to12(P9alt, Bv, vol), _to12(plain, Bv, vol)
    Hd = np.array([_f(r) for r in H])
    Hscale = float(np.abs(Hd).max())
    gap = float(max(abs(H[i][j] - Hp[i][j]) for i in range(12) for j in range(12))) / Hscale
    clamped = any(b != 0 for b in info["branch"]) or any(info["threshold"]) or any(info["s"][k] + info["s"][kp] < SS_CLAMP for k, kp in PAIRS)
    assert clamped or gap < 1e-25, (case["name"], gap)  # no 2 x 2 block touched: the rule IS the eigen-projection of the 9 x 9
    sv = [abs(v) for v in info["s"]]
    near = any(abs(sv[k] - sv[kp]) <= mpf("1e-6") * sv[k] for k, kp in PAIRS)
    ambiguous = any(info["threshold"]) or (near and any(b != 0 for b in info["branch"]))  # see THE BASIS in the module docstring
    return dict(E=float(E0), g=_f(g), H=Hd, Halt=np.array([_f(r) for r in Halt]), Escale=float(max(abs(E0), vol * mu * 3 / 2)), gscale=float(max(abs(v) for v in g)), Hscale=Hscale, gap=gap,
                negA3=info["negA3"], branch=np.array(info["branch"]), threshold=np.array(info["threshold"]), s=_f(info["s"]),
                specA=_f([vol * v for v in info["specA"]]), specB=np.array([_f([vol * v for v in b]) for b in info["specB"]]),
                specBalt=np.array([_f([vol * v for v in b]) for b in info["specBalt"]]), ambiguous=bool(ambiguous))


def perturbed(X, seed):
    """every coordinate moved by +-4 ulp, the signs fixed by `seed` (zeros stay: they have no ulp to speak of)"""
    X = np.asarray(X, dtype=np.float64)
    up = np.random.default_rng(seed).integers(0, 2, size=X.shape).astype(bool)
    Y = X.copy()
    for _ in range(4):
        Y = np.where(X == 0.0, Y, np.nextafter(Y, np.where(up, np.inf, -np.inf)))
    return Y


def spectrum(r, alt=(False, False, False), pre=""):
    """the nine eigenvalues of the projected 9 x 9 (times vol), ascending; alt[n]: block n takes its other outcome"""
    return np.sort(np.concatenate([r[pre + "specA"]] + [(r[pre + "specBalt"] if alt[n] else r[pre + "specB"])[n] for n in range(3)]))


def evaluate_element(case, seed):
    r = element_reference(case)
    p = element_reference(case, perturbed(case["Xr"], seed), perturbed(case["X"], seed + 1))
    sens = {k: np.abs(np.asarray(p[k]) - np.asarray(r[k])) for k in ("E", "g", "H")}
    sens["S"] = np.abs(spectrum(p) - spectrum(r))
    sens["H"] = sens["H"] + np.abs(r["Halt"] - r["H"])  # the jump of the rule at L2 = 0, for blocks that sit on it
    r.pop("Halt")
    return r, sens


# ---- step bound ------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def step_coefficients(X, P):
    x, p = _pts(X), _pts(P)
    v = [[x[k + 1][i] - x[0][i] for i in range(3)] for k in range(3)]
    q = [[p[k + 1][i] - p[0][i] for i in range(3)] for k in range(3)]

    def det(c0, c1, c2):
        return _dot(c2, _cross(c0, c1))
    a = det(q[0], q[1], q[2])
    b = det(v[0], q[1], q[2]) + det(q[0], v[1], q[2]) + det(q[0], q[1], v[2])
    c = det(q[0], v[1], v[2]) + det(v[0], q[1], v[2]) + det(v[0], v[1], q[2])
    d0 = det(v[0], v[1], v[2])
    return a, b, c, (1 - mpf(SLACKNESS)) * d0, d0


def _formula_roots(a, b, c, d):
    """t1, t2, t3 of the closed form in its own order (principal square and cube roots); at 500 digits: with delta0 ~ 1e-33 b^2 the sum delta1 + sqrt(..) keeps
    none of 100"""
    with mp.workdps(500):
        d0 = b * b - 3 * a * c
        d1 = 2 * b ** 3 - 9 * a * b * c + 27 * a * a * d
        C = mp.cbrt((d1 + mp.sqrt(mp.mpc(d1 * d1 - 4 * d0 ** 3))) / 2)
        if C == 0:
            C = mp.cbrt((d1 - mp.sqrt(mp.mpc(d1 * d1 - 4 * d0 ** 3))) / 2)
        u = [mp.mpc(1), mp.mpc(-0.5, mp.sqrt(3) / 2), mp.mpc(-0.5, -mp.sqrt(3) / 2)]
        ts = [(b + w * C + d0 / (w * C)) / (-3 * a) for w in u]
    return [+z for z in ts], +d0, +d1


def step_layer_a(a, b, c, d):
    """(root or -1, the path taken, the index of the chosen formula root or -1)"""
    tol = mpf(ROOT_TOL)
    if abs(a) <= tol:
        if abs(b) <= tol:
            if c == 0:
                return mpf(-1), "linear", -1  # -d / 0: no finite root
            return -d / c, "linear", -1
        desc = c * c - 4 * b * d
        if desc > 0:
            t = (-c - mp.sqrt(desc)) / (2 * b)
            if t < 0:
                t = (-c + mp.sqrt(desc)) / (2 * b)
            return t, "quadratic", -1
        return mpf(-1), "quadratic", -1
    ts, _, _ = _formula_roots(a, b, c, d)
    t, which = mpf(-1), -1
    for k, z in enumerate(ts):
        if abs(z.imag) < tol and z.real > 0 and (z.real < t or t < 0):
            t, which = z.real, k
    return t, "cubic", which


def step_layer_b(a, b, c, d, tmax):
    """smallest root in (0, tmax) of the polynomial as it is (leading zeros removed), or None"""
    co = [a, b, c, d]
    while co and co[0] == 0:
        co = co[1:]
    if len(co) < 2:
        return None
    r = [z.real for z in mp.polyroots(co, maxsteps=500, extraprec=400) if abs(z.imag) < mpf("1e-60") * max(1, abs(z.real))]
    r = sorted(t for t in r if 0 < t < tmax)
    return r[0] if r else None


def step_reference(case, X=None, P=None, check=True):
    a, b, c, d, d0 = step_coefficients(case["X"] if X is None else X, case["P"] if P is None else P)
    tmax = mpf(float(case["tmax"]))
    t, path, which = step_layer_a(a, b, c, d)
    bound = t if 0 < t < tmax else tmax
    if check and case["layer_b"]:
        tb = step_layer_b(a, b, c, d, tmax)
        assert abs((tb if tb is not None else tmax) - bound) <= mpf("1e-50"), (case["name"], tb, bound)
    return dict(bound=float(bound), root=float(t), path=path, which=which, coef=_f([a, b, c, d]))


def evaluate_step(case, seed):
    r = step_reference(case)
    p = step_reference(case, perturbed(case["X"], seed), perturbed(case["P"], seed + 1), check=False)
    return r, {"bound": abs(p["bound"] - r["bound"])}


def step_valid(case):
    """a factor 100 from every threshold of layer (a), double roots apart by more than 1e-3 relative"""
    a, b, c, d, d0 = step_coefficients(case["X"], case["P"])
    tol = mpf(ROOT_TOL)
    ok = d0 > 0 and (a == 0 or abs(a) <= tol / 100 or abs(a) >= 100 * tol)
    if abs(a) <= tol:
        ok = ok and (b == 0 or abs(b) <= tol / 100 or abs(b) >= 100 * tol)
        return bool(ok)
    ts, _, _ = _formula_roots(a, b, c, d)
    for k, z in enumerate(ts):
        ok = ok and (abs(z.imag) <= tol / 100 or abs(z.imag) >= 100 * tol)
        for w in ts[k + 1:]:
            ok = ok and abs(z - w) > mpf("1e-3") * max(abs(z), abs(w))
    return bool(ok)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
UNIT = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def _rot(seed):
    Q, _ = np.linalg.qr(np.random.default_rng(3000 + seed).normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def rest_shape(kind):
    if kind == "unit":
        return UNIT.copy(), 1.0
    if kind == "edge 1e-3":
        return (UNIT + 0.25) @ _rot(1).T * 1e-3, 1e-3
    if kind == "edge 1e2":
        return (UNIT - 0.5) @ _rot(2).T * 1e2, 1e2
    if kind == "sliver":  # the fourth node 1e-3 above the opposite face
        R = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.9, 0.0], [0.45, 0.3, 1e-3]])
        return R @ _rot(3).T, 1.0
    if kind == "permuted":  # an even permutation of a skewed tet
        R = np.array([[0.1, 0.0, 0.2], [1.1, 0.1, 0.0], [0.0, 0.9, 0.1], [0.2, 0.1, 1.2]])
        return R[[1, 2, 0, 3]], 1.0
    raise KeyError(kind)


def _elem(name, energy, s, rest_kind="unit", YM=1e5, PR=0.4, rots=(None, None), dtype=(0, 0, 0, 0), F=None):
    Xr, size = rest_shape(rest_kind)
    if F is None:
        F = np.diag(np.asarray(s, dtype=np.float64))
        if rots[0] is not None:
            F = _rot(rots[0] + 100 * REPLACED.get(name, 0)) @ F
        if rots[1] is not None:
            F = F @ _rot(rots[1]).T
    X = Xr @ np.asarray(F).T
    return dict(name=f"{ENERGY_NAMES[energy]} {name}", energy=energy, Xr=Xr, X=X, YM=float(YM), PR=float(PR), size=float(size), dtype=np.array(dtype))


def _search_sigma(want, energy, PR, seed):
    """singular values whose sigma-space blocks do what `want(negA3, branches)` asks, by a seeded search over the closed forms (used to FIND a case only: what it
    enters is established in mp and stored)"""
    rng = np.random.default_rng(seed)
    mu, lam = 1.0 / (2 * (1 + PR)), PR / ((1 + PR) * (1 - 2 * PR))
    for _ in range(30000):
        s = np.sort(np.exp(rng.uniform(np.log(0.2), np.log(6.0), 3)))[::-1].copy()
        if energy == FCR and rng.integers(0, 2):
            s[2] = -s[2]
        if min(abs(s[k] + s[kp]) for k, kp in PAIRS) < 0.05 or min(abs(abs(s[k]) - abs(s[kp])) for k, kp in PAIRS) < 0.05:
            continue
        J = s.prod()
        if energy == NH:
            L = np.log(J)
            dE = mu * (s - 1 / s) + lam * L / s
            A3 = np.diag(mu * (1 + 1 / s ** 2) - lam * (L - 1) / s ** 2) + lam * (1 - np.eye(3)) / np.outer(s, s)
            BL = [(mu + (mu - lam * L) / (s[k] * s[kp])) / 2 for k, kp in PAIRS]
        else:
            no = np.array([s[1] * s[2], s[2] * s[0], s[0] * s[1]])
            dE = 2 * mu * (s - 1) + lam * (J - 1) * no
            A3 = np.diag(2 * mu + lam * no ** 2)
            for i in range(3):
                for j in range(3):
                    if i != j:
                        A3[i, j] = lam * (s[3 - i - j] * (J - 1) + no[i] * no[j])
            BL = [mu - lam / 2 * s[3 - k - kp] * (J - 1) for k, kp in PAIRS]
        ev = np.linalg.eigvalsh(A3)
        if np.abs(ev).min() < 0.02 * np.abs(ev).max():
            continue
        br = []
        for n, (k, kp) in enumerate(PAIRS):
            rc = (dE[k] + dE[kp]) / (2 * (s[k] + s[kp]))
            e1, e2 = 2 * BL[n], 2 * rc
            if min(abs(e1), abs(e2)) < 0.02 * max(abs(e1), abs(e2)):
                br = None
                break
            br.append(0 if min(e1, e2) > 0 else (1 if max(e1, e2) < 0 else 3))
        if br is not None and want(int((ev < 0).sum()), br):
            return s
    return None


def element_cases():
    out = []
    for en in (NH, FCR):
        add = lambda name, s, **kw: out.append(_elem(name, en, s, **kw))
        add("F = I", (1, 1, 1))
        add("pure rotation", (1, 1, 1), rots=(11, None))
        add("uniform scale 0.5", (0.5, 0.5, 0.5))
        add("uniform scale 2", (2, 2, 2))
        add("uniform scale 0.5, rotated", (0.5, 0.5, 0.5), rots=(12, None))
        add("two equal singular values", (2, 2, 0.7))
        add("uniform scale 2, rotated", (2, 2, 2), rots=(8, None))
        add("two equal singular values (2, 2, 0.7), rotated", (2, 2, 0.7), rots=(9, 10))
        add("two equal singular values, rotated", (1.5, 0.8, 0.8), rots=(13, 14))
        add("singular values 1e-8 apart", (1.3, 1.3 * (1 + 1e-8), 0.8), rots=(15, 16))
        add("singular values 1e-12 apart", (1.1, 0.7, 0.7 * (1 + 1e-12)), rots=(17, 18))
        add("general", (1.4, 0.9, 0.6), rots=(19, 20))
        add("stretch 10 x", (10, 1.1, 0.9), rots=(21, 22))
        for k in (1, 2, 3):
            pr = 0.45 if (en, k) == (NH, 1) else 0.499
            sv = _search_sigma(lambda n, br, k=k: n == k, en, pr, 40 + k)
            if sv is not None:  # (FCR: a wider search, 0.02 <= |s_i| <= 50 at four Poisson ratios, finds at most two negative eigenvalues)
                add(f"A3 with {k} negative eigenvalue(s)", sv, PR=pr, rots=(23 + k, 27 + k))
        add("no block clamped", _search_sigma(lambda n, br: n == 0 and br == [0, 0, 0], en, 0.4, 50), rots=(31, 32))
        add("twist eigenvalue negative", _search_sigma(lambda n, br: br.count(3) >= 1, en, 0.4, 51), rots=(33, 34))
        add("all three 2 x 2 blocks clamped", _search_sigma(lambda n, br: br == [3, 3, 3], en, 0.4 if en == NH else 0.499, 52), rots=(35, 36), PR=0.4 if en == NH else 0.499)
        # reflection-prone: a rotation by pi about an axis times a stretch, and an F whose polar factor is close to a half turn
        add("half turn about x", (1, 1, 1), F=np.diag([1.3, -0.9, -0.7]))
        add("half turn, rotated", (1, 1, 1), F=_rot(37) @ np.diag([-1.2, 0.8, -0.6]) @ _rot(38).T)
        add("negative diagonal, permuted axes", (1, 1, 1), F=np.array([[0.0, -1.1, 0.0], [0.0, 0.0, -0.8], [1.3, 0.0, 0.0]]))
        for rk in ("edge 1e-3", "edge 1e2", "sliver", "permuted"):
            add(f"rest {rk}", (1.3, 0.9, 0.75), rest_kind=rk, rots=(39, 40))
        for PR in (0.0, 0.4, 0.499):
            for YM in (1e3, 1e9):
                add(f"PR {PR:g} YM {YM:g}", (1.2, 1.05, 0.85), PR=PR, YM=YM, rots=(41, 42))
        add("zero stiffness", (1.2, 0.9, 0.8), YM=0.0, rots=(43, 44))
        n = 0
        for typ in (1, 2):
            for cnt in (1, 2, 3, 4):
                nodes = [(n + k) % 4 for k in range(cnt)]
                add(f"Dirichlet type {typ} on {cnt} node(s)", ((1.3, 0.85, 0.7), (0.9, 0.8, 0.6))[n % 2], dtype=tuple(typ if k in nodes else 0 for k in range(4)), rots=(45 + n, 60 + n))
                n += 1
        add("Dirichlet types 1 and 2 mixed", (1.25, 1.0, 0.7), dtype=(1, 0, 2, 0), rots=(70, 71))
    nh = lambda name, s, **kw: out.append(_elem(name, NH, s, **kw))
    nh("compression to J 1e-2", (1.1, 0.9, 1e-2 / 0.99), rots=(72, 73))
    nh("compression to J 1e-4", (1.1, 0.9, 1e-4 / 0.99), rots=(74, 75))
    nh("compression to J 1e-4, all directions", (0.05, 0.04, 0.05), rots=(76, 77))
    fc = lambda name, s, **kw: out.append(_elem(name, FCR, s, **kw))
    fc("inverted, s_2 -0.5", (1.2, 0.9, -0.5), rots=(78, 79))
    fc("inverted, s_2 -1e-3", (1.2, 0.9, -1e-3), rots=(80, 81))
    fc("inverted, s_2 -0.5, unrotated", (1.2, 0.9, -0.5))
    fc("half turn about x, rotated", (1, 1, 1), F=_rot(97) @ np.diag([1.3, -0.9, -0.7]) @ _rot(98).T)
    nh("half turn about x, rotated", (1, 1, 1), F=_rot(97) @ np.diag([1.3, -0.9, -0.7]) @ _rot(98).T)
    fc("inverted, PR 0.499", (1.1, 0.95, -0.3), PR=0.499, rots=(82, 83))
    fc("both block eigenvalues negative", _search_sigma(lambda n, br: 1 in br, FCR, 0.45, 53), PR=0.45, rots=(84, 85))
    fc("clamp: s_1 + s_2 1e-9", (1.2, 0.5, -0.5 + 1e-9), rots=(86, 87))
    fc("clamp: s_1 + s_2 2e-7", (1.2, 0.5, -0.5 + 2e-7), rots=(88, 89))
    return out


def block_mesh():
    """(rest positions 27 x 3, tets 48 x 4, current positions) of a 2 x 2 x 2 block of cells of edge 0.5, six tets per cell along the cell's diagonal; the
    current state is a smooth, non-affine map of the rest state (every tet has its own F)"""
    idx = lambda i, j, k: (i * 3 + j) * 3 + k
    V = np.array([[0.5 * i, 0.5 * j, 0.5 * k] for i in range(3) for j in range(3) for k in range(3)])
    F = []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                    c, t = [i, j, k], []
                    t.append(idx(*c))
                    for a in perm:
                        c[a] += 1
                        t.append(idx(*c))
                    if np.linalg.det(V[t[1:]] - V[t[0]]) < 0:
                        t[2], t[3] = t[3], t[2]
                    F.append(t)
    x, y, z = V.T
    X = V @ (_rot(95) @ np.diag([1.15, 0.95, 0.85]) @ _rot(96).T).T + 0.06 * np.stack([np.sin(2.0 * y) + z * z, x * z - 0.5 * y * y, np.cos(1.5 * x) * y], axis=1)
    return V, np.array(F, dtype=np.int32), X


def block_cases():
    V, F, X = block_mesh()
    return [dict(name=f"block tet {t}", energy=NH, Xr=V[f].copy(), X=X[f].copy(), YM=1e5, PR=0.4, size=0.5, dtype=np.zeros(4, dtype=int)) for t, f in enumerate(F)]


CLAMP_CASES = ("FCR clamp: s_1 + s_2 1e-9", "FCR clamp: s_1 + s_2 2e-7")


def _step(name, X, P, tmax=1.0, layer_b=True):
    return dict(name=name, X=np.asarray(X, dtype=np.float64), P=np.asarray(P, dtype=np.float64), tmax=float(tmax), layer_b=bool(layer_b))


def _with_root(name, X, P, target, tmax=1.0):
    """P scaled so that the root lands at `target` (the roots of the cubic scale with 1 / |P|)"""
    r = step_reference(_step(name, X, P, 1e30, False), check=False)["root"]
    assert r > 0
    return _step(name, X, P * (r / target), tmax)


def step_cases():
    out = []
    Q = _rot(90)
    X = (UNIT * np.array([1.0, 1.2, 0.9])) @ Q.T + 0.1

    def shrink(al):  # node k+1 moves along its own edge: det(t) = d0 (1 + al0 t)(1 + al1 t)(1 + al2 t)
        P = np.zeros((4, 3))
        P[1:] = (X[1:] - X[0]) * np.asarray(al)[:, None]
        return P
    rng = np.random.default_rng(91)
    out.append(_step("one real root", X, shrink((-1.0, -0.3, 0.2)) + 0.05 * rng.normal(size=(4, 3))))
    found = {}
    for _ in range(400):  # three real roots: which of t1, t2, t3 is the smallest positive one depends on the branch of the cube root
        al = -np.exp(rng.uniform(np.log(0.6), np.log(6.0), 3)) * rng.choice([1.0, 1.0, -0.5], 3)
        c = _step("", X, shrink(al) + 0.02 * rng.normal(size=(4, 3)))
        a, b, cc, d, _ = step_coefficients(c["X"], c["P"])
        if abs(a) < 1e-4 or not step_valid(c):
            continue
        ts, _, _ = _formula_roots(a, b, cc, d)
        if all(abs(z.imag) < mpf("1e-50") for z in ts):
            w = step_layer_a(a, b, cc, d)[2]
            if w >= 0 and w not in found:
                found[w] = c
                c["name"] = f"three real roots, the smallest positive one is t{w + 1}"
        if len(found) == 3:
            break
    assert len(found) == 3, sorted(found)
    out += [found[k] for k in range(3)]
    P = shrink((-1.0, -0.7, 0.0))
    P[3] = P[0]
    out.append(_step("a exactly 0 (planar direction)", X, P))
    P = np.zeros((4, 3))
    P[1] = -(X[1] - X[0]) * 1.5 + 0.1 * (X[2] - X[0])
    out.append(_step("a = b = 0 (one node moves)", X, P))
    out.append(_step("rigid translation: no root", X, np.tile([0.3, -0.2, 0.5], (4, 1))))
    out.append(_step("expansion: no positive root", X, shrink((0.5, 0.7, 0.2))))
    out.append(_step("uniform shrink: delta0 = 0 up to round-off, delta1 < 0", X, shrink((-1.25, -1.25, -1.25))))
    out.append(_step("near-uniform shrink: delta0 small, delta1 < 0", X, shrink((-1.25, -1.25 * (1 + 1e-4), -1.25 * (1 - 2e-4)))))
    base = shrink((-1.0, -0.45, 0.3)) + 0.05 * np.random.default_rng(92).normal(size=(4, 3))
    for tmax in (1.0, 0.3):
        for target, nm in ((1e-6, "1e-6"), (0.5 * tmax, "tMax / 2"), (tmax * (1 - 1e-9), "just below tMax"), (tmax * (1 + 1e-9), "just above tMax")):
            out.append(_with_root(f"root at {nm}, tMax {tmax:g}", X, base, target, tmax))
    out.append(_with_root("root at 0.9, tMax 0.3: outside", X, base, 0.9, 0.3))
    # element scale 1e-2: a = s^3 al0 al1 al2 = -4e-9, b = 4e-4 -- the quadratic path drops a t^3; layer (a) only
    Xs = X * 1e-2
    Ps = np.zeros((4, 3))
    Ps[1:] = (Xs[1:] - Xs[0]) * np.array([-20.0, -20.0, -1e-5])[:, None]
    out.append(_step("element scale 1e-2: the quadratic path", Xs, Ps, 1.0, layer_b=False))
    return out


# ---- the stored file -------------------------------------------------------------------------------------------------------------------------
def reference_seed(i):
    return 7000 + 2 * i


def _triu(H):
    return np.asarray(H)[np.triu_indices(12)]


def untriu(v):
    H = np.zeros((12, 12))
    H[np.triu_indices(12)] = v
    return H + np.triu(H, 1).T


def _eval(job):
    fn, case, seed = job
    return fn(case, seed)


E_IN = ("energy", "Xr", "X", "YM", "PR", "size", "dtype")
E_REF = ("E", "g", "H", "Escale", "gscale", "Hscale", "gap", "negA3", "branch", "threshold", "s", "specA", "specB", "specBalt", "ambiguous")
S_IN = ("X", "P", "tmax", "layer_b")


def _pack_elements(out, pre, elems, seed0, map_fn):
    res = list(map_fn(_eval, [(evaluate_element, c, reference_seed(seed0 + i)) for i, c in enumerate(elems)]))
    for k in E_IN:
        out[pre + k] = np.array([c[k] for c in elems])
    out[pre + "name"] = np.array([c["name"] for c in elems])
    for k in E_REF:
        f = _triu if k == "H" else np.asarray
        out[pre + "ref_" + k] = np.array([f(r[0][k]) for r in res])
    for k in ("E", "g", "H", "S"):
        f = _triu if k == "H" else np.asarray
        out[pre + "sens_" + k] = np.array([f(r[1][k]) for r in res])


def pack(elems, steps, map_fn=map):
    out = {}
    _pack_elements(out, "e_", elems, 0, map_fn)
    Vb, Fb, Xb = block_mesh()
    _pack_elements(out, "b_", block_cases(), 2000, map_fn)
    out["m_V"], out["m_F"], out["m_X"] = Vb, Fb, Xb
    res = list(map_fn(_eval, [(evaluate_step, c, reference_seed(1000 + i)) for i, c in enumerate(steps)]))
    for k in S_IN:
        out["s_" + k] = np.array([c[k] for c in steps])
    out["s_name"] = np.array([c["name"] for c in steps])
    out["s_ref_bound"] = np.array([r[0]["bound"] for r in res])
    out["s_ref_root"] = np.array([r[0]["root"] for r in res])
    out["s_ref_path"] = np.array([r[0]["path"] for r in res])
    out["s_ref_which"] = np.array([r[0]["which"] for r in res])
    out["s_ref_coef"] = np.array([r[0]["coef"] for r in res])
    out["s_sens_bound"] = np.array([float(r[1]["bound"]) for r in res])
    return out


def load(path=GOLDEN, prefix="e_"):
    """the cases of one family ('e_' elements, 's_' step bounds) with their references: a list of dicts"""
    Z = np.load(path)
    keys = [k[len(prefix):] for k in Z.files if k.startswith(prefix)]
    out = []
    for i in range(len(Z[prefix + "name"])):
        c = {k: Z[prefix + k][i] for k in keys}
        c["name"], c["index"] = str(c["name"]), i
        if prefix in ("e_", "b_"):
            c["energy"], c["ref_ambiguous"] = int(c["energy"]), bool(c["ref_ambiguous"])
            for k in ("ref_H", "sens_H"):
                c[k] = untriu(c[k])
        else:
            c["layer_b"], c["ref_path"] = bool(c["layer_b"]), str(c["ref_path"])
        out.append(c)
    return out


# ---- Dirichlet drop, ratios --------------------------------------------------------------------------------------------------------------------
def dropped_nodes(case, projectDBC, newton=False):
    """(local nodes whose gradient entries are dropped, local nodes whose Hessian rows and columns are dropped); newton: the gradient of the whole Newton
    system, which is also cleared on the nodes whose rows are dropped (Optimizer.cpp:3512-3516) -- a type 1 node without projectDBC"""
    t = [int(k) for k in case["dtype"]]
    hn = [k for k in range(4) if t[k] == 1 or (t[k] == 2 and projectDBC)]
    return [k for k in range(4) if (projectDBC and t[k] != 0) or (newton and k in hn)], hn


def expected(case, k, coef=1.0, projectDBC=True, newton=False):
    """(reference, sens) of quantity k at `coef`, the Dirichlet entries dropped"""
    ref, sens = coef * np.array(case["ref_" + k], dtype=np.float64), coef * np.array(case["sens_" + k], dtype=np.float64)
    if k in ("g", "H"):
        for n in dropped_nodes(case, projectDBC, newton)[0 if k == "g" else 1]:
            for a in (ref, sens):
                a[3 * n:3 * n + 3] = 0.0
                if k == "H":
                    a[:, 3 * n:3 * n + 3] = 0.0
    return ref, sens


def scale_of(case, k):
    if k == "bound":
        return float(case["ref_bound"])
    return float(case["ref_" + k + "scale"])


def margin(case, k):
    """M, except for the Hessian of the two cases inside the clamp"""
    return M_CLAMP_H if k == "H" and case["name"] in CLAMP_CASES else M


def tol(case, k, coef=1.0, projectDBC=True, newton=False):
    return margin(case, k) * (expected(case, k, coef, projectDBC, newton)[1] + U * coef * scale_of(case, k))


def ratio(case, k, got, coef=1.0, projectDBC=True, newton=False):
    """worst |got - ref| / (sens + u scale) over the entries of quantity k; an entry that is exactly 0 in the reference with no sens and no scale (a dropped
    Dirichlet row, a zero-stiffness element) must come out exactly 0"""
    if k == "bound":
        ref, sens = float(case["ref_bound"]), float(case["sens_bound"])
    else:
        ref, sens = expected(case, k, coef, projectDBC, newton)
    den = sens + U * coef * scale_of(case, k)
    if k in ("g", "H"):
        for n in dropped_nodes(case, projectDBC, newton)[0 if k == "g" else 1]:
            den[3 * n:3 * n + 3] = 0.0
            if k == "H":
                den[:, 3 * n:3 * n + 3] = 0.0
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))))


def spectrum_ratio(case, H, coef=1.0):
    """for a case whose projected Hessian depends on the SVD basis (THE BASIS): the nine eigenvalues of vol x the projected 9 x 9, read out of the 12 x 12 of a
    UNIT rest tet (dF_ij / dx_{j+1, i} = 1: the rows and columns of nodes 1..3, reordered), against the stored ones; a block on the threshold may take either
    outcome.  Returns the smallest over the outcomes of the worst |eigenvalue - ref| / (sens + u scale)."""
    assert np.all(case["Xr"] == UNIT) and not np.any(case["dtype"])
    idx = [3 * (j + 1) + i for i in range(3) for j in range(3)]
    H = np.asarray(H, dtype=np.float64)
    ev = np.sort(np.linalg.eigvalsh((H[np.ix_(idx, idx)] + H[np.ix_(idx, idx)].T) / 2))
    den = coef * (case["sens_S"] + U * spectrum_scale(case))
    best = np.inf
    th = [bool(t) for t in case["ref_threshold"]]
    for m in range(8):
        alt = [bool(m >> n & 1) for n in range(3)]
        if any(a and not t for a, t in zip(alt, th)):
            continue
        best = min(best, float(np.max(np.abs(ev - coef * spectrum(case, alt, "ref_")) / den)))
    return best


def spectrum_scale(case):
    return float(max(np.abs(case["ref_specA"]).max(), np.abs(case["ref_specB"]).max(), np.abs(case["ref_specBalt"]).max()))


def hessian_ratio(case, H, coef=1.0, projectDBC=True):
    """the measure of a 12 x 12 block: entry by entry, or -- where the entries depend on the SVD basis -- its basis-invariant parts: the spectrum of the 9 x 9,
    symmetry and the null space of translations, each at u x the block's scale"""
    if not case["ref_ambiguous"]:
        return ratio(case, "H", H, coef, projectDBC)
    H = np.asarray(H, dtype=np.float64)
    hs = U * coef * scale_of(case, "H")
    trans = np.abs(H.reshape(12, 4, 3).sum(axis=1)).max() / (4 * hs)  # four entries, each good to u scale
    return max(spectrum_ratio(case, H, coef), float(np.abs(H - H.T).max() / hs), float(trans))


# ---- carrier mesh -----------------------------------------------------------------------------------------------------------------------------
def carrier(lay):
    """(rest positions, tets, current positions) of the layout: lay[t] is an element case; tet t owns nodes 4t..4t+3"""
    V = np.concatenate([c["Xr"] for c in lay])
    X = np.concatenate([c["X"] for c in lay])
    return V, np.arange(4 * len(lay), dtype=np.int32).reshape(-1, 4), X


def configure(m, lay, set_dbc=True):
    """materials and Dirichlet types of the layout on a mesh object (ipc_amd Context or oracle Mesh) that was created with YM = 0"""
    t = 0
    while t < len(lay):  # runs of equal material in one call
        e = t
        while e < len(lay) and lay[e]["YM"] == lay[t]["YM"] and lay[e]["PR"] == lay[t]["PR"]:
            e += 1
        if lay[t]["YM"] > 0:
            m.set_component_material((4 * t, 4 * e), (t, e), DENSITY, float(lay[t]["YM"]), float(lay[t]["PR"]))
        t = e
    if set_dbc:
        for typ in (1, 2):
            ids = [4 * t + k for t, c in enumerate(lay) for k in range(4) if int(c["dtype"][k]) == typ]
            if ids:
                m.set_dbc(np.array(ids, dtype=np.int32), typ)


def mass_mp(Xr_all, n_tets):
    """lumped nodal masses of the carrier mesh in mp, as doubles: density vol / 4 per node of a tet"""
    out = np.zeros(4 * n_tets)
    for t in range(n_tets):
        out[4 * t:4 * t + 4] = float(mpf(DENSITY) * rest(Xr_all[4 * t:4 * t + 4])[1] / 4)
    return out


# ---- the oracle under the same measure ----------------------------------------------------------------------------------------------------------
def oracle_ratios(orc, path=GOLDEN):
    """{quantity: (worst ratio, case, median ratio)} of the oracle over every stored case"""
    rec = {k: [] for k in ("E", "g", "H", "H clamp", "bound")}
    elems = load(path, "e_")
    for en in (NH, FCR):
        lay = [c for c in elems if c["energy"] == en]
        V, F, X = carrier(lay)
        m = orc.Mesh(V, F, YM=0.0, PR=0.4, density=DENSITY)
        m.set_energy_type(ENERGY_NAMES[en])
        configure(m, lay)
        m.set_V(X)
        _, pe = m.elastic_energy(1.0, per_elem=True)
        g = {p: m.elastic_gradient(1.0, projectDBC=p) for p in (True, False)}
        for t, c in enumerate(lay):
            rec["E"].append((ratio(c, "E", pe[t]), c["name"]))
            H = m.elastic_hessian_elem(t, 1.0, True) if c["YM"] > 0 else np.zeros((12, 12))
            for p in (True, False):
                rec["g"].append((ratio(c, "g", g[p][12 * t:12 * t + 12], 1.0, p), c["name"]))
                Hd = np.array(H)
                for n in dropped_nodes(c, p)[1]:
                    Hd[3 * n:3 * n + 3, :] = 0.0
                    Hd[:, 3 * n:3 * n + 3] = 0.0
                rec["H clamp" if c["name"] in CLAMP_CASES else "H"].append((hessian_ratio(c, Hd, 1.0, p), c["name"]))
    for c in load(path, "s_"):
        m = orc.Mesh(c["X"], np.arange(4, dtype=np.int32).reshape(1, 4), YM=1e5, PR=0.4, density=DENSITY)
        rec["bound"].append((ratio(c, "bound", m.filter_step_size(c["P"].reshape(-1), float(c["tmax"]))), c["name"]))
    return {k: max(v) + (float(np.median([r for r, _ in v])),) for k, v in rec.items()}
