"""Per-element reference of the Cauchy stress record of `ipcgpu_elastic_stress` (sxx, syy, szz, sxy, syz, sxz, von Mises, J) in plain mpmath, for the
neo-Hookean and the fixed corotated energy, and a plain float64 NumPy restatement of the same formulas.

A helper module (like elastic_mp.py, whose cases, mp primitives and working precision it uses), for test_stress_mp.py, test_gpu_stress.py and
tools/make_stress_mp_golden.py.  Nothing here shares code or arithmetic with ipc_amd/.

  F = [x1-x0, x2-x0, x3-x0] [X1-X0, X2-X0, X3-X0]^-1    J = det F    mu, lam from YM, PR (elastic_mp.lame)    sigma = P F^T / J, P = dpsi/dF
  NH   sigma = (mu (F F^T - I) + lam ln J I) / J
  FCR  sigma = 2 mu (F - R) F^T / J + lam (J - 1) I,   R = U V^T of elastic_mp.svd_rotations (U, V rotations, only the smallest singular value signed)
  von Mises  sqrt(1/2 ((sxx - syy)^2 + (syy - szz)^2 + (szz - sxx)^2) + 3 (sxy^2 + syz^2 + sxz^2))  =  sqrt(3/2 dev sigma : dev sigma)
  mu = lam = 0: zeros and J.    NH with J <= 0: NaN in all eight entries (the element is counted as invalid).

SCALE.  Every output comes with the scale sum |t_i| of the terms t_i its formula adds up, so that `eps * scale` is the size of one rounding of that sum:
  sigma_ij NH    mu F_ik F_jk / J (k = 0..2), and on the diagonal -mu / J and lam ln J / J
  sigma_ij FCR   2 mu F_ik F_jk / J and -2 mu R_ik F_jk / J (k = 0..2), and on the diagonal lam J and -lam; an off-diagonal entry is the mean of (i, j) and
                 (j, i), so its terms are the halves of both
  J              the six products of the determinant
  von Mises      vm is a seminorm of sigma, so |vm(sigma + d) - vm(sigma)| <= vm(d); with |d_k| <= scale_k that is at most
                 sqrt(1/2 ((sxx+syy)^2 + (syy+szz)^2 + (szz+sxx)^2) + 3 (sxy^2 + syz^2 + sxz^2)) of the SCALES; vm itself is added for the rounding of the root
The scale says nothing about the conditioning of F, J or R in the inputs (a sliver rest shape, J = 1e-4, a polar rotation with s_1 + s_2 = 1e-9): what a
straight float64 evaluation loses there is MEASURED, by the NumPy restatement below, and stored with the cases -- the baseline the GPU tolerance is taken from.
"""
import os

import numpy as np
from mpmath import mp, mpf

import elastic_mp as emp

NH, FCR = emp.NH, emp.FCR
EPS = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stress_cases.npz")
COMPONENTS = ("sxx", "syy", "szz", "sxy", "syz", "sxz", "von_mises", "J")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))  # the record's order: VTK's XX YY ZZ XY YZ XZ
NAN_CASE = "NH inverted, s_2 -0.5 (NaN rule)"


def cases():
    """elastic_mp.element_cases() and one NH element with J < 0"""
    out = emp.element_cases()
    c = emp._elem("inverted, s_2 -0.5 (NaN rule)", NH, (1.2, 0.9, -0.5), rots=(78, 79))
    assert c["name"] == NAN_CASE
    return out + [c]


def deformation_gradient(Xr, X):
    A, _ = emp.rest(Xr)
    return emp._mul(emp._edges(emp._pts(X)), A)


def _vm(s):
    return mp.sqrt(((s[0] - s[1]) ** 2 + (s[1] - s[2]) ** 2 + (s[2] - s[0]) ** 2) / 2 + 3 * (s[3] ** 2 + s[4] ** 2 + s[5] ** 2))


def _det_terms(F):
    return [F[0][0] * F[1][1] * F[2][2], -F[0][0] * F[1][2] * F[2][1], -F[0][1] * F[1][0] * F[2][2], F[0][1] * F[1][2] * F[2][0],
            F[0][2] * F[1][0] * F[2][1], -F[0][2] * F[1][1] * F[2][0]]


def stress_of_F(energy, F, mu, lam):
    """(record of 8, scales of 8, asymmetry) in mp; record None for an NH element with J <= 0.  asymmetry: the largest |(i, j) - (j, i)| before the mean, over
    the scale of that entry (exactly symmetric formulas: round-off of the working precision only)"""
    jt = _det_terms(F)
    J, Jscale = sum(jt), sum(abs(t) for t in jt)
    if mu == 0 and lam == 0:
        return [mpf(0)] * 7 + [J], [mpf(0)] * 7 + [Jscale], mpf(0)
    if energy == NH and J <= 0:
        return None, None, mpf(0)
    if energy == FCR:
        Uu, _, V = emp.svd_rotations(F)
        R = [[sum(Uu[i][k] * V[j][k] for k in range(3)) for j in range(3)] for i in range(3)]

    def terms(i, j):
        if energy == NH:
            t = [mu * F[i][k] * F[j][k] / J for k in range(3)]
            return t + ([-mu / J, lam * mp.log(J) / J] if i == j else [])
        t = [2 * mu * F[i][k] * F[j][k] / J for k in range(3)] + [-2 * mu * R[i][k] * F[j][k] / J for k in range(3)]
        return t + ([lam * J, -lam] if i == j else [])
    s, sc, asym = [], [], mpf(0)
    for i, j in PAIRS:
        tij = terms(i, j)
        if i == j:
            s.append(sum(tij))
            sc.append(sum(abs(t) for t in tij))
        else:
            tji = terms(j, i)
            both = [t / 2 for t in tij + tji]
            s.append(sum(both))
            sc.append(sum(abs(t) for t in both))
            asym = max(asym, abs(sum(tij) - sum(tji)) / sc[-1] if sc[-1] > 0 else abs(sum(tij) - sum(tji)))
    vm = _vm(s)
    vmscale = mp.sqrt(((sc[0] + sc[1]) ** 2 + (sc[1] + sc[2]) ** 2 + (sc[2] + sc[0]) ** 2) / 2 + 3 * (sc[3] ** 2 + sc[4] ** 2 + sc[5] ** 2)) + vm
    return s + [vm, J], sc + [vmscale, Jscale], asym


def stress_reference(case):
    """(ref[8], scale[8]) as doubles; NaN in both for the NaN rule"""
    mu, lam = emp.lame(case["YM"], case["PR"])
    rec, sc, _ = stress_of_F(int(case["energy"]), deformation_gradient(case["Xr"], case["X"]), mu, lam)
    if rec is None:
        return np.full(8, np.nan), np.full(8, np.nan)
    return np.array([float(v) for v in rec]), np.array([float(v) for v in sc])


def stress_by_differences(energy, F, mu, lam, h=mpf("1e-30")):
    """sigma = J^-1 (dpsi/dF) F^T with dpsi/dF by central differences of elastic_mp.psi; the six entries in the record's order, each the mean of (i, j) and (j, i).
    h = 1e-30 at 100 digits: the truncation term h^2 psi''' / 6 is below 1e-40 of the stress for every placed case (psi''' <= 1e18 mu at s_1 + s_2 = 1e-9) and the
    cancellation 1e-100 / h = 1e-70"""
    P = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            Gp, Gm = [list(r) for r in F], [list(r) for r in F]
            Gp[i][j] += h
            Gm[i][j] -= h
            P[i][j] = (emp.psi(energy, Gp, mu, lam) - emp.psi(energy, Gm, mu, lam)) / (2 * h)
    J = emp._det(F)
    S = [[sum(P[i][k] * F[j][k] for k in range(3)) / J for j in range(3)] for i in range(3)]
    return [(S[i][j] + S[j][i]) / 2 for i, j in PAIRS]


# ---- the plain float64 restatement ------------------------------------------------------------------------------------------------------------
def stress_numpy(case):
    """the record in straight float64: numpy.linalg.inv for the rest shape, numpy.linalg.det, numpy.linalg.svd for R"""
    Xr, X = np.asarray(case["Xr"], dtype=np.float64), np.asarray(case["X"], dtype=np.float64)
    YM, PR = float(case["YM"]), float(case["PR"])
    mu, lam = YM / 2.0 / (1.0 + PR), YM * PR / (1.0 + PR) / (1.0 - 2.0 * PR)
    F = (X[1:] - X[0]).T @ np.linalg.inv((Xr[1:] - Xr[0]).T)
    J = float(np.linalg.det(F))
    if mu == 0.0 and lam == 0.0:
        return np.array([0.0] * 7 + [J])
    I = np.eye(3)
    if int(case["energy"]) == NH:
        if not J > 0.0:
            return np.full(8, np.nan)
        S = (mu * (F @ F.T - I) + lam * np.log(J) * I) / J
    else:
        U, _, Vt = np.linalg.svd(F)
        if np.linalg.det(U @ Vt) < 0.0:
            U[:, 2] = -U[:, 2]  # the sign goes on the smallest singular value
        S = 2.0 * mu * ((F - U @ Vt) @ F.T) / J + lam * (J - 1.0) * I
    S = (S + S.T) / 2.0
    s = [S[i, j] for i, j in PAIRS]
    vm = np.sqrt(0.5 * ((s[0] - s[1]) ** 2 + (s[1] - s[2]) ** 2 + (s[2] - s[0]) ** 2) + 3.0 * (s[3] ** 2 + s[4] ** 2 + s[5] ** 2))
    return np.array(s + [vm, J])


def ratio(got, ref, scale):
    """worst |got - ref| / (eps scale) over the eight outputs; an output whose scale is 0 (an element without stiffness) must be exactly 0; the NaN rule asks
    for NaN everywhere (ratio 0) and gives inf otherwise"""
    got, ref, scale = (np.asarray(a, dtype=np.float64) for a in (got, ref, scale))
    if np.all(np.isnan(ref)):
        return 0.0 if np.all(np.isnan(got)) else np.inf
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(scale > 0, err / (EPS * scale), np.where(err == 0, 0.0, np.inf))))


def margin(worst_ratio):
    """K of the GPU test: 4 x the NumPy restatement's worst ratio, rounded up to a power of two, at least 16"""
    return 16.0 if 4.0 * worst_ratio <= 16.0 else float(2.0 ** np.ceil(np.log2(4.0 * worst_ratio)))


# ---- the stored file --------------------------------------------------------------------------------------------------------------------------
def pack():
    cs = cases()
    out = {k: np.array([c[k] for c in cs]) for k in ("energy", "Xr", "X", "YM", "PR")}
    out["name"] = np.array([c["name"] for c in cs])
    refs = [stress_reference(c) for c in cs]
    out["ref"] = np.array([r[0] for r in refs])
    out["scale"] = np.array([r[1] for r in refs])
    out["numpy_ratio"] = np.array([ratio(stress_numpy(c), *r) for c, r in zip(cs, refs)])
    # the 48 elements of elastic_mp.block_mesh() under both energies: [energy, element, output]
    blocks = [[dict(c, energy=en) for c in emp.block_cases()] for en in (NH, FCR)]
    brefs = [[stress_reference(c) for c in row] for row in blocks]
    out["b_ref"] = np.array([[r[0] for r in row] for row in brefs])
    out["b_scale"] = np.array([[r[1] for r in row] for row in brefs])
    out["b_numpy_ratio"] = np.array([[ratio(stress_numpy(c), *r) for c, r in zip(row, rr)] for row, rr in zip(blocks, brefs)])
    for en, nm in ((NH, "NH"), (FCR, "FCR")):
        out["numpy_worst_" + nm] = np.array(max([r for r, c in zip(out["numpy_ratio"], cs) if c["energy"] == en] + list(out["b_numpy_ratio"][en])))
    return out


def load_block(path=GOLDEN):
    """(ref[2, 48, 8], scale[2, 48, 8]) of the block mesh's elements, first index the energy"""
    Z = np.load(path)
    return Z["b_ref"], Z["b_scale"]


def load(path=GOLDEN):
    Z = np.load(path)
    cs = []
    for i in range(len(Z["name"])):
        c = {k: Z[k][i] for k in ("energy", "Xr", "X", "YM", "PR", "ref", "scale", "numpy_ratio")}
        c["name"], c["energy"], c["index"] = str(Z["name"][i]), int(c["energy"]), i
        cs.append(c)
    return cs, {NH: float(Z["numpy_worst_NH"]), FCR: float(Z["numpy_worst_FCR"])}
