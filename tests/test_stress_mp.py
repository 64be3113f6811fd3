"""The mpmath restatement of the Cauchy stress record (tests/stress_mp.py) pinned on what is already pinned -- sigma = J^-1 (dpsi/dF) F^T with dpsi/dF by
central differences of elastic_mp.psi -- plus the properties the closed forms must have, and the stored file tests/golden/stress_cases.npz (expected values,
scales, and the error of a plain float64 NumPy restatement, the baseline of the GPU tolerance of test_gpu_stress.py).  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import stress_mp as smp

CASES = smp.cases()
TRUNC = mpf("1e-25")


def _F(c):
    return smp.deformation_gradient(c["Xr"], c["X"])


def test_cases_are_elastic_mp_cases_plus_the_nan_rule():
    names = [c["name"] for c in CASES]
    assert names[:-1] == [c["name"] for c in emp.element_cases()] and names[-1] == smp.NAN_CASE
    c = CASES[-1]
    assert c["energy"] == smp.NH and emp._det(_F(c)) < 0
    ref, scale = smp.stress_reference(c)
    assert np.all(np.isnan(ref)) and np.all(np.isnan(scale))
    assert np.all(np.isnan(smp.stress_numpy(c)))


@pytest.mark.parametrize("energy", (smp.NH, smp.FCR), ids=emp.ENERGY_NAMES)
def test_closed_forms_against_differences_of_psi(energy):
    """every stiff case with a stress: the six entries against J^-1 (dpsi/dF) F^T, and the formulas' exact symmetry"""
    n = 0
    for c in CASES:
        mu, lam = emp.lame(c["YM"], c["PR"])
        if c["energy"] != energy or (mu == 0 and lam == 0) or c["name"] == smp.NAN_CASE:
            continue
        F = _F(c)
        rec, scale, asym = smp.stress_of_F(energy, F, mu, lam)
        fd = smp.stress_by_differences(energy, F, mu, lam)
        top = max(scale[:6])
        for k in range(6):
            assert abs(rec[k] - fd[k]) <= TRUNC * top, (c["name"], smp.COMPONENTS[k], rec[k], fd[k])
        assert asym <= mpf("1e-80"), (c["name"], asym)
        n += 1
    assert n >= 40


def _rational_rotation():
    """the rotation of the quaternion (1, 2, 3, 4) / sqrt(30): every entry a multiple of 1 / 30"""
    w, x, y, z = (mpf(v) for v in (1, 2, 3, 4))
    n = w * w + x * x + y * y + z * z
    return [[(w * w + x * x - y * y - z * z) / n, 2 * (x * y - w * z) / n, 2 * (x * z + w * y) / n],
            [2 * (x * y + w * z) / n, (w * w - x * x + y * y - z * z) / n, 2 * (y * z - w * x) / n],
            [2 * (x * z - w * y) / n, 2 * (y * z + w * x) / n, (w * w - x * x - y * y + z * z) / n]]


@pytest.mark.parametrize("energy", (smp.NH, smp.FCR), ids=emp.ENERGY_NAMES)
def test_a_pure_rotation_carries_no_stress(energy):
    mu, lam = emp.lame(1e5, 0.4)
    for F in ([[mpf(int(i == j)) for j in range(3)] for i in range(3)], _rational_rotation()):
        rec, _, _ = smp.stress_of_F(energy, F, mu, lam)
        assert all(abs(v) <= mpf("1e-90") * mu for v in rec[:7]) and abs(rec[7] - 1) <= mpf("1e-95")


@pytest.mark.parametrize("energy", (smp.NH, smp.FCR), ids=emp.ENERGY_NAMES)
def test_small_strain_limit(energy):
    """F = Q (I + d G): sigma -> Q (lam tr eps I + 2 mu eps) Q^T with eps = d sym G, up to O(d^2)"""
    mu, lam = emp.lame(1e5, 0.3)
    G = [[mpf(v) / 8 for v in r] for r in ((3, -2, 1), (5, 1, -4), (2, 2, 2))]
    nG = sum(v * v for r in G for v in r)
    I3 = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    for Q in (I3, _rational_rotation()):
        for d in (mpf("1e-6"), mpf("1e-12")):
            F = emp._mul(Q, [[I3[i][j] + d * G[i][j] for j in range(3)] for i in range(3)])
            eps = [[d * (G[i][j] + G[j][i]) / 2 for j in range(3)] for i in range(3)]
            tr = eps[0][0] + eps[1][1] + eps[2][2]
            lin = [[lam * tr * I3[i][j] + 2 * mu * eps[i][j] for j in range(3)] for i in range(3)]
            Qt = [[Q[j][i] for j in range(3)] for i in range(3)]
            want = emp._mul(emp._mul(Q, lin), Qt)
            rec, _, _ = smp.stress_of_F(energy, F, mu, lam)
            for k, (i, j) in enumerate(smp.PAIRS):
                assert abs(rec[k] - want[i][j]) <= 50 * (mu + lam) * d * d * nG, (d, i, j)
                assert abs(want[i][j]) > 1e3 * (mu + lam) * d * d * nG  # the linear term is what is being checked


def test_element_without_stiffness_and_von_mises_identity():
    c = next(c for c in CASES if c["name"] == "NH zero stiffness")
    ref, scale = smp.stress_reference(c)
    assert np.all(ref[:7] == 0.0) and np.all(scale[:7] == 0.0) and ref[7] > 0.0 and scale[7] > 0.0
    c = next(c for c in CASES if c["name"] == "FCR general")
    mu, lam = emp.lame(c["YM"], c["PR"])
    rec, _, _ = smp.stress_of_F(smp.FCR, _F(c), mu, lam)
    p = (rec[0] + rec[1] + rec[2]) / 3
    dev2 = sum((rec[k] - p) ** 2 for k in range(3)) + 2 * sum(rec[k] ** 2 for k in (3, 4, 5))
    assert abs(rec[6] - mp.sqrt(mpf(3) / 2 * dev2)) <= mpf("1e-90") * rec[6]


def test_stored_file_is_what_the_module_computes_and_holds_the_numpy_baseline():
    """tools/make_stress_mp_golden.py's arrays, recomputed: the same cases, expected values, scales and NumPy ratios; K follows from the stored ratios"""
    Z = np.load(smp.GOLDEN)
    P = smp.pack()
    assert sorted(Z.files) == sorted(P)
    for k in ("name", "energy", "Xr", "X", "YM", "PR", "ref", "scale", "b_ref", "b_scale"):
        assert np.array_equal(Z[k], P[k], equal_nan=k in ("ref", "scale")), k
    assert Z["b_ref"].shape == (2, 48, 8) and np.all(np.isfinite(Z["b_ref"])) and float(Z["b_numpy_ratio"].max()) < 64.0
    # LAPACK's last bits may differ between builds: the recorded ratios are compared loosely, the well-conditioned ones absolutely
    a, b = Z["numpy_ratio"], P["numpy_ratio"]
    assert np.all((np.abs(a - b) <= 64.0) | (np.abs(a - b) <= 0.5 * np.maximum(a, b))), np.abs(a - b).max()
    cs, worst = smp.load()
    for en, nm in ((smp.NH, "NH"), (smp.FCR, "FCR")):
        assert worst[en] == max([c["numpy_ratio"] for c in cs if c["energy"] == en] + list(Z["b_numpy_ratio"][en])) and np.isfinite(worst[en])
        print(f"{nm}: NumPy restatement worst err / (eps scale) = {worst[en]:.4g}, K = {smp.margin(worst[en]):g}")
    assert smp.margin(0.0) == 16.0 and smp.margin(4.0) == 16.0 and smp.margin(4.1) == 32.0 and smp.margin(339.1) == 2048.0
