"""The time stepper with plastic flow: one tet against a scalar mpmath reference (as test_gpu_snh_step.py::test_one_tet_recovers_from_inversion), a bar stretched
by grips and returned, the status file, and the refusals on a sharded context."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import plastic_mp as pm

pytestmark = pytest.mark.gpu

DT = 0.1
REL_TOL = 1e-5  # (test_gpu_snh_step.py explains why not tighter)
YIELD = 0.05
# the one-tet runs: released from s = 1.6 the node is at 1.063 after the first backward-Euler step of 0.1 (n = sqrt(2/3) ln 1.063 = 0.05 there), so the yield
# strain lies well below that
TET_YIELD = 0.01


@pytest.fixture(autouse=True)
def _precision():
    with mp.workdps(pm.DPS):  # (the mp helper modules of this folder leave 50 or 100 digits behind, whichever was imported last)
        yield


def _one_tet(gpu_lib, yld, creep):
    import snh_mp as smp  # (not at import time: see plastic_mp.M)
    X = smp.UNIT.copy()
    X[3] = (0.0, 0.0, 1.6)  # node 3 pulled out along z, at rest: F = diag(1, 1, 1.6)
    c = gpu_lib.Context(0)
    c.set_mesh(smp.UNIT, np.arange(4, dtype=np.int32).reshape(1, 4), YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    c.set_positions(X)
    c.opt_init(DT, False)  # no gravity; no contact
    c.set_time_integration("BE")
    c.add_dirichlet(np.array([0, 1, 2], dtype=np.int32))  # fixed
    c.set_rel_tol(REL_TOL)
    if yld is not None:
        c.set_plasticity((0, 1), yld, creep)
    return c


def _run_one_tet(gpu_lib, yld, creep, steps):
    """By symmetry the state is (s, a, b): s = z of node 3 and A = diag(a, a, b), so F = diag(a, a, s b).  Per step the reference is the minimiser of
        f(s) = m/2 (s - s~)^2 + dt^2 V psi(diag(a, a, s b)),   s~ = 2 s_n - s_(n-1)   (backward Euler, no gravity; s~ = s_0 in the first step)
    by a scalar Newton solve in mpmath from the run's own positions and its own A, then plastic_mp.flow at the positions the run reached.  The solver stops at
    |p|_inf < targetGRes, and p = f'(s) / h(s) in this 1-D problem, so |s - s*| <= targetGRes h(s) / min f'' + 64 u max(1, |s|) (test_gpu_snh_step.py).
    A and alpha after the step are within plastic_mp's tolerance of the flow of the run's own state."""
    import snh_mp as smp
    c = _one_tet(gpu_lib, yld, creep)
    c.precompute()
    m = mpf(float(c.features()["mass"][3]))
    vol, dt = mpf(1) / 6, mpf(DT)
    muL, lamL = emp.lame(1e5, 0.4)
    target = mpf(REL_TOL) * mp.sqrt(3) * dt
    assert abs(float(target) - c.state()["targetGRes"]) <= 1e-12 * float(target)
    hist = [mpf(1.6), mpf(1.6)]
    A, alpha = pm.to3(c.features()["restTriInv"][0]), 0.0
    assert np.array_equal(A, np.eye(3))
    worst, worstA, last = 0.0, 0.0, None
    for step in range(steps):
        it = c.solve_timestep(200)
        assert it < 200
        V = c.state()["V"]
        assert np.all(V[:3] == smp.UNIT[:3]) and np.all(np.abs(V[3, :2]) <= 1e-13), V
        assert np.all(np.abs(A - np.diag(np.diag(A))) <= 1e-14) and abs(A[0, 0] - A[1, 1]) <= 1e-14
        a, b = mpf(float(A[0, 0])), mpf(float(A[2, 2]))
        F = lambda s: [[a, 0, 0], [0, a, 0], [0, 0, s * b]]
        d1 = lambda s, st: m * (s - st) + dt * dt * vol * smp.piola(F(s), muL, lamL)[2][2] * b
        d2 = lambda s: m + dt * dt * vol * smp.d2psi(F(s), muL, lamL)[8, 8] * b * b
        hproj = lambda s: m + dt * dt * vol * smp.eig_clamp(smp.d2psi(F(s), muL, lamL), 9)[0][8, 8] * b * b
        s = mpf(float(V[3, 2]))
        st = 2 * hist[-1] - hist[-2]
        z = s
        for _ in range(60):
            dz = d1(z, st) / d2(z)
            z -= dz
            if abs(dz) < mpf("1e-60"):
                break
        assert abs(d1(z, st)) < mpf("1e-50") and d2(z) > 0
        curv = min(d2(s), d2(z))
        assert curv > 0
        bound = target * hproj(s) / curv + 64 * smp.U * max(1, abs(s))
        worst = max(worst, float(abs(s - z) / bound))
        assert abs(s - z) <= bound, (step, float(s), float(z), float(bound))
        hist.append(s)
        A1 = pm.to3(c.features()["restTriInv"][0])
        al1 = float(c.plastic_get()["alpha"][0])
        if yld is not None:
            case = {"X": V, "A": A, "yield": yld, "creep": creep, "harden": 0.0, "alpha": alpha, "dt": DT}
            r = pm.reference(case, seed=step)
            worstA = max(worstA, float((np.abs(A1 - r["A1"]) / r["tolA"]).max()) * pm.M)
            assert np.all(np.abs(A1 - r["A1"]) <= r["tolA"]) and abs(al1 - r["alpha1"]) <= r["tolAlpha"], (step, A1, r["A1"])
            assert al1 >= alpha
            last = (float(pm.strain_norm(V, A1)), max(float(abs(v)) for v in pm.hencky(pm.deformation(V, A1))[0]))
        else:
            assert np.array_equal(A1, np.eye(3)) and al1 == 0.0
        A, alpha = A1, al1
    print(f"yield {yld} creep {creep}: s {[round(float(v), 5) for v in hist[1:8]]} ... {float(hist[-1]):.6f}; A = diag({A[0, 0]:.6f}, {A[1, 1]:.6f}, {A[2, 2]:.6f}), alpha {alpha:.6f}; "
          f"worst |s - s*| / bound = {worst:.3g}, worst |A' - ref| / (sens + u scale) = {worstA:.3g}")
    c.close()
    return hist, A, alpha, last


@pytest.mark.parametrize("creep", [pm.INF, 20.0])
def test_one_tet_keeps_a_permanent_stretch(gpu_lib, creep):
    hist, A, alpha, (n, emax) = _run_one_tet(gpu_lib, TET_YIELD, creep, 60)
    # at rest, and not at s = 1: ten times farther from it than the 1e-4 within which the elastic run below comes back (the node swings through its rest
    # position and flows both ways, so what stays is a few 1e-3)
    assert abs(hist[-1] - hist[-2]) <= 1e-4 and abs(hist[-1] - 1) > 1e-3
    assert alpha > 0 and abs(np.linalg.det(A) - 1) <= 60 * pm.M * pm.U
    assert n <= TET_YIELD + pm.M * pm.U * (1 + emax)  # on or inside the yield surface (n from three logarithms of size <= emax)


def test_one_tet_without_plasticity_returns_to_rest(gpu_lib):
    for yld in (None, pm.INF):
        hist, A, alpha, _ = _run_one_tet(gpu_lib, yld, pm.INF, 30)
        assert abs(hist[-1] - 1) <= 1e-4


# ---- a bar stretched by grips and returned ---------------------------------------------------------------------------------------------------------
BAR_DT, BAR_OUT = 0.025, 10


def bar_mesh():
    """1 x 1 x 3 cubes of six tets each (Kuhn's subdivision): 16 nodes, 18 tets"""
    V = np.array([[i, j, k] for k in range(4) for j in range(2) for i in range(2)], dtype=np.float64)
    nid = lambda i, j, k: i + 2 * j + 4 * k
    T = []
    for k in range(3):
        for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            q, tet = [0, 0, 0], [nid(0, 0, k)]
            for ax in p:
                q[ax] = 1
                tet.append(nid(q[0], q[1], k + q[2]))
            D = V[tet[1:]] - V[tet[0]]
            if np.linalg.det(D) < 0:
                tet[2], tet[3] = tet[3], tet[2]
            T.append(tet)
    return V, np.array(T, dtype=np.int32)


def _bar(gpu_lib, plastic):
    """plastic: None (never called), or (yield, creep)"""
    V, T = bar_mesh()
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(BAR_DT, False)
    c.set_time_integration("BE")
    c.add_dirichlet(np.nonzero(V[:, 2] == 0.0)[0].astype(np.int32))
    c.add_dirichlet(np.nonzero(V[:, 2] == 3.0)[0].astype(np.int32), lin_vel=(0.0, 0.0, 0.9 / (BAR_OUT * BAR_DT)))  # 30 % out in BAR_OUT steps
    c.set_rel_tol(1e-7)
    if plastic is not None:
        c.set_plasticity((0, len(T)), *plastic)
    return c, V, T


def _bar_step(c, step):
    if step == BAR_OUT:
        c.set_dirichlet_motion(1, lin_vel=(0.0, 0.0, -0.9 / (BAR_OUT * BAR_DT)))  # and back
    assert c.solve_timestep(200) < 200


def test_switched_off_plasticity_changes_no_bit(gpu_lib, tmp_path):
    runs = []
    for plastic in (None, (pm.INF, pm.INF)):
        c, V, T = _bar(gpu_lib, plastic)
        c.precompute()
        X = []
        for step in range(2 * BAR_OUT):
            _bar_step(c, step)
            X.append(c.state()["V"].copy())
        c.save_status(tmp_path / "status")
        assert "plastic" not in open(tmp_path / "status").read().split()  # the file of a run without a plastic element is what it always was
        runs.append(X)
        c.close()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert abs(runs[0][BAR_OUT - 1][:, 2].max() - 3.9) <= 1e-12 and abs(runs[0][-1][:, 2].max() - 3.0) <= 1e-12


def test_bar_stretched_and_returned(gpu_lib, tmp_path):
    steps, K = 2 * BAR_OUT, 13
    c, V, T = _bar(gpu_lib, (YIELD, pm.INF))
    c.precompute()
    A0 = c.features()["restTriInv"].copy()
    assert np.array_equal(c.plastic_get()["restTriInv0"], A0)
    det = lambda A9: np.array([np.linalg.det(pm.to3(a)) for a in A9])
    alpha = np.zeros(len(T))
    Amax = float(np.abs(A0).max())
    saved = None
    for step in range(steps):
        _bar_step(c, step)
        X = c.state()["V"]
        A, al = c.features()["restTriInv"], c.plastic_get()["alpha"]
        assert np.all(al >= alpha)  # the accumulated plastic strain never decreases
        assert np.array_equal(A[al == 0.0], A0[al == 0.0])  # an element that never yielded has its rest shape to the bit
        assert np.all(np.abs(det(A) / det(A0) - 1) <= (step + 1) * pm.M * pm.U)  # isochoric: one product of determinant 1 per step
        pe, tot = c.plastic_state()
        # r = 1: every element ends the step on or inside the yield surface.  n is recomputed from A', whose entries carry u |A|: through F = Ds A' (|Ds| <= the
        # longest edge, sqrt(3) 1.3) and the logarithms (s_min >= 1/2 here) that is 2 u |A|_max |Ds|_max, times the M of every tolerance of this kernel
        assert np.all(np.isfinite(pe)) and np.all(pe[:, 0] <= pe[:, 1] + 2 * pm.M * pm.U * (1 + 2.3 * float(np.abs(A).max()))), (step, pe)
        assert np.all(pe[:, 1] == YIELD) and np.array_equal(pe[:, 2], al) and tot[1] == 0 and tot[2] == al.max()
        alpha = al.copy()
        if step == K - 1:
            c.save_status(tmp_path / "status")
            txt = open(tmp_path / "status").read().split()
            i = txt.index("plastic")
            assert txt[i + 1:i + 3] == [str(len(T)), "10"] and len(txt) == i + 3 + 10 * len(T) and txt.index("dx_Elastic") < i
        if step == K:
            saved = (X.copy(), A.copy(), al.copy())
    print(f"bar: alpha max {alpha.max():.4f}, {int((alpha > 0).sum())} of {len(T)} elements yielded; length at the end {c.state()['V'][:, 2].max():.3f}")
    assert (alpha > 0).any()
    c.close()
    # a fresh context continues from the file: step K + 1 to the bit
    c2, _, _ = _bar(gpu_lib, (YIELD, pm.INF))
    c2.load_status(tmp_path / "status")
    c2.precompute()
    _bar_step(c2, BAR_OUT)  # (K > BAR_OUT: the grips are on their way back)
    assert np.array_equal(c2.state()["V"], saved[0]) and np.array_equal(c2.features()["restTriInv"], saved[1]) and np.array_equal(c2.plastic_get()["alpha"], saved[2])
    assert np.array_equal(c2.plastic_get()["restTriInv0"], A0)  # the rest shape a reset restores is the mesh's, not the file's
    # a truncated plastic section is refused
    lines = open(tmp_path / "status").read().splitlines()
    open(tmp_path / "cut", "w").write("\n".join(lines[:-3]) + "\n")
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*plastic"):
        c2.load_status(tmp_path / "cut")
    c2.close()


def test_refused_on_a_sharded_context(gpu_lib):
    V, T = bar_mesh()
    E = gpu_lib.IpcGpuError
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=1e5, PR=0.4, density=1000.0)
    c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_plasticity((0, len(T)), YIELD)
    c.close()
    c = gpu_lib.Context(0)
    c.set_mesh(V, T, YM=1e5, PR=0.4, density=1000.0)
    c.set_plasticity((0, len(T)), pm.INF)  # nothing switched on: sharding is still allowed
    c.set_shard(0, 1)
    c.set_plasticity((0, 4), YIELD)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    for bad in ((-1, 4, 0.1, 1.0, 0.0), (0, 19, 0.1, 1.0, 0.0), (0, 4, -0.1, 1.0, 0.0), (0, 4, 0.1, 0.0, 0.0), (0, 4, 0.1, 1.0, -1.0), (0, 4, np.nan, 1.0, 0.0)):
        with pytest.raises(E, match="ipcgpu error -1"):
            c.set_plasticity(bad[:2], *bad[2:])
    assert int(np.sum(c.plastic_get()["yield"] < pm.INF)) == 4  # the refused calls changed nothing
    c.close()
