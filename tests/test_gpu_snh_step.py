"""The time stepper under the stable neo-Hookean energy: one tet recovering from inversion against a scalar mpmath reference, and a block squashed to 20 % of its
height -- states that NH cannot enter."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import snh_mp as smp

pytestmark = pytest.mark.gpu

DT = 0.1
# 1e-3 of the scene default (1e-2): |p|_inf < 1.7e-6 (ipcgpu_opt_set_rel_tol takes the tolerance itself; the stepper squares it into relGL2Tol).  Not tighter: the line
# search accepts a step when the energy does not rise, and a step p changes it by h p^2 / 2 (h >= m = 41.7), which at the inverted start (E = 700) drowns in the
# energy's own rounding, u E = 8e-14, below |p| = sqrt(2 u E / m) = 6e-8; 1e-10 (|p| < 1.7e-11) stalls there for 200 iterations.  1.7e-6 keeps a factor 30 from it.
REL_TOL = 1e-5


def _one_tet(gpu_lib, energy):
    X = smp.UNIT.copy()
    X[3] = (0.0, 0.0, -1.0)  # node 3 reflected through the plane of nodes 0-2: F = diag(1, 1, -1)
    c = gpu_lib.Context(0)
    c.set_mesh(smp.UNIT, np.arange(4, dtype=np.int32).reshape(1, 4), YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type(energy)
    c.set_positions(X)
    c.opt_init(DT, False)  # no gravity; no contact: self-collision is never enabled
    c.set_time_integration("BE")
    c.add_dirichlet(np.array([0, 1, 2], dtype=np.int32))  # fixed
    c.set_rel_tol(REL_TOL)
    return c


def test_one_tet_recovers_from_inversion(gpu_lib):
    """By symmetry the motion is one scalar, s = z of node 3 (F = diag(1, 1, s)).  Per step the reference is the minimiser of
        f(s) = m/2 (s - s~)^2 + dt^2 V psi(diag(1, 1, s)),      s~ = 2 s_n - s_(n-1)  (backward Euler, no gravity; s~ = s_0 in the first step)
    found by a scalar Newton solve in mpmath from the positions the run itself went through.  The solver stops when its Newton direction has |p|_inf <
    targetGRes = relTol bbox dt; in this 1-D problem p = f'(s) / h(s), h the (projected) matrix entry, so |f'(s)| < targetGRes h(s) and
        |s - s*| <= targetGRes h(s) / min f''   (the smaller of f'' at s and at s*: they are 1e-9 apart)   + 64 u max(1, |s|) for the double arithmetic.
    psi has no stationary point at s < 0, so s crosses zero and settles at 1."""
    c = _one_tet(gpu_lib, "SNH")
    c.precompute()
    m = mpf(float(c.features()["mass"][3]))
    assert abs(m - mpf(smp.DENSITY) / 24) <= mpf("1e-15") * m
    vol, dt = mpf(1) / 6, mpf(DT)
    muL, lamL = emp.lame(1e5, 0.4)
    target = mpf(REL_TOL) * mp.sqrt(3) * dt  # sqrt(relTol^2 bbox^2 dt^2); the rest shape's bounding box has diagonal^2 = 3
    assert abs(float(target) - c.state()["targetGRes"]) <= 1e-12 * float(target)
    F = lambda s: [[mpf(1), 0, 0], [0, mpf(1), 0], [0, 0, s]]
    psi = lambda s: smp.psi(F(s), muL, lamL)
    d1 = lambda s, st: m * (s - st) + dt * dt * vol * smp.piola(F(s), muL, lamL)[2][2]
    d2 = lambda s: m + dt * dt * vol * smp.d2psi(F(s), muL, lamL)[8, 8]
    hproj = lambda s: m + dt * dt * vol * smp.eig_clamp(smp.d2psi(F(s), muL, lamL), 9)[0][8, 8]
    # psi' < 0 on s <= 0: the only way to rest is through s = 0
    assert all(smp.piola(F(mpf(x)), muL, lamL)[2][2] < 0 for x in np.linspace(-3.0, 0.0, 61))
    hist = [mpf(-1), mpf(-1)]
    worst, crossed = 0.0, False
    for step in range(30):
        it = c.solve_timestep(200)
        assert it < 200
        V = c.state()["V"]
        assert np.all(V[:3] == smp.UNIT[:3]) and np.all(np.abs(V[3, :2]) <= 1e-13), V
        s = mpf(float(V[3, 2]))
        st = 2 * hist[-1] - hist[-2]
        z = s
        for _ in range(60):  # scalar Newton from the solver's answer: it converges to the stationary point next to it
            dz = d1(z, st) / d2(z)
            z -= dz
            if abs(dz) < mpf("1e-60"):
                break
        assert abs(d1(z, st)) < mpf("1e-50") and d2(z) > 0
        f = lambda x: m / 2 * (x - st) ** 2 + dt * dt * vol * psi(x)
        assert f(z) <= f(hist[-1])  # a descent from the start of the step
        curv = min(d2(s), d2(z))
        assert curv > 0
        bound = target * hproj(s) / curv + 64 * smp.U * max(1, abs(s))
        worst = max(worst, float(abs(s - z) / bound))
        assert abs(s - z) <= bound, (step, float(s), float(z), float(bound))
        crossed = crossed or (hist[-1] < 0 < s)
        hist.append(s)
    print(f"s per step: {[round(float(v), 6) for v in hist[1:12]]} ...; worst |s - s*| / bound = {worst:.3g}")
    assert crossed and hist[-1] > 0 and abs(hist[-1] - 1) <= 1e-4  # settled (each step is within its own bound, ~ targetGRes, of its minimiser); J = s > 0 in the last step
    assert c.check_inversion()
    c.close()


def test_the_same_start_fails_under_nh(gpu_lib):
    """the inverted start has no NH energy (log of a negative J): the run needs SNH"""
    c = _one_tet(gpu_lib, "NH")
    from ipc_amd.lib import IpcGpuError
    failed = False
    try:
        c.precompute()
        failed = not np.isfinite(c.state()["E"])
        if not failed:  # (a start whose energy is not a number is not stepped from)
            c.solve_timestep(50)
            failed = not np.isfinite(c.state()["E"]) or not np.all(np.isfinite(c.state()["V"]))
    except IpcGpuError:
        failed = True
    assert failed
    c.close()


def _squash(gpu_lib):
    """the 48-tet block (27 nodes, edge 1): bottom face fixed, top face moved down so that the block is at 20 % of its height after 10 steps; no contact"""
    Z = np.load(emp.GOLDEN)
    V, F = Z["m_V"], Z["m_F"]
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    c.opt_init(0.025, False)
    bottom = np.nonzero(V[:, 2] == 0.0)[0].astype(np.int32)
    top = np.nonzero(V[:, 2] == 1.0)[0].astype(np.int32)
    assert len(bottom) == 9 and len(top) == 9
    c.add_dirichlet(bottom)
    c.add_dirichlet(top, lin_vel=(0.0, 0.0, -0.8 / (10 * 0.025)))
    c.set_rel_tol(1e-7)  # |p|_inf < 4.3e-9 on positions of size 1 (1e-10 asks for 4e-12, which the round-off of a squashed block's solve does not reach)
    c.precompute()
    energies, states = [], []
    for step in range(10):
        c.begin_timestep()
        E = []
        for _ in range(200):
            done = c.newton_iter()
            E.append(c.state()["E"])
            if done:
                break
        print(f"step {step}: {len(E)} iterations, E {E[0]!r} -> {E[-1]!r}")
        assert done, step
        c.end_timestep()
        energies.append(E)
        states.append(c.state()["V"].copy())
    c.close()
    return V, top, energies, states


def test_block_squashed_to_a_fifth(gpu_lib):
    V, top, energies, states = _squash(gpu_lib)
    for step, E in enumerate(energies):
        assert np.all(np.isfinite(E)) and np.all(np.diff(E) <= 0.0), (step, E)  # every Newton iteration's incremental potential <= the previous one
    for X in states:
        assert np.all(np.isfinite(X))
    assert np.all(np.abs(states[-1][top, 2] - 0.2) <= 1e-12)
    V2, _, energies2, states2 = _squash(gpu_lib)
    assert all(np.array_equal(a, b) for a, b in zip(states, states2)) and energies == energies2  # the same run twice: identical bits
