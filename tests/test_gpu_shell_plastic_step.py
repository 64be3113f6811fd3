"""The shells' plastic flow in the time stepper: a fold that stays, a sheet stretched by grips and returned, switched off against never called, the status
round trip, the refusals, and the membrane call that must not wipe a flowed rest shape.  Small meshes, no contact."""
import numpy as np
import pytest

import shell_plastic_mp as spm
from codim_common import step_context

pytestmark = pytest.mark.gpu

INF = float("inf")
PR, RHO = 0.3, 1000.0


# ---- (a) a fold that stays --------------------------------------------------------------------------------------------------------------------------
FOLD_H, FOLD_E, FOLD_DT, FOLD_STEPS, FOLD_START = 0.002, 1e8, 0.01, 60, 1.0


def _fold(gpu_lib, bend_yield):
    """two triangles over one hinge, 0.1 in size; the nodes of the first triangle are fixed, the fourth node starts folded by FOLD_START and is released"""
    Xr, x0 = 0.1 * spm.hinge_rest(0.0), 0.1 * spm.hinge_rest(FOLD_START)
    c = step_context(gpu_lib, Xr, lambda c: c.set_shell(spm.HINGE_TRI, FOLD_H, FOLD_E, PR, RHO, bend_scale=1.0), YM=FOLD_E, density=RHO, dt=FOLD_DT, gravity=False, held=[0, 1, 2], x0=x0)
    c.set_rel_tol(1e-8)
    if bend_yield is not None:
        c.shell_set_plasticity((0, 2), INF, bend_yield)
    c.precompute()
    for _ in range(FOLD_STEPS):
        assert c.solve_timestep(100) < 100
    return c, float(spm.hinge_theta(c.state()["V"]))


def test_a_released_fold_keeps_a_permanent_angle(gpu_lib):
    """g = h w_e / (2 |eBar|) is about 0.04 here, so the fold of 1 rad is an outer-fibre strain of 0.04, ten times the yield strain 0.004.  The flow runs at the
    END of a step: the stiff hinge swings most of the way back within the first step, and the rest angle follows the end-of-step angles while they are more
    than 0.004 / g = 0.1 rad away from it (measured: it settles at 0.124 rad).  The elastic control run of the same set-up swings back to flat; what it leaves
    after the same number of steps (measured: 1e-17) is the measure of `at rest`."""
    ce, residual = _fold(gpu_lib, None)
    ce.close()
    c, angle = _fold(gpu_lib, 0.004)
    g = c.shell_plastic_get()
    _, ph, tot = c.shell_plastic_state()
    print(f"fold: permanent angle {angle:.6f}, thetaBar {g['thetaBar'][0]:.6f}, alphaB {g['alphaB'][0]:.5f}; elastic control residual {residual:.3e}")
    assert abs(angle) > 10 * abs(residual)
    assert abs(angle - g["thetaBar"][0]) <= 10 * abs(residual) + 1e-6 * abs(angle)  # at rest in its new rest angle
    assert g["alphaB"][0] > 0 and ph[0, 3] == g["thetaBar"][0] - g["thetaBar0"][0] and g["thetaBar0"][0] == 0.0
    assert np.array_equal(g["B"], g["B0"]) and np.all(g["alpha"] == 0.0)  # the membrane flow is off
    assert c.shell_get()["restAngle"][0] == 0.0  # ipcgpu_shell_get keeps returning the plan's rest angle
    c.shell_plastic_reset()
    g = c.shell_plastic_get()
    assert g["thetaBar"][0] == 0.0 and g["alphaB"][0] == 0.0
    c.close()


# ---- (b) - (d), (f): a sheet stretched by grips and returned ---------------------------------------------------------------------------------------
NX, NY, SP = 5, 3, 0.1  # 4 x 2 quads
SH_H, SH_E, SH_DT, SH_OUT, YIELD = 0.002, 1e5, 0.025, 10, 0.02


def sheet_mesh():
    V = np.array([[SP * i, 0.0, SP * j] for i in range(NX) for j in range(NY)])
    nid = lambda i, j: NY * i + j
    tri = [t for i in range(NX - 1) for j in range(NY - 1) for t in ((nid(i, j), nid(i, j + 1), nid(i + 1, j)), (nid(i + 1, j), nid(i, j + 1), nid(i + 1, j + 1)))]
    return V, np.array(tri, dtype=np.int32)


def _sheet(gpu_lib, plastic):
    """plastic: None (never called), or (yield, bendYield, creep, harden)"""
    V, tri = sheet_mesh()
    c = step_context(gpu_lib, V, lambda c: c.set_shell(tri, SH_H, SH_E, PR, RHO, bend_scale=1.0), YM=SH_E, density=RHO, dt=SH_DT, gravity=False)
    c.add_dirichlet(np.arange(NY, dtype=np.int32))
    c.add_dirichlet(np.arange(NY * (NX - 1), NY * NX, dtype=np.int32), lin_vel=(0.3 * SP * (NX - 1) / (SH_OUT * SH_DT), 0.0, 0.0))  # 30 % out in SH_OUT steps
    c.set_rel_tol(1e-7)
    if plastic is not None:
        c.shell_set_plasticity((0, len(tri)), *plastic)
    return c, V, tri


def _sheet_step(c, step):
    if step == SH_OUT:
        c.set_dirichlet_motion(1, lin_vel=(-0.3 * SP * (NX - 1) / (SH_OUT * SH_DT), 0.0, 0.0))  # and back
    assert c.solve_timestep(200) < 200


def test_switched_off_plasticity_changes_no_bit(gpu_lib, tmp_path):
    runs = []
    for plastic in (None, (INF, INF, INF, 0.0)):
        c, V, tri = _sheet(gpu_lib, plastic)
        c.precompute()
        X = []
        for step in range(2 * SH_OUT):
            _sheet_step(c, step)
            X.append(c.state()["V"].copy())
        c.save_status(tmp_path / "status")
        assert "shellplastic" not in open(tmp_path / "status").read().split()  # the file of a run with nothing plastic is what it always was
        runs.append(X)
        c.close()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert abs(runs[0][SH_OUT - 1][:, 0].max() - 1.3 * SP * (NX - 1)) <= 1e-12


def test_sheet_stretched_and_returned(gpu_lib, tmp_path):
    steps, K = 2 * SH_OUT, 13
    c, V, tri = _sheet(gpu_lib, (YIELD, 0.004, INF, 0.0))
    c.precompute()
    g0 = c.shell_plastic_get()
    mass0 = c.features()["mass"].copy()
    assert np.array_equal(g0["B"], g0["B0"])
    alpha, alphaB = np.zeros(len(tri)), np.zeros(len(g0["alphaB"]))
    saved, peak = None, 0.0
    for step in range(steps):
        _sheet_step(c, step)
        X = c.state()["V"]
        g = c.shell_plastic_get()
        assert np.all(g["alpha"] >= alpha) and np.all(g["alphaB"] >= alphaB)  # the accumulated plastic strains never decrease
        never = g["alpha"] == 0.0
        assert np.array_equal(g["B"][never], g0["B"][never])  # a triangle that never yielded has its rest shape to the bit
        assert np.array_equal(g["triConst"][:, 4:], g0["triConst"][:, 4:]) and np.array_equal(c.features()["mass"], mass0)  # h A mu, h A lambda_ps, masses: untouched
        pt, ph, tot = c.shell_plastic_state()
        # r = 1: every triangle ends the step on or inside the yield surface.  n is recomputed from B', whose entries carry M U |B|_max (tolB); through F = E B' (two
        # products per entry, |E| <= the longest edge, sqrt(2) 1.3 SP) and e = ln(l) / 2 (smallest stretch >= 1/2 here, so an error of F doubles at most) that
        # is 4 M U |E|_max |B|_max, beside the M U (n + max |e|) <= M U of the norm itself
        Bmax = float(np.abs(g["B"]).max())
        assert np.all(np.isfinite(pt)) and np.all(pt[:, 0] <= pt[:, 1] + spm.M * spm.U * (1.0 + 4.0 * 1.3 * np.sqrt(2.0) * SP * Bmax)), (step, pt)
        assert np.all(pt[:, 1] == YIELD) and np.array_equal(pt[:, 2], g["alpha"]) and tot[1] == 0 and tot[4] == g["alpha"].max() and tot[5] == g["alphaB"].max()
        alpha, alphaB = g["alpha"].copy(), g["alphaB"].copy()
        peak = max(peak, float(pt[:, 3].max()))
        if step == K - 1:
            c.save_status(tmp_path / "status")
            txt = open(tmp_path / "status").read().split()
            i = txt.index("shellplastic")
            nH = len(g["alphaB"])
            assert txt[i + 1:i + 5] == [str(len(tri)), "5", str(nH), "2"] and len(txt) == i + 5 + 5 * len(tri) + 2 * nH and txt.index("dx_Elastic") < i
        if step == K:
            saved = (X.copy(), g["B"].copy(), g["alpha"].copy(), g["thetaBar"].copy(), g["alphaB"].copy())
    print(f"sheet: alpha max {alpha.max():.4f}, {int((alpha > 0).sum())} of {len(tri)} triangles yielded, rest-area ratio at most {peak:.4f}, {pt[:, 3].max():.4f} at the end")
    # at full stretch the plastic strain along the pull is about ln 1.3 - 0.03 = 0.23 and, with free edges, about half of it is lost across: the rest area
    # has grown by about exp(0.12); the way back compresses the longer sheet past its yield strain again and takes most of that out
    assert (alpha > 0).sum() >= len(tri) // 2 and peak > 1.05
    c.close()
    # (d) a fresh context continues from the file: step K + 1 to the bit
    c2, _, _ = _sheet(gpu_lib, (YIELD, 0.004, INF, 0.0))
    c2.load_status(tmp_path / "status")
    c2.precompute()
    _sheet_step(c2, SH_OUT)  # (K > SH_OUT: the grips are on their way back)
    g2 = c2.shell_plastic_get()
    assert np.array_equal(c2.state()["V"], saved[0])
    assert all(np.array_equal(g2[k], s) for k, s in zip(("B", "alpha", "thetaBar", "alphaB"), saved[1:]))
    assert np.array_equal(g2["B0"], g0["B0"])  # the rest shape a reset restores is the shell's, not the file's
    # a truncated section is refused, with a message that names it
    lines = open(tmp_path / "status").read().splitlines()
    open(tmp_path / "cut", "w").write("\n".join(lines[:-3]) + "\n")
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*shellplastic"):
        c2.load_status(tmp_path / "cut")
    c2.close()


def test_refusals_leave_the_state_as_it_was(gpu_lib):
    V, tri = sheet_mesh()
    E = gpu_lib.IpcGpuError
    nTri = len(tri)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=SH_E, PR=0.4, density=RHO)
    with pytest.raises(E, match="ipcgpu error -3"):  # no shell
        c.shell_set_plasticity((0, 1), YIELD)
    c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -4"):  # a sharded context
        c.shell_set_plasticity((0, 1), YIELD)
    c.close()
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=SH_E, PR=0.4, density=RHO)
    c.set_shell(tri, SH_H, SH_E, PR, RHO)
    c.shell_set_plasticity((0, 4), YIELD, 0.004, 5.0, 0.5)
    with pytest.raises(E, match="ipcgpu error -4"):  # ... and the other way round
        c.set_shard(0, 2)
    for bad in ((-1, 4, 0.1, 0.1, 1.0, 0.0), (0, nTri + 1, 0.1, 0.1, 1.0, 0.0), (3, 2, 0.1, 0.1, 1.0, 0.0), (0, 4, -0.1, 0.1, 1.0, 0.0), (0, 4, 0.1, -0.1, 1.0, 0.0),
                (0, 4, 0.1, 0.1, 0.0, 0.0), (0, 4, 0.1, 0.1, 1.0, -1.0), (0, 4, 0.1, 0.1, 1.0, INF), (0, 4, np.nan, 0.1, 1.0, 0.0), (0, 4, 0.1, np.nan, 1.0, 0.0)):
        with pytest.raises(E, match="ipcgpu error -1"):
            c.shell_set_plasticity(bad[:2], *bad[2:])
    # rubber both ways round
    model = np.zeros(nTri, dtype=np.int32)
    model[2] = 1
    with pytest.raises(E, match="ipcgpu error -4"):  # triangle 2 is plastic
        c.set_shell_membrane(model)
    model[:] = 0
    model[nTri - 1] = 1
    c.set_shell_membrane(model)  # the last triangle is not
    with pytest.raises(E, match="ipcgpu error -4"):
        c.shell_set_plasticity((nTri - 2, nTri), YIELD)
    c.shell_set_plasticity((nTri - 2, nTri), INF, INF)  # switching plasticity OFF on a rubber triangle is no conflict
    g = c.shell_plastic_get()
    assert np.array_equal(g["yield"] < INF, np.arange(nTri) < 4) and np.array_equal(g["bendYield"] < INF, np.arange(nTri) < 4)  # the refused calls changed nothing
    assert np.all(g["yield"][:4] == YIELD) and np.all(g["creep"][:4] == 5.0) and np.all(g["harden"][:4] == 0.5)
    with pytest.raises(E, match="ipcgpu error -1"):
        c.shell_plastic_update(0.0)
    with pytest.raises(E, match="ipcgpu error -1"):
        c.shell_plastic_set_state(alpha=-np.ones(nTri))
    c.set_shell(tri, SH_H, SH_E, PR, RHO)  # a new shell drops parameters and history
    assert np.all(c.shell_plastic_get()["yield"] == INF)
    c.close()


def test_the_membrane_call_keeps_a_flowed_rest_shape(gpu_lib):
    V, tri = sheet_mesh()
    nTri = len(tri)
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=SH_E, PR=0.4, density=RHO)
    c.set_shell(tri, SH_H, SH_E, PR, RHO)
    c.opt_init(SH_DT, False)
    c.shell_set_plasticity((0, nTri - 2), YIELD)
    c.set_positions(V * [1.2, 1.0, 0.95])
    counts = c.shell_plastic_update(SH_DT)
    assert counts == (nTri - 2, 0, 0, 0)
    g1 = c.shell_plastic_get()
    assert not np.any(np.all(g1["B"][:nTri - 2] == g1["B0"][:nTri - 2], axis=1))
    model = np.zeros(nTri, dtype=np.int32)
    model[nTri - 1] = 1
    c.set_shell_membrane(model, 0.1)
    g2 = c.shell_plastic_get()
    assert np.array_equal(g2["B"], g1["B"])  # rows 0-3: the flowed B of every triangle, to the bit
    assert np.array_equal(g2["triConst"][:nTri - 1, 4:], g1["triConst"][:nTri - 1, 4:]) and np.all(g2["triConst"][nTri - 1, 4:] == 0.0)  # rows 4-5: the rubber rule
    c.set_shell_membrane(None)  # ... and back: the plan's own constants, the flowed B still
    g3 = c.shell_plastic_get()
    assert np.array_equal(g3["B"], g1["B"]) and np.array_equal(g3["triConst"][:, 4:], g1["triConst"][:, 4:])
    c.close()
