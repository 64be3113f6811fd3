"""What the stepper reads back through its scalar board (csrc/scalar_slots.h) and the contact handler's read-back record, against the building-block
entry points evaluated at the same state: after every Newton iteration of two time steps, on the three paths that read back differently -- the
contact-free fast path, the same bar over a half-space (general path), two mats with self-collision and friction."""
import numpy as np
import pytest

from ipc_amd import scene

pytestmark = pytest.mark.gpu

DT, DT_MATS, GRAVITY, MU = 0.025, 0.01, -9.80665, 0.3
EPS = float(np.finfo(np.float64).eps)
TWIST = 0.4 * np.pi  # rad / s at either end of the fast-path bar
# Relative deviation of state()['E'] from the reference, per path; the bound is ten times the largest seen at the parent commit, at least 4 ulp.
#   fast           E read as S_E_TRIAL through k_publish2 against ipcgpu_incremental_potential (S_E_ITERATE through the plain publish): same kernels,
#                  same reduction order; measured 0.0 -> 4 ulp
#   half_space     against the sum of separate entry points (below): measured 3.33e-16
#   mats_friction  the same sum with the contact and friction terms: measured 2.23e-15
E_RTOL = {"fast": 4 * EPS, "half_space": max(4 * EPS, 10 * 3.33e-16), "mats_friction": max(4 * EPS, 10 * 2.23e-15)}


def _bar_mesh():
    return scene.make_bar(2, 2, 2, size=(1.0, 1.0, 1.0))


def _bar(gpu_lib, half_space):
    V, F = _bar_mesh()
    left, right = scene.border_verts(V, 0.01)
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(DT, half_space)  # gravity only where there is a floor to fall on
    planes = []
    if half_space:
        c.set_surface(scene.surface_tris(F))
        planes.append(c.add_half_space([0.0, float(V[:, 1].min()) - 2e-3, 0.0], [0.0, 1.0, 0.0]))
    else:
        c.set_twist(left, right, TWIST)
    c.precompute()
    return c, planes


def _mats_mesh():
    V, F, nA = scene.make_mat_stack(2, 2, gap=1.2e-3)
    return V, F


def _mats(gpu_lib):
    V, F = _mats_mesh()
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_positions(scene.jitter(V, F, rel=2e-3))
    c.opt_init(DT_MATS, True)
    c.set_surface(scene.surface_tris(F))
    c.enable_self_collision(1e-3)
    c.set_friction(MU, 1, 1e-3)
    c.set_ccd_mode(0)  # the stepper's full CCD is then the sweep ipcgpu_ccd_full runs
    c.precompute()
    return c, []


def _probe(gpu_lib, path):
    """a second context on the same mesh that never steps: the step bounds are asked of it at the positions an iteration started from"""
    V, F = _mats_mesh() if path == "mats_friction" else _bar_mesh()
    q = gpu_lib.Context(0)
    q.set_mesh(V, F, YM=2e4 if path == "mats_friction" else 1e5, PR=0.4, density=1000.0)
    q.opt_init(DT_MATS if path == "mats_friction" else DT, False)
    if path == "mats_friction":
        q.set_surface(scene.surface_tris(F))
    return q, np.unique(scene.surface_tris(F))


def _sum_of_entry_points(c, dt, planes, kappa, x_tilde, mass, v_start, seen):
    """E of the general paths from separate entry points, none of which is computeEnergyVal(): the elastic term (ipcgpu_elastic_energy, read through
    S_SCRATCH), the inertia term on the host from the positions, the barrier of the sets held (ipcgpu_contact_energy, read through ContactReadback::energy,
    and ipcgpu_halfspace_energy) at the kappa the line search used, and the lagged friction (ipcgpu_friction_energy)"""
    s = c.state()
    E = c.elastic_energy(dt * dt) + 0.5 * float(np.sum(mass[:, None] * (np.asarray(s["V"]) - x_tilde) ** 2))
    for h in planes:
        Eh = c.halfspace_energy(h, s["dHat"], kappa)
        seen["half_space"] += Eh > 0.0
        E += Eh
    if not planes:
        st = c.contact_state()
        if st["nActive"] + st["nPara"]:
            E += c.contact_energy(s["dHat"], kappa)
            seen["contact"] += 1
        fr = c.friction_state()
        if fr["fricDHat"] > 0.0 and fr["n_lagged"]:
            E += c.friction_energy(v_start, fr["fricDHat"], MU)
            seen["friction"] += 1
    return E


def _run(gpu_lib, path, rtol):
    c, planes = _mats(gpu_lib) if path == "mats_friction" else _bar(gpu_lib, path == "half_space")
    q, surface = _probe(gpu_lib, path)
    dt = DT_MATS if path == "mats_friction" else DT
    mass = c.features()["mass"]
    worst, bit, seen = 0.0, 0, dict(half_space=0, contact=0, friction=0)
    for step in range(2):
        # x~ = x^n + dt v^n + dt^2 g (backward Euler; no Dirichlet node on the two paths that use it)
        v_start = np.array(c.state()["V"])
        x_tilde = v_start + dt * c.kinematics()["velocity"].reshape(-1, 3) + dt * dt * np.array([0.0, GRAVITY, 0.0])
        c.begin_timestep()
        for it in range(60):
            before = c.state()
            p_inf = float(np.abs(before["searchDir"]).max())
            done = c.newton_iter()
            # the convergence decision is |p|_inf of the last direction (read through S_DIR_NORM) against targetGRes; never in the first pass
            assert done == (it > 0 and p_inf < before["targetGRes"]), (path, step, it, p_inf, before["targetGRes"])
            if done:
                break
            s = c.state()
            assert 0.0 < s["stepSize"] <= s["alphaFeasible"] <= 1.0, (path, step, it, s["stepSize"], s["alphaFeasible"])
            # the feasible step (S_TRIAL_ALPHA / S_STEP_FILTER on the fast path, filterStepSize and the step bounds elsewhere) against the bounds the entry
            # points give for this direction at the positions the iteration started from
            p = np.array(s["searchDir"])
            q.set_positions(np.array(before["V"]))
            bound = q.filter_step_size(p, 1.0)
            if path == "mats_friction":
                # Optimizer.cpp:1884-2040: outside the CFL ball the full CCD decides, but never below alpha_CFL = sqrt(dHat) / (2 max |p_v|) over the surface
                # nodes; that term is recomputed here in numpy, hence 4 ulp on it
                bound = min(bound, q.ccd_full(p, 0.8, 1.0)[0])
                p_max = float(np.sqrt((p.reshape(-1, 3)[surface] ** 2).sum(axis=1)).max())
                bound = max(bound, np.sqrt(s["dHat"]) / (2.0 * p_max) * (1.0 + 4 * EPS))
            bit += bound < 1.0
            print(f"{path} step {step} iteration {it}: alphaFeasible {s['alphaFeasible']!r} bound {bound!r}")
            assert s["alphaFeasible"] <= bound, (path, step, it, s["alphaFeasible"], bound)
            E = c.incremental_potential(dt * dt) if path == "fast" else _sum_of_entry_points(c, dt, planes, before["kappa"], x_tilde, mass, v_start, seen)
            dev = abs(s["E"] - E) / abs(E)
            worst = max(worst, dev)
            print(f"{path} step {step} iteration {it}: E {s['E']!r} reference {E!r} relative deviation {dev:.3e}")
            assert dev <= rtol, (path, step, it, s["E"], E)
        else:
            raise AssertionError(f"{path}: no convergence in 60 iterations")
        c.end_timestep()
    print(f"{path}: largest relative deviation of E {worst:.3e}; the step bound was below 1 in {bit} iterations; terms compared {seen}")
    # the comparison must have had the terms it is about: a barrier on the plane, an active set and a lagged friction set between the mats
    if path == "half_space":
        assert seen["half_space"] > 0, seen
    if path == "mats_friction":
        assert seen["contact"] > 0 and seen["friction"] > 0, seen
    c.close()
    q.close()
    return worst


@pytest.mark.parametrize("path", ["fast", "half_space", "mats_friction"])
def test_stepper_readbacks_match_entry_points(gpu_lib, path):
    _run(gpu_lib, path, E_RTOL[path])


def test_hessian_error_survives_other_readbacks(gpu_lib):
    """a pattern without the contact connectivity: the "outside the CSR pattern" error of the barrier Hessian arrives, also after a CCD and a barrier energy
    have used the read-back record in between.  This is the IMMEDIATE route (ipcgpu_contact_hessian_add downloads the counter block): it never touches
    ContactReadback::hessError and would pass with that member anywhere.  The deferred route is reached only inside ipcgpu_assemble_newton and the stepper,
    which take the flag before they return and whose pattern always covers the sets, so no public entry point can make it carry a non-zero flag across
    another read-back: that member's separation is checked by the struct's static_asserts and by reading, not by this test."""
    V, F, nA = scene.make_mat_stack(4, 2, gap=1.2e-3)
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_positions(scene.jitter(V, F, rel=2e-3))
    c.opt_init(0.01, True)
    c.set_surface(scene.surface_tris(F))
    dHat = 1e-6 * float(np.sum((V.max(0) - V.min(0)) ** 2))
    assert len(c.contact_build(dHat)["active"]) > 0
    c.set_pattern()  # the mesh's own connectivity only
    p = 1e-3 * np.random.default_rng(3).normal(size=3 * len(V))
    for between in (False, True):
        if between:
            c.ccd_full(p, 0.8, 1.0)
            assert c.contact_energy(dHat, 1e3) > 0.0
        c.set_zero()
        with pytest.raises(Exception, match="outside the CSR pattern"):
            c.contact_hessian_add(dHat, 1e3, True)
    c.close()
