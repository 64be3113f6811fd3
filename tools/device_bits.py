"""Bits of the deterministic device paths: one SHA-256 per case over the raw bytes of what the case returns, and one digest over the digests.
    python tools/device_bits.py            (on the GPU; run it at two commits and compare the lines)
Every case runs twice on fresh contexts.  A case whose two runs differ (or that raises) is reported and left out of the final digest: only paths without
fp64 atomics are listed, so that should not happen.  Sizes: a 14 x 14 x 2 mat stack and a 6 x 6 x 6 bar (item counts between 257 and a few thousand, no
multiples of 64), and one bar of 65 856 tets for elastic_energy alone, whose reduction strides over more than 256 partial sums.  The step3_* cases run three
time steps of the stepper and hash positions, energy, step sizes, iteration counts and the contact state after each.  The analytic obstacles: the
half-space on the mat stack and its lagged friction inside the potential, gradient and matrix of a begun time step; a solid sphere, a hollow sphere and
a capsule on the bar and on a finer bar whose sets span several workgroups (every entry point, the friction pieces and the state query); and a stepper
case with a plane and a capsule, both with friction, the capsule registered first."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ipc_amd  # noqa: E402
from ipc_amd import scene  # noqa: E402

DT, DTSQ, KAPPA = 0.01, 1e-4, 1e3


def raw(*xs):
    h = hashlib.sha256()
    for x in xs:
        if isinstance(x, dict):
            x = [x[k] for k in sorted(x)]
        if isinstance(x, (list, tuple)):
            h.update(raw(*x).encode())
        else:
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def bar_ctx(nx=6, ny=6, nz=6, solver=None, before_init=None):
    V, F = scene.make_bar(nx, ny, nz, size=(3.0, 1.0, 1.0))
    Vt = scene.twist_state(scene.jitter(V, F), 0.25)
    left, right = scene.border_verts(V, 0.01)
    c = ipc_amd.Context(0) if solver is None else ipc_amd.Context(0, solver=solver)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    if before_init:
        before_init(c, F)
    c.opt_init(0.025, False)
    c.set_dbc(np.concatenate([left, right]), 2)
    c.set_positions(Vt)
    return c, V, F, Vt


def direction(n, seed=5):
    return 1e-2 * np.random.default_rng(seed).normal(size=(n, 3))


def mat_ctx():
    V, F, nA = scene.make_mat_stack(14, 2, gap=1.2e-3)
    Vs = scene.jitter(V, F, rel=2e-3)
    border = np.nonzero((np.abs(V[:nA, 0]) > 0.49) | (np.abs(V[:nA, 2]) > 0.49))[0].astype(np.int32)
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_dbc(border, 1)
    c.set_positions(Vs)
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    dHat = 1e-6 * float(np.sum((V.max(0) - V.min(0)) ** 2))
    c.contact_build(dHat)
    c.set_pattern(c.contact_connectivity())
    return c, V, F, Vs, dHat


# ---- nh_kernels ---------------------------------------------------------------------------------------------------------------------------------------------
def case_elastic():
    c, V, F, Vt = bar_ctx()
    out = [c.elastic_energy(DTSQ), c.incremental_potential(DTSQ), int(c.check_inversion()), c.filter_step_size(direction(len(V)).reshape(-1), 1.0),
           c.filter_step_size(40.0 * direction(len(V), 6).reshape(-1), 1.0)]
    c.close()
    return out


def case_elastic_energy_large():
    c, V, F, Vt = bar_ctx(28, 28, 14)
    assert len(F) >= 65537, len(F)
    out = [c.elastic_energy(DTSQ)]
    c.close()
    return out


# ---- hip_contact --------------------------------------------------------------------------------------------------------------------------------------------
def case_contact():
    c, V, F, Vs, dHat = mat_ctx()
    out = [c.contact_energy(dHat, KAPPA), c.contact_gradient_add(dHat, KAPPA, True)]
    c.set_zero()
    c.contact_hessian_add(dHat, KAPPA, True)
    out.append(c.get_a())
    c.close()
    return out


def case_friction_and_report():
    c, V, F, Vs, dHat = mat_ctx()
    c.friction_update(dHat, KAPPA)
    Vprev = Vs + direction(len(V), 7) * 0.05
    eps2 = 1e-8
    out = [c.friction_energy(Vprev, eps2, 0.3), c.friction_gradient_add(Vprev, eps2, 0.3)]
    c.set_zero()
    c.friction_hessian_add(Vprev, eps2, 0.3, True)
    out.append(c.get_a())
    rep = c.contact_report(dHat, KAPPA, Vprev, eps2, 0.3)
    out.append(rep.tobytes())
    c.close()
    return out


def case_ccd_full():
    c, V, F, Vs, dHat = mat_ctx()
    p = direction(len(V), 8).reshape(-1)
    out = list(c.ccd_full(p, 0.8, 1.0))  # the bound, the limiting pair, the number of candidates
    c.close()
    return out


# ---- vertex_collider: the half-space ------------------------------------------------------------------------------------------------------------------------
def case_halfspace():
    c, V, F, Vs, dHat = mat_ctx()
    y0 = float(Vs[:, 1].min())
    h = c.add_half_space([0.0, y0 - 5e-4, 0.0], [0.0, 1.0, 0.0])
    dh = 1e-5
    verts = c.halfspace_build(h, dh)
    assert len(verts) > 64, len(verts)
    out = [verts, c.halfspace_energy(h, dh, KAPPA)]
    c.set_zero()
    c.halfspace_hessian_add(h, dh, KAPPA, True)
    out.append(c.get_a())
    out.append(c.halfspace_step_bound(h, direction(len(V), 9), 0.9, 1.0))
    out.append(c.half_space_move(h, [0.0, 2e-3, 0.0], 0.5))
    c.close()
    return out


def case_halfspace_friction():
    # the plane's lagged friction terms at entry-point level.  No entry point takes a half-space's friction alone, so: begin_timestep lags the plane at x^n
    # (self-contact is off, the plane is the only obstacle), the nodes are then displaced along and off the plane, and the incremental potential, the
    # Newton gradient and the matrix are taken with the plane's friction and again without it; both enter the digest and have to differ
    V, F = scene.make_bar(6, 6, 6, size=(3.0, 1.0, 1.0))
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    h = c.add_half_space([0.0, float(V[:, 1].min()) - 2e-3, 0.0], [1e-3, 1.0, -5e-4])  # (tilted a little: no component of the normal is zero)
    c.set_half_space_friction(h, 0.3)
    c.precompute()
    c.begin_timestep()
    fs = c.friction_state()
    assert fs["n_half_space_lagged"] > 16 and fs["n_lagged"] == 0 and fs["fricDHat"] > 0.0, fs
    d = 100.0 * direction(len(V), 7) * np.sqrt(fs["fricDHat"])  # displacements of the order of eps_v h: sticking and sliding entries
    d[:, 1] = np.abs(d[:, 1])
    c.set_positions(c.state()["V"] + d)
    out = [fs]
    for mu in (0.3, 0.0):
        c.set_half_space_friction(h, mu)
        out += [c.incremental_potential(DT * DT), c.assemble_newton(DT * DT, True), c.get_a()]
    assert out[1] != out[4] and not np.array_equal(out[2], out[5]) and not np.array_equal(out[3], out[6]), "the plane's friction terms did not act"
    c.close()
    return out


# ---- round colliders: a solid sphere under the 6 x 6 x 6 bar, a hollow sphere around it, a capsule along its bottom face -----------------------------------
ROUNDS = [dict(p0=[0.1, -1.6, 0.05], p1=[0.1, -1.6, 0.05], R=1.0, hollow=False, dHat=0.25, delta=[0.0, 0.2, 0.0]),
          dict(p0=[0.05, 0.02, -0.03], p1=[0.05, 0.02, -0.03], R=1.8, hollow=True, dHat=1.0, delta=[0.3, 0.0, 0.0]),
          dict(p0=[-1.0, -0.8, 0.02], p1=[1.1, -0.78, -0.04], R=0.25, hollow=False, dHat=0.16, delta=[0.0, 0.1, 0.0])]


def round_ctx(n=(6, 6, 6)):
    V, F = scene.make_bar(*n, size=(3.0, 1.0, 1.0))
    Vs = scene.jitter(V, F, rel=2e-3)
    left, _ = scene.border_verts(V, 0.01)
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.set_dbc(left, 1)
    c.set_positions(Vs)
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    c.set_pattern()
    ids = [c.add_round_collider(r["p0"], r["p1"], r["R"], r["hollow"]) for r in ROUNDS]
    return c, V, Vs, ids


def case_round_barrier(n=(6, 6, 6), at_least=(16, 16, 16)):
    c, V, Vs, ids = round_ctx(n)
    out = []
    for k, (i, r) in enumerate(zip(ids, ROUNDS)):
        verts = c.round_build(i, r["dHat"])
        assert len(verts) > at_least[k] and len(verts) % 64, (k, len(verts))
        out += [verts, c.round_energy(i, r["dHat"], KAPPA), c.round_gradient_add(i, r["dHat"], KAPPA)]
        c.set_zero()
        c.round_hessian_add(i, r["dHat"], KAPPA, True)
        out += [c.get_a(), c.round_step_bound(i, 10.0 * direction(len(V), 9 + k), 0.9, 1.0)]
    for i, r in zip(ids, ROUNDS):  # (the moves last: the three share one set of positions)
        out += [c.round_move(i, r["delta"], 0.5), c.round_get(i)]
    c.close()
    return out


def case_round_friction(n=(6, 6, 6), which=2, at_least=16):
    c, V, Vs, ids = round_ctx(n)
    i, r = ids[which], ROUNDS[which]
    c.set_round_collider_friction(i, 0.4)
    out = [c.round_build(i, r["dHat"]), c.round_lag_update(i, r["dHat"], KAPPA)]
    assert out[1] > at_least and out[1] % 64, out[1]
    Vprev = Vs + direction(len(V), 7) * 0.05
    eps2 = 1e-8
    out += [c.round_friction_energy(i, Vprev, eps2), c.round_friction_gradient_add(i, Vprev, eps2)]
    c.set_zero()
    c.round_friction_hessian_add(i, Vprev, eps2, True)
    out += [c.get_a(), c.round_state(i, r["dHat"], KAPPA)]
    c.close()
    return out


# ---- pcg ----------------------------------------------------------------------------------------------------------------------------------------------------
def case_pcg(precond):
    def run():
        c, V, F, Vt = bar_ctx(solver=2)
        c.set_pattern()
        c.assemble_newton(0.025 ** 2, True, with_gradient=False)
        n = 3 * len(V)
        c.set_iterative(1e-10, n, precond, 8)
        c.analyze_pattern()
        assert c.factorize()
        x = c.solve(np.random.default_rng(14).normal(size=n))
        out = [x, c.iter_stats()["iterations"]]
        c.close()
        return out
    return run


# ---- chamber_kernels, shell_limit_kernels -------------------------------------------------------------------------------------------------------------------
def case_chamber():
    c, V, F, Vt = bar_ctx(before_init=lambda c, F: c.set_chambers([scene.surface_tris(F)], [30.0]))
    out = [c.chamber_energy(1.0)]
    c.chamber_set_gas([True], ambient=1e3, gamma=1.4)
    out += [c.chamber_gas_state(), c.chamber_energy(1.0)]
    c.close()
    return out


def case_shell_stretch():
    n = 21  # a flat sheet of 441 nodes and 800 triangles without tetrahedra, pulled to 1.3 x 1.1 of its rest size
    X, Z = np.meshgrid(np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, n), indexing="ij")
    V = np.column_stack([X.ravel(), np.zeros(n * n), Z.ravel()])
    idx = np.arange(n * n).reshape(n, n)
    q = [idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()]
    tri = np.concatenate([np.column_stack([q[0], q[1], q[2]]), np.column_stack([q[0], q[2], q[3]])]).astype(np.int32)
    c = ipc_amd.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=1e5, PR=0.3, density=1000.0)
    c.set_shell(tri, 1e-3, 1e5, 0.3, 1000.0)
    c.set_shell_strain_limit(1.5)
    c.opt_init(0.01, True)
    c.set_positions(V * np.array([1.3, 1.0, 1.1]) + 1e-3 * np.random.default_rng(11).normal(size=V.shape))
    out = [c.shell_stretch()]
    c.close()
    return out


# ---- twelve Newton steps with friction and a half-space -----------------------------------------------------------------------------------------------------
def case_newton_steps():
    V, F, nA = scene.make_mat_stack(14, 2, gap=1.2e-3)
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_positions(scene.jitter(V, F, rel=2e-3))
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    c.enable_self_collision(1e-3)
    c.set_friction(0.3, 1, 1e-3)
    h = c.add_half_space([0.0, float(V[:, 1].min()) - 2e-3, 0.0], [0.0, 1.0, 0.0])
    c.set_half_space_friction(h, 0.3)
    c.precompute()
    out = []
    c.begin_timestep()
    for _ in range(12):
        done = c.newton_iter()
        out.append(c.state()["V"].copy())
        if done:
            c.end_timestep()
            c.begin_timestep()
    c.close()
    return out


# ---- three time steps through the stepper: every read-back of the scalar board and of the contact handler --------------------------------------------------
def stepped(c, steps=3, max_iter=100, extra=None, contact=False):
    out = []
    for _ in range(steps):
        n = c.solve_timestep(max_iter)
        s = c.state()
        out += [s["V"].copy(), s["E"], s["stepSize"], s["alphaFeasible"], n, s["innerIterAmt"]]
        if contact:  # (the entry point refuses a context without self-collision and half-spaces)
            out.append(c.contact_state())
        if extra:
            out.append(extra(c))
    c.close()
    return out


def step_bar(energy="NH", twist=True, setup=None):
    V, F = scene.make_bar(6, 6, 6, size=(3.0, 1.0, 1.0))
    left, right = scene.border_verts(V, 0.01)
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.set_energy_type(energy)
    c.opt_init(0.025, False)
    if twist:
        c.set_twist(left, right)
    if setup:
        setup(c, V, left, right)
    c.precompute()
    return c


def case_step_bar(energy):
    return lambda: stepped(step_bar(energy))  # the fast path: k_iter_reset, k_publish2, alpha and both energies (FCR: no inversion guard, the filter slot unused)


def case_step_damping_neumann():
    def setup(c, V, left, right):
        c.set_damping(0.1)
        c.add_neumann(np.nonzero(np.abs(V[:, 0] - V[:, 0].mean()) < 0.3)[0].astype(np.int32), [0.0, -20.0, 0.0])
    return stepped(step_bar(setup=setup))


def case_step_mdbc():
    # the right end moves 0.6 (more than a cell) per step against the held left end: the inversion guard cuts the scripted step short, the rest goes the penalty route
    seen = []

    def setup(c, V, left, right):
        c.add_dirichlet(left)
        c.add_dirichlet(right, lin_vel=(-24.0, 0.0, 0.0))

    def extra(c):
        d = c.dbc_state()
        seen.append(d["rho"] > 0.0 or not d["projectDBC"])
        return d
    out = stepped(step_bar(twist=False, setup=setup), max_iter=40, extra=extra)
    assert any(seen), "the penalty route was not taken"
    return out


def case_step_mats(ccd_mode):
    def run():
        V, F, nA = scene.make_mat_stack(14, 2, gap=1.2e-3)
        c = ipc_amd.Context(0)
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.set_positions(scene.jitter(V, F, rel=2e-3))
        c.opt_init(DT, True)
        c.set_surface(scene.surface_tris(F))
        c.enable_self_collision(1e-3)
        c.set_friction(0.3, 1, 1e-3)
        c.set_ccd_mode(ccd_mode)  # 0: the swept-box sweep, 1: the reference's sweep
        c.precompute()
        full = []
        out = stepped(c, contact=True, extra=lambda c: full.append(c.contact_state()["nFullCCD"]) or full[-1])
        assert full[-1] > 0, "the stepper never ran its full CCD: the sweep's read-backs are not covered"
        return out
    return run


def case_step_plane_capsule():
    # the 6 x 6 x 6 bar sliding along +x under gravity on a plane and a capsule that lies in it, both with friction; the capsule is registered BEFORE the
    # plane (the stepper walks the planes first whatever the order of registration)
    V, F = scene.make_bar(6, 6, 6, size=(3.0, 1.0, 1.0))
    c = ipc_amd.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    y0 = float(V[:, 1].min()) - 2e-3
    r = c.add_round_collider([-1.0, y0 - 0.2, 0.0], [1.0, y0 - 0.2, 0.0], 0.2)
    h = c.add_half_space([0.0, y0, 0.0], [0.0, 1.0, 0.0])
    c.set_round_collider_friction(r, 0.4)
    c.set_half_space_friction(h, 0.3)
    c.set_velocity(np.tile([0.5, 0.0, 0.0], (len(V), 1)))
    c.precompute()
    seen = []

    def extra(c):
        s = c.round_state(r)
        seen.append((s["n"], c.friction_state()["n_half_space_lagged"]))
        return [s, c.round_get(r)]
    out = stepped(c, contact=True, extra=extra)
    assert all(a > 0 and b > 0 for a, b in seen), seen  # both obstacles act in every step
    return out


CASES = [("elastic_energy+incremental_potential+check_inversion+filter_step_size", case_elastic), ("elastic_energy_65k_tets", case_elastic_energy_large),
         ("contact_energy+gradient_add+hessian_add", case_contact), ("friction_energy+gradient+hessian+contact_report", case_friction_and_report),
         ("ccd_full", case_ccd_full), ("halfspace_energy+hessian_add+step_bound+move", case_halfspace), ("pcg_block_jacobi", case_pcg(0)),
         ("pcg_lagged_factor", case_pcg(1)), ("pcg_two_level", case_pcg(2)), ("chamber_energy+gas_state", case_chamber), ("shell_stretch", case_shell_stretch),
         ("newton_12_steps_friction_halfspace", case_newton_steps), ("step3_bar_NH_fast_path", case_step_bar("NH")), ("step3_bar_FCR", case_step_bar("FCR")),
         ("step3_bar_damping_neumann", case_step_damping_neumann), ("step3_bar_moving_dirichlet_penalty", case_step_mdbc),
         ("step3_mats_self_collision_friction", case_step_mats(0)), ("step3_mats_reference_ccd", case_step_mats(1)),
         ("round_build+energy+gradient+hessian+step_bound+move+get_x3", case_round_barrier),
         ("round_lag_update+friction_energy+gradient+hessian+state", case_round_friction),
         # (the same on a 24 x 10 x 10 bar, 1 162 surface vertices: sets of more than one workgroup, the friction pieces on the hollow sphere)
         ("round_barrier_x3_fine_bar", lambda: case_round_barrier((24, 10, 10), (64, 512, 256))),
         ("round_friction+state_fine_bar", lambda: case_round_friction((24, 10, 10), 1, 512)),
         ("halfspace_lagged_friction_in_potential+gradient+matrix", case_halfspace_friction),
         ("step3_bar_capsule_then_plane_friction", case_step_plane_capsule)]


def main():
    only = sys.argv[1:]
    kept, ran = [], 0
    for name, fn in CASES:
        if only and not any(o in name for o in only):
            continue
        ran += 1
        try:
            a, b = raw(*fn()), raw(*fn())
        except Exception as e:  # noqa: BLE001
            print(f"{name:78s} LEFT OUT: {type(e).__name__}: {e}", flush=True)
            continue
        if a != b:
            print(f"{name:78s} LEFT OUT: two runs differ ({a[:16]} / {b[:16]})", flush=True)
            continue
        kept.append(a)
        print(f"{name:78s} {a}", flush=True)
    print(f"{'digest of ' + str(len(kept)) + ' digests':78s} {hashlib.sha256(''.join(kept).encode()).hexdigest()}", flush=True)
    return 0 if len(kept) == ran else 1


if __name__ == "__main__":
    sys.exit(main())  # non-zero when a case was left out
