"""Run one of the reference's scene scripts (src/Config.cpp grammar) on the GPU through the C ABI.
usage: python tools/run_scene.py <scene.txt> [--root DIR] [--steps N] [--status-every K] [--out DIR] [--precond {0,1,2}] [--report DIR] [--fields DIR [--fields-every K]] [--contact-report DIR]
`--root` is the directory the script's relative mesh paths are resolved against (the reference resolves them against its
repository root).  `--precond` chooses the preconditioner of a `linearSolver AMGCL` scene (0 block Jacobi, the default; 1 lagged Cholesky; 2 two-level).  `--report DIR` writes the reference's system report, `DIR/sysE.txt`, `sysM.txt` and `sysL.txt`: energy, linear and angular momentum per mesh component, one line
after precompute() and one per time step (17 significant digits).  `--fields DIR` writes `DIR/fields<N>.vtu` after every K-th time step (K = 1 unless
`--fields-every` says otherwise): an ASCII VTK unstructured grid with the Cauchy stress, von Mises stress and J per element (and the accumulated plastic strain `plasticStrain` when a shape carries `plastic`, the fibre stretch `fiberStretch` and direction `fiberDir` when one carries `fiber`), the nodal mean stress, its von
Mises stress and the velocity per node, and -- when the scene has contact -- the contact and friction forces per node (ipc_amd/scene_script.py FieldsWriter).
`--contact-report DIR` writes `DIR/contact.txt`: after every time step one line per pair of components (or component and half-space) in contact -- smallest
squared distance, constraint counts by kind, barrier forces and torques on either side, friction forces and work (ipc_amd/scene_script.py
ContactReportWriter); it is taken on the constraint sets the stepper holds and does not change the run.  Prints one line per time step; writes `status<N>` checkpoints in the reference's format."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipc_amd import lib, scene_script as ss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("scene")
ap.add_argument("--root", default=None)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--status-every", type=int, default=0)
ap.add_argument("--out", default=".")
ap.add_argument("--precond", type=int, choices=(0, 1, 2), default=None)
ap.add_argument("--report", default=None)
ap.add_argument("--fields", default=None)
ap.add_argument("--fields-every", type=int, default=1)
ap.add_argument("--contact-report", default=None)
args = ap.parse_args()

root = args.root or os.path.dirname(os.path.abspath(args.scene))
cfg = ss.SceneConfig.parse(open(args.scene).read(), root)
sc = ss.assemble(cfg, lib.read_tet_mesh)
print(f"{len(cfg.shapes)} shapes, {sc.V.shape[0]} nodes, {sc.T.shape[0]} tets, {sc.SF.shape[0]} surface triangles, dt = {cfg.dt}")
ctx = lib.Context(0, solver=cfg.linear_solver)  # `linearSolver AMGCL` -> the iterative solver
if args.precond is not None:
    if cfg.linear_solver != lib.SOLVER_PCG:
        sys.exit("--precond needs a scene with `linearSolver AMGCL`")
    ctx.set_iterative(precond=args.precond)
c = ss.apply(sc, ctx)  # (the `aero` shapes and the `wind` line included: set_aero, aero_set_wind)
if sc.aero is not None:
    print(f"{len(sc.aero['tri_lists'])} aerodynamic surfaces, {sum(len(t) for t in sc.aero['tri_lists'])} triangles, wind {cfg.wind}, air density {cfg.air_density}")
report = ss.ReportWriter(args.report) if args.report else None
if report:
    report.write(c)
has_contact = cfg.self_collision or sc.obstacle_nodes is not None
fields = ss.FieldsWriter(args.fields, sc, has_contact, cfg.effective_self_fric() if cfg.self_collision else 0.0) if args.fields else None
contact_report = None
if args.contact_report and (cfg.self_collision or cfg.half_spaces):
    contact_report = ss.ContactReportWriter(args.contact_report, cfg.effective_self_fric() if cfg.self_collision else 0.0)
elif args.contact_report:
    print("--contact-report: the scene has neither self-collision nor a half-space, nothing will be written")
steps = args.steps if args.steps is not None else int(round(cfg.duration / cfg.dt))
timestep = c.state()["timestep"] if fields else 0  # not 0 after `restart`
for step in range(steps):
    t0 = time.time()
    sc.move_round_colliders(c)  # `sphereCollider` / `capsuleCollider` with a `velocity`: v dt plus what the last move left over
    sc.before_step(c, step * cfg.dt)  # state-dependent script decisions (AnimScripter::stepAnimScript)
    ramped = sc.chamber_pressures((step + 1) * cfg.dt)  # `pressure <p> ramp <seconds>`: p min(1, t / ramp) at the time this step ends; None without a ramp
    if ramped is not None:
        c.chamber_set_pressure(ramped)
    for group, act in sc.fiber_activations((step + 1) * cfg.dt) or ():  # `fiber ... activate <act> ramp <seconds>`: act min(1, t / ramp) at the time this step ends
        c.fiber_set_activation(group, act)
    writes_fields = fields is not None and (timestep + 1) % max(args.fields_every, 1) == 0
    x_prev = c.get_positions() if writes_fields or contact_report else None  # the friction field / columns need the positions the step started from
    it = c.solve_timestep(1000)
    st = c.state()
    timestep = st["timestep"]
    cs = c.contact_state() if cfg.self_collision or cfg.half_spaces else {}
    print(f"step {st['timestep']:5d}  {it:4d} Newton iterations  {1e3 * (time.time() - t0):8.1f} ms  E = {st['E']:.6e}  active = {cs.get('nActive', 0)}", flush=True)
    for k in range(len(cfg.round_colliders)):
        rs = c.round_state(k)
        print(f"            round collider {k}: {rs['n']} active, min s = {rs['min_s']:.3e}, force on the bodies {rs['force'] / cfg.dt ** 2}", flush=True)
    if report:
        report.write(c)
    if contact_report:  # (before the fields writer, which rebuilds the constraint set)
        contact_report.write(c, st["timestep"], x_prev)
    if writes_fields:
        _, n_invalid = fields.write(c, st["timestep"], x_prev)
        if n_invalid:
            print(f"step {st['timestep']:5d}  {n_invalid} inverted element(s): their stress is NaN", flush=True)
    if args.status_every and st["timestep"] % args.status_every == 0:
        c.save_status(os.path.join(args.out, f"status{st['timestep']}"))
c.close()
