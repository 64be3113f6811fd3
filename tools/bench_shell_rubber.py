"""Rubber-membrane kernels on hardware (not part of bench.py): on the same n x n-node sheet, stretched 1.2 x 1.1 and perturbed, the StVK shell, the all-rubber
shell and a half-and-half shell (every second triangle rubber) -- HIP-event medians of the shell energy (ipcgpu_shell_energy: every shell term), of
ipcgpu_assemble_newton (gradient + Hessian; what the rubber costs is the difference between the three sheets, mesh and pattern being the same) and of the
rubber term alone; then the Newton iterations per step of the level-3 balloon at constant pressure (and the host wall time per iteration of that run).  Prints one JSON line
(committed as profiles/shell_rubber_bench.json).
  * events are recorded on the context's own stream (tools/_timing.py); the entry points add a few-byte read-back each, which the event pair includes;
  * the StVK kernels are untouched: on a rubber triangle they read zeros for their two constants and do all their work on them (the 6 x 6 Jacobi projection
    of a zero matrix included), so their cost does not depend on the rubber fraction; "stvk_kernels_on_all_rubber_ms" is ipcgpu_shell_hessian_add minus
    ipcgpu_shell_rubber_hessian_add on the all-rubber sheet, beside the StVK sheet's ipcgpu_shell_hessian_add.
usage: python tools/bench_shell_rubber.py [--n 200] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from _timing import timed  # noqa: E402
from bench_shell import grid  # noqa: E402
from ipc_amd import lib  # noqa: E402

H, YM, PR, RHO = 1e-3, 1e5, 0.3, 1000.0
NO_T = np.zeros((0, 4), dtype=np.int32)


def context(V, tri, model):
    c = lib.Context(0)
    c.set_mesh(V, NO_T, YM=YM, PR=0.4, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    if model is not None:
        c.set_shell_membrane(model, 0.1)
    c.opt_init(0.01, True)
    return c


def balloon(level):
    from chamber_gas_mp import icosphere
    V, tri = icosphere(level)
    E, h = 3e5, 0.01
    c = lib.Context(0)
    c.set_mesh(V, NO_T, YM=E, PR=0.4, density=RHO)
    c.set_shell(tri, h, E, PR, RHO, bend_scale=0.0)
    c.set_shell_membrane(1, 0.0)
    c.set_chambers([tri], [0.4 * 2 * (E / 3) * h])
    c.opt_init(1.0, False)
    c.set_time_integration("BE")
    c.set_surface(tri)
    c.set_damping(0.1)
    c.set_rel_tol(1e-8)
    c.precompute()
    its, t0 = [], time.time()
    for _ in range(6):
        its.append(c.solve_timestep(300))
    # host wall time over the six steps, first step's set-up and all host work included, no warm-up: not comparable with the HIP-event medians above
    return {"level": level, "triangles": int(len(tri)), "newton_iterations_per_step": its, "newton_iteration_wall_ms": 1e3 * (time.time() - t0) / max(sum(its), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = grid(args.n, 1.0 / (args.n - 1))
    rng = np.random.default_rng(0)
    x = V * [1.2, 1.0, 1.1] + 2e-4 * rng.standard_normal(V.shape)
    rec = {"tool": "bench_shell_rubber", "nodes": int(len(V)), "triangles": int(len(tri)), "reps": args.reps}
    half = (np.arange(len(tri)) % 2).astype(np.int32)
    for label, model in (("stvk", None), ("rubber", np.ones(len(tri), dtype=np.int32)), ("half", half)):
        c = context(V, tri, model)
        c.set_pattern()
        c.set_positions(x)
        r = {}
        r["shell_energy_ms"], _ = timed(c, lambda: c.shell_energy(1e-4), args.reps)
        r["assemble_newton_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
        r["shell_gradient_ms"], _ = timed(c, lambda: c.shell_gradient_add(1e-4, True), args.reps)
        r["shell_hessian_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
        if model is not None:
            r["rubber_energy_ms"], _ = timed(c, lambda: c.shell_rubber_energy(1e-4), args.reps)
            r["rubber_hessian_ms"], _ = timed(c, lambda: c.shell_rubber_hessian_add(1e-4, True), args.reps)
            r["stvk_kernels_ms_by_difference"] = r["shell_hessian_ms"] - r["rubber_hessian_ms"]
        rec[label] = r
        del c
    rec["stvk_kernels_on_all_rubber_ms"] = rec["rubber"]["stvk_kernels_ms_by_difference"]
    rec["assemble_newton_rubber_minus_stvk_ms"] = rec["rubber"]["assemble_newton_ms"] - rec["stvk"]["assemble_newton_ms"]
    rec["balloon"] = balloon(3)
    rec["believed_bound"] = {"rubber": "fp64 issue of the 6 x 6 Jacobi sweeps at one 64-lane workgroup per triangle block, then L2 atomics (45 adds per triangle), as the "
                                       "StVK membrane kernel; a belief to test, not a measurement"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
