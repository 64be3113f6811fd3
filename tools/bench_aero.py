"""Air-drag kernels on hardware (not part of bench.py): HIP-event times of the energy, the gradient + Hessian and the state query on the icosphere of
tools/bench_chamber.py (default: 6 subdivisions, 81 920 triangles, 40 962 nodes, radius 0.1, slightly perturbed) as one two-sided aerodynamic surface in a
wind, and -- the yardstick, in the same run on the same mesh -- launch_chamber_assemble through the chamber entry points.  Prints one JSON line
(committed as profiles/aero_bench.json).
  * events are recorded on the context's own stream around the C entry points, which add up- and downloads of their arguments (tools/bench_chamber.py): the
    assemble kernels are timed through ipcgpu_aero_hessian_add / ipcgpu_chamber_hessian_add (no transfer beyond the 4-byte error flag) and through
    ipcgpu_assemble_newton with and without the term; the state query downloads 3 nTri forces, 8 nTri records and 5 totals, so it is timed with the totals
    alone as well;
  * the refresh kernel has no entry point of its own (it runs inside ipcgpu_opt_begin_timestep): it is not timed here;
  * medians of --reps;
  * byte bound: what one pass has to read at least -- 3 node ids and 1 surface id per triangle (16 B), the lagged record (64 B) and every node's position
    once (24 B) -- at the 6.3 TB/s a copy kernel reaches on this part; the Hessian adds 45 fp64 atomic adds per triangle (3 diagonal blocks of 6, 3
    off-diagonal blocks of 9) beside the 9 of the gradient, exactly as a chamber triangle.
usage: python tools/bench_aero.py [--subdiv 6] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from bench_chamber import ACHIEVABLE_BW, H, PR, RADIUS, RHO, YM, icosphere  # noqa: E402
from ipc_amd import lib  # noqa: E402

WIND = (3.0, -1.0, 2.0)


def context(V, tri, x, term, dt=0.01):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    if term == "aero":
        c.set_aero([tri], 1.28, 0.1, False)
        c.aero_set_wind(WIND, 1.225)
    if term == "chamber":
        c.set_chambers([tri], [20.0])
    c.opt_init(dt, False)
    c.set_pattern()
    c.set_positions(x)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = icosphere(args.subdiv, RADIUS)
    x = V + 2e-5 * np.random.default_rng(0).standard_normal(V.shape)
    nTri, nV = len(tri), len(V)
    rec = {"tool": "bench_aero", "subdiv": args.subdiv, "nodes": int(nV), "triangles": int(nTri), "reps": args.reps, "wind": WIND}
    c = context(V, tri, x, "aero")
    rec["energy_ms"], _ = timed(c, lambda: c.aero_energy(1e-4), args.reps)
    rec["hessian_ms"], _ = timed(c, lambda: c.aero_hessian_add(1e-4, True), args.reps)
    rec["gradient_entry_point_ms"], _ = timed(c, lambda: c.aero_gradient_add(1e-4, True), args.reps)
    rec["state_ms"], _ = timed(c, lambda: c.aero_state(), args.reps)
    tot = np.zeros(5)
    rec["state_totals_only_ms"], _ = timed(c, lambda: c._chk(c._L.ipcgpu_aero_state(c.h, None, None, tot.ctypes.data_as(lib.c_dp))), args.reps)
    rec["assemble_newton_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    F, lag, tot = c.aero_state()
    rec["loaded_area_over_sphere"] = float(tot[4] / (4.0 * np.pi * RADIUS ** 2))
    rec["total_force"], rec["power"] = [float(v) for v in tot[:3]], float(tot[3])
    del c
    c = context(V, tri, x, "chamber")
    rec["chamber_hessian_ms"], _ = timed(c, lambda: c.chamber_hessian_add(1e-4, True), args.reps)
    rec["chamber_assemble_newton_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    del c
    c = context(V, tri, x, None)
    rec["assemble_newton_without_term_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    del c
    rec["gradient_plus_hessian_ms_by_difference"] = rec["assemble_newton_ms"] - rec["assemble_newton_without_term_ms"]
    rec["chamber_gradient_plus_hessian_ms_by_difference"] = rec["chamber_assemble_newton_ms"] - rec["assemble_newton_without_term_ms"]
    rec["hessian_over_chamber_hessian"] = rec["hessian_ms"] / rec["chamber_hessian_ms"]
    read_bytes = (16 + 64) * nTri + 24 * nV
    rec["algorithmic_read_bytes"] = int(read_bytes)
    rec["byte_bound_ms"] = read_bytes / ACHIEVABLE_BW * 1e3
    for k in ("energy_ms", "hessian_ms", "state_totals_only_ms"):
        rec[k.replace("_ms", "_over_byte_bound")] = rec[k] / rec["byte_bound_ms"]
    rec["atomic_adds_per_hessian"] = int(45 * nTri)
    rec["hessian_atomic_adds_per_s"] = 45 * nTri / (rec["hessian_ms"] * 1e-3)
    rec["refresh"] = "not timed: no entry point of its own"
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
