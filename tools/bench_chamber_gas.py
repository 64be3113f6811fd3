"""The gas law of the pressure chambers on hardware (not part of bench.py), on the icosphere of tools/bench_chamber.py (default: 81 920 triangles, 40 962 nodes)
as ONE gas chamber.  Prints one JSON line (committed as profiles/chamber_gas_bench.json).  Medians of --reps, HIP events on the context's stream (tools/_timing.py).
  * gas energy evaluation: ipcgpu_chamber_energy on the gas chamber -- both passes of the volume reduction (320 slices; one wave for the chamber) --, beside
    the constant chamber's ipcgpu_chamber_energy and the one-workgroup ipcgpu_chamber_state of the same sphere in the same run; the byte bound is
    bench_chamber.py's (16 B per triangle, 24 B per node at 6.3 TB/s);
  * Newton-iteration cost, k = 1: ipcgpu_chamber_gas_solve beside ipcgpu_linsys_solve on the same factor (both move 3 nV doubles each way: the difference is
    the gas update, gradV, the second solve, the dot products, the small solve and the apply), and the wall time per Newton iteration of the inflation below
    beside the same inflation with a constant chamber;
  * the 20-step inflation of bench_chamber.py with ambient = 1e5 (gamma 1.4): Newton iterations per step, gas and constant.
usage: python tools/bench_chamber_gas.py [--subdiv 6] [--reps 20] [--steps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from bench_chamber import ACHIEVABLE_BW, H, PR, RADIUS, RHO, YM, context, icosphere  # noqa: E402
from ipc_amd import lib  # noqa: E402

AMBIENT, GAMMA = 1.0e5, 1.4


def inflation(V, tri, p, gas, steps):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    c.set_chambers([tri], [p])
    if gas:
        c.chamber_set_gas(True, AMBIENT, GAMMA)
    c.opt_init(0.01, False)
    c.set_time_integration("BE")
    c.set_rel_tol(1e-5)
    c.precompute()
    v0 = c.chamber_gas_state()[0][0]
    first = int(c.solve_timestep(200))  # (the first step carries the symbolic analysis: counted, not timed)
    t0 = time.perf_counter()
    its = [int(c.solve_timestep(200)) for _ in range(steps - 1)]
    wall = time.perf_counter() - t0
    vol, gauge, _ = c.chamber_gas_state()
    return {"steps": steps, "dt": 0.01, "rel_tol": 1e-5, "newton_iterations_per_step": [first] + its, "ms_per_newton_iteration_after_the_first_step": 1e3 * wall / max(1, sum(its) + len(its)),
            "volume_over_rest": float(vol[0] / v0), "gauge": float(gauge[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pressure", type=float, default=20.0)
    args = ap.parse_args()
    V, tri = icosphere(args.subdiv, RADIUS)
    x = V + 2e-5 * np.random.default_rng(0).standard_normal(V.shape)
    nTri, nV = len(tri), len(V)
    rec = {"tool": "bench_chamber_gas", "subdiv": args.subdiv, "nodes": int(nV), "triangles": int(nTri), "reps": args.reps, "pressure": args.pressure,
           "ambient": AMBIENT, "gamma": GAMMA, "slices": int(-(-nTri // 256))}
    c = context(V, tri, x, args.pressure)
    rec["constant_energy_ms"], _ = timed(c, lambda: c.chamber_energy(1e-4), args.reps)
    rec["state_ms"], _ = timed(c, lambda: c.chamber_state(), args.reps)
    c.chamber_set_gas(True, AMBIENT, GAMMA)
    rec["gas_energy_ms"], _ = timed(c, lambda: c.chamber_energy(1e-4), args.reps)
    rec["gas_state_entry_point_ms"], _ = timed(c, lambda: c.chamber_gas_state(), args.reps)
    rec["byte_bound_ms"] = (16 * nTri + 24 * nV) / ACHIEVABLE_BW * 1e3
    rec["gas_energy_over_byte_bound"] = rec["gas_energy_ms"] / rec["byte_bound_ms"]
    rec["state_over_gas_energy"] = rec["state_ms"] / rec["gas_energy_ms"]
    rec["gas_energy_over_constant_energy"] = rec["gas_energy_ms"] / rec["constant_energy_ms"]
    # the solve: the matrix of a Newton iteration at dt = 0.01, factorised once
    coef = 1e-4
    c.set_xtilde(x)
    c.assemble_newton(coef, True)
    c.analyze_pattern()
    assert c.factorize()
    rhs = np.random.default_rng(1).standard_normal(3 * nV)
    rec["plain_solve_ms"], _ = timed(c, lambda: c.solve(rhs), args.reps)
    rec["gas_solve_ms"], _ = timed(c, lambda: c.chamber_gas_solve(coef, rhs), args.reps)
    rec["rank_one_correction_ms"] = rec["gas_solve_ms"] - rec["plain_solve_ms"]
    del c
    rec["inflation_gas"] = inflation(V, tri, args.pressure, True, args.steps)
    rec["inflation_constant"] = inflation(V, tri, args.pressure, False, args.steps)
    rec["believed_bound"] = {"gas_energy": "latency of two small dependent launches and the read-back, as the constant energy",
                             "rank_one_correction": "a second pair of triangular sweeps on the retained factor; the dots and the apply stream 3 + 2 vectors of 3 nV doubles"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
