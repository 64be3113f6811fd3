"""Round-collider entry points against the half-space's on the same vertices, in one run: the 81 920-triangle icosphere of tools/bench_chamber.py resting
just inside dHat of a hollow sphere, so that every vertex is active.  HIP-event medians of `--reps` calls of build, energy, gradient_add, hessian_add and
step_bound, then the same five calls of a half-space whose set is handed the same vertices (a plane cannot have them all inside dHat; the kernels do the
same work per entry whatever the distance).  Both columns are entry-point times: each includes its read-back (build: the set; gradient_add: 24 nV bytes
each way), alike for the two.  One JSON line.
    python tools/bench_round_collider.py > profiles/round_collider_bench.json"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from bench_chamber import H, PR, RADIUS, RHO, YM, icosphere  # noqa: E402
from ipc_amd import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = icosphere(args.subdiv, RADIUS)
    gap, dHat, kappa = 5e-4, 1e-6, 1e3  # every vertex at half the activation distance
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    c.opt_init(0.01, False)
    c.set_surface(tri)
    c.set_pattern()
    rc = c.add_sphere_collider([0.0, 0.0, 0.0], RADIUS + gap, True, 1e-3)
    hs = c.add_half_space([0.0, -2 * RADIUS, 0.0], [0.0, 1.0, 0.0], 1e-3)
    p = 1e-5 * np.random.default_rng(0).standard_normal(V.shape)
    rec = {"tool": "bench_round_collider", "subdiv": args.subdiv, "nodes": int(len(V)), "triangles": int(len(tri)), "reps": args.reps, "dHat": dHat,
           "gap": gap, "statistic": "median ms of HIP-event intervals around the entry point, after one warm-up call"}
    n = len(c.round_build(rc, dHat))
    assert n == len(V), (n, len(V))
    c.halfspace_set(hs, np.arange(len(V), dtype=np.int32))
    rec["active"] = int(n)
    g = np.zeros(3 * len(V))
    calls = {"build": (lambda: c.round_build(rc, dHat), lambda: c.halfspace_build(hs, dHat)),
             "energy": (lambda: c.round_energy(rc, dHat, kappa), lambda: c.halfspace_energy(hs, dHat, kappa)),
             "gradient_add": (lambda: c.round_gradient_add(rc, dHat, kappa, g), lambda: c.halfspace_gradient_add(hs, dHat, kappa, g)),
             "hessian_add": (lambda: c.round_hessian_add(rc, dHat, kappa, True), lambda: c.halfspace_hessian_add(hs, dHat, kappa, True)),
             "step_bound": (lambda: c.round_step_bound(rc, p, 0.9, 1.0), lambda: c.halfspace_step_bound(hs, p, 0.9, 1.0))}
    for name, (fr, fh) in calls.items():
        if name == "energy":  # (the half-space's build emptied its set: no vertex is inside dHat of the plane)
            c.halfspace_set(hs, np.arange(len(V), dtype=np.int32))
        rec[f"round_{name}_ms"], _ = timed(c, fr, args.reps)
        rec[f"halfspace_{name}_ms"], _ = timed(c, fh, args.reps)
        rec[f"{name}_ratio"] = rec[f"round_{name}_ms"] / rec[f"halfspace_{name}_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
