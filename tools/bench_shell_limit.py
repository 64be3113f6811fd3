"""Strain-limit kernels of the shells on hardware (not part of bench.py): HIP-event times of the limit energy, its gradient alone and gradient plus Hessian
on the n x n-node cloth of tools/bench_shell.py, pre-stretched so that about half of its triangles are inside the barrier's range.  Prints one JSON line
(committed as profiles/shell_limit_bench.json).
  * the cloth is stretched along x by 0.9 + 0.2 x (x in [0, 1]) and compressed to 0.98 across: triangles right of the middle are past the onset 1.0, the others
    below it in every direction; the largest stretch is 1.1 (1.13 with the noise on the nodes), the limit 1.15;
  * events are recorded on the context's own stream around the entry points, as bench_shell.py does; ipcgpu_shell_limit_gradient_add carries its vector to
    the device and back (3 nV doubles each way), which its event pair includes -- the kernel alone is the difference of the two Newton assemblies below;
  * gradient plus Hessian in one launch is what the stepper runs: ipcgpu_assemble_newton with the limit set minus the same call with the limit removed.
usage: python tools/bench_shell_limit.py [--n 200] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from bench_shell import context, grid  # noqa: E402

ONSET, LIMIT = 1.0, 1.15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = grid(args.n, 1.0 / (args.n - 1))
    x = V + 2e-5 * np.random.default_rng(0).standard_normal(V.shape)  # (0.4 % of the spacing: the stretches stay below the limit)
    x[:, 0] = 0.9 * x[:, 0] + 0.1 * x[:, 0] ** 2  # d x' / d x = 0.9 + 0.2 x
    x[:, 2] *= 0.98
    c = context(V, tri)
    c.set_shell_strain_limit(LIMIT, ONSET)
    c.set_pattern()
    c.set_positions(x)
    sigma, ratio = c.shell_stretch()
    per = c.shell_limit_energy_per_elem()
    rec = {"tool": "bench_shell_limit", "nodes": int(len(V)), "triangles": int(len(tri)), "active_triangles": int(np.count_nonzero(per > 0)),
           "largest_stretch": float(sigma[:, 0].max()), "max_ratio": float(ratio), "reps": args.reps}
    assert ratio < 1.0 and np.all(np.isfinite(per))
    rec["energy_ms"], _ = timed(c, lambda: c.shell_limit_energy(1e-4), args.reps)
    rec["stretch_query_ms"], _ = timed(c, lambda: c.shell_stretch(), args.reps)
    rec["gradient_only_with_vector_copies_ms"], _ = timed(c, lambda: c.shell_limit_gradient_add(1e-4, True), args.reps)
    rec["hessian_only_ms"], _ = timed(c, lambda: c.shell_limit_hessian_add(1e-4, True), args.reps)
    rec["membrane_plus_hinge_plus_limit_hessian_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
    rec["assemble_newton_gradient_and_hessian_with_limit_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    rec["assemble_newton_gradient_with_limit_ms"], _ = timed(c, lambda: c.gradient(1e-4, True), args.reps)
    c.set_shell_strain_limit(None)
    rec["assemble_newton_gradient_and_hessian_without_limit_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    rec["assemble_newton_gradient_without_limit_ms"], _ = timed(c, lambda: c.gradient(1e-4, True), args.reps)
    rec["membrane_plus_hinge_hessian_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
    rec["gradient_plus_hessian_ms_by_difference"] = (rec["assemble_newton_gradient_and_hessian_with_limit_ms"]
                                                     - rec["assemble_newton_gradient_and_hessian_without_limit_ms"])
    rec["gradient_only_ms_by_difference"] = rec["assemble_newton_gradient_with_limit_ms"] - rec["assemble_newton_gradient_without_limit_ms"]
    # what limits the kernel (a belief to test, not a measurement): an active triangle adds 3 x 6 + 3 x 9 = 45 Hessian entries, 9 more with the gradient
    adds = 45 * rec["active_triangles"]
    rec["atomic_adds_per_hessian"] = int(adds)
    rec["atomic_adds_per_s"] = adds / (rec["hessian_only_ms"] * 1e-3)
    rec["believed_bound"] = {"energy": "latency of two small launches (kernel + one-workgroup reduction) and the read-back",
                             "gradient": "launch latency; 9 fp64 atomics per active triangle",
                             "hessian": "L2 fp64 atomics, 45 adds per active triangle, as the membrane's scatter -- no eigen-iteration in front of them"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
