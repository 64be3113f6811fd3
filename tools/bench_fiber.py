"""Times of the fibre kernels (ipc_amd/csrc/fiber_kernels.hip) on a mat150-sized mesh (scene.make_mat(150): 45 000 nodes, 133 206 tets) with EVERY element
fibred, and of the tetrahedral assembly beside them in the same run.  One JSON line.  HIP events on the context's stream around the C entry points
(tools/_timing.py): an entry point's time holds its launches and what it reads back (a scalar for the energy, the error flag for the Hessian, the three totals
for the state); the gradient entry point also moves the 3 nV vector both ways and is listed for completeness only.
Two yardsticks from the same run: `tet_launch_assemble_ms` is ipcgpu_elastic_hessian_add, the tet launch_assemble alone into the same matrix (no gradient, one
synchronisation) -- what `assemble_hessian_ms` of the fibres (matrix only, plus the read-back of the error flag) is compared with; and
`tet_assemble_newton_ms`, the stepper's whole assembly WITH gradient (patch kernels, not launch_assemble), whose difference with and without fibres is the fibre
term as the stepper pays for it (gradient and matrix in one launch).  That difference of two medians can be dominated by their spread: it is given, with the
spread (median - minimum) of both, and no rate is derived from it.

The fibre assemble issues at most 4 x 3 + 4 x 6 + 6 x 9 = 90 fp64 atomic adds per element (closed-form projection; a node whose coefficient c_i is exactly 0
issues none: `atomic_adds_issued` counts them from b = A a of this mesh, the matrix-only launch issuing the 78 of them that are not gradient entries); the tet
assemble eigen-projects a 12 x 12 block per element.

usage: python tools/bench_fiber.py [--n 150] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from ipc_amd import lib, scene  # noqa: E402

DIR = (0.48, 0.6, 0.64)


def context(V, F, x, law, dt=0.04):
    c = lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    if law is not None:
        c.set_fibers((0, len(F)), DIR, 1e4, law=law, k2=2.0)
        if law == "spring":
            c.fiber_set_activation(0, 0.2)
    c.opt_init(dt, False)
    c.set_pattern()
    c.set_positions(x)
    c.set_xtilde(x)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, F = scene.make_mat(args.n)
    x = V * np.array([1.03, 1.0, 1.02]) + 1e-5 * np.random.default_rng(0).standard_normal(V.shape)  # a little stretched along the fibres: every lane is on
    nT, nV = len(F), len(V)
    rec = {"tool": "bench_fiber", "n": args.n, "nodes": int(nV), "tets": int(nT), "reps": args.reps}
    base = context(V, F, x, None)
    rec["tet_launch_assemble_ms"], lo = timed(base, lambda: base.elastic_hessian_add(1.6e-3, True), args.reps)
    rec["tet_launch_assemble_spread_ms"] = rec["tet_launch_assemble_ms"] - lo
    rec["tet_assemble_newton_ms"], lo = timed(base, lambda: base.assemble_newton(1.6e-3, True, with_gradient=True), args.reps)
    rec["tet_assemble_newton_spread_ms"] = rec["tet_assemble_newton_ms"] - lo
    A = base.features()["restTriInv"].reshape(nT, 3, 3).transpose(0, 2, 1)  # column-major inside the 9
    b = A @ (np.asarray(DIR) / np.linalg.norm(DIR))
    m = (b != 0.0).sum(1) + (b.sum(1) != 0.0)  # nodes with c_i != 0
    rec["atomic_adds_issued"] = int((3 * m + 6 * m + 9 * m * (m - 1) // 2).sum())
    rec["atomic_adds_issued_matrix_only"] = int((6 * m + 9 * m * (m - 1) // 2).sum())
    del base
    for law in ("spring", "exp"):
        c = context(V, F, x, law)
        assert c.fiber_get()["n"] == nT
        r = {}
        r["energy_ms"], _ = timed(c, lambda: c.fiber_energy(1.6e-3), args.reps)
        r["assemble_hessian_ms"], _ = timed(c, lambda: c.fiber_hessian_add(1.6e-3, True), args.reps)
        tot = np.zeros(3)
        r["state_totals_only_ms"], _ = timed(c, lambda: c._chk(c._L.ipcgpu_fiber_state(c.h, None, tot.ctypes.data_as(lib.c_dp))), args.reps)
        r["state_ms"], _ = timed(c, lambda: c.fiber_state(), args.reps)
        r["gradient_entry_point_ms"], _ = timed(c, lambda: c.fiber_gradient_add(1.6e-3, True), args.reps)
        r["assemble_newton_ms"], lo = timed(c, lambda: c.assemble_newton(1.6e-3, True, with_gradient=True), args.reps)
        r["assemble_newton_spread_ms"] = r["assemble_newton_ms"] - lo
        r["gradient_plus_hessian_ms_by_difference"] = r["assemble_newton_ms"] - rec["tet_assemble_newton_ms"]
        r["assemble_hessian_over_tet_launch_assemble"] = r["assemble_hessian_ms"] / rec["tet_launch_assemble_ms"]
        r["energy_over_tet_launch_assemble"] = r["energy_ms"] / rec["tet_launch_assemble_ms"]
        r["state_totals_only_over_tet_launch_assemble"] = r["state_totals_only_ms"] / rec["tet_launch_assemble_ms"]
        r["stretch_min_max"] = [float(v) for v in c.fiber_state(per_elem=False)[1][:2]]
        rec[law] = r
        del c
    rec["atomic_adds_per_element_at_most"] = 90
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
