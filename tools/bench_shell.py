"""Shell kernels on hardware (not part of bench.py): HIP-event times of the energy, membrane and hinge kernels on an n x n-node cloth, and one Newton
iteration of a falling cloth with the shell terms beside the same scene with the cloth's elastic energy left out (both measured).  Prints one JSON line (committed as
profiles/shell_bench.json).
  * events are recorded on the context's own stream (ipcgpu_ctx_get_stream) through torch.cuda.ExternalStream around ipcgpu_shell_energy /
    ipcgpu_shell_hessian_add; the entry points add a few-byte read-back each, which the event pair includes (tens of microseconds);
  * the membrane kernel alone is timed on a "soup" of the same triangles with no shared node (no interior edge, hence no hinge); the hinge kernel is the
    difference to the connected cloth.  The soup scatters into more distinct rows, so the difference slightly favours the hinge kernel.
usage: python tools/bench_shell.py [--n 200] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from ipc_amd import lib, scene  # noqa: E402

H, YM, PR, RHO = 1e-3, 1e5, 0.3, 1000.0


def grid(n, spacing):
    V = np.array([[i * spacing, 1.0, -j * spacing] for j in range(n) for i in range(n)])
    a = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).ravel()
    tri = np.concatenate([np.column_stack([a, a + 1, a + n + 1]), np.column_stack([a, a + n + 1, a + n])]).astype(np.int32)
    return V, tri


def context(V, tri, dt=0.01, gravity=True):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=0.4, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    c.opt_init(dt, gravity)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = grid(args.n, 1.0 / (args.n - 1))
    rng = np.random.default_rng(0)
    x = V + 2e-4 * rng.standard_normal(V.shape)
    c = context(V, tri)
    c.set_pattern()
    c.set_positions(x)
    info = c.shell_get()
    rec = {"tool": "bench_shell", "nodes": int(len(V)), "triangles": int(info["nTri"]), "hinges": int(info["nHinge"]), "reps": args.reps}
    rec["energy_ms"], _ = timed(c, lambda: c.shell_energy(1e-4), args.reps)
    rec["membrane_plus_hinge_hessian_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
    rec["assemble_newton_with_shell_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=False), args.reps)
    # membrane alone: the same triangles without shared nodes
    Vs, xs = V[tri.ravel()], x[tri.ravel()]
    ts = np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3)
    s = context(Vs, ts)
    s.set_pattern()
    s.set_positions(xs)
    rec["membrane_hessian_ms"], _ = timed(s, lambda: s.shell_hessian_add(1e-4, True), args.reps)
    rec["hinge_hessian_ms_by_difference"] = rec["membrane_plus_hinge_hessian_ms"] - rec["membrane_hessian_ms"]
    del s
    del c
    # One Newton iteration with and without the shell terms, both measured: the crumpled cloth falling beside a small tetrahedral plate (no contact), once as
    # an elastic shell, once with the same nodes carrying the same masses but no elastic energy (ipcgpu_set_codim_nodes).  Same mesh, same surface; the run
    # with the shell also has the hinges' opposite pairs in its pattern.  Wall time per iteration of ipcgpu_opt_solve_timestep over three time steps.
    Vb, Tb = scene.make_bar(24, 2, 24, size=(1.0, 0.05, 1.0))
    Vb = Vb + np.array([0.0, -1.0, 0.0]) - Vb.min(0)
    Vall, xall = np.vstack([Vb, V]), np.vstack([Vb, x])
    triAll = tri + len(Vb)
    SF = np.vstack([scene.surface_tris(Tb), triAll]).astype(np.int32)
    for label, with_shell in (("with_shell", True), ("without_shell_terms", False)):
        k = lib.Context(0)
        k.set_mesh(Vall, Tb, YM=YM, PR=0.4, density=RHO)
        if with_shell:
            k.set_shell(triAll, H, YM, PR, RHO)
        else:
            k.set_codim_nodes(np.arange(len(Vb), len(Vall)), info["mass"])
        k.set_positions(xall)
        k.opt_init(0.01, True)
        k.set_surface(SF)
        k.set_rel_tol(1e-6)
        k.precompute()
        its, t0 = 0, time.time()
        for _ in range(3):
            its += k.solve_timestep(30)
        rec[f"newton_iterations_{label}"] = its
        rec[f"newton_iteration_{label}_ms"] = 1e3 * (time.time() - t0) / max(its, 1)
        del k
    # what limits each kernel (a belief to test, not a measurement).  Atomic adds per Hessian: a diagonal block adds its 6 upper entries, an off-diagonal one 9:
    # 3 x 6 + 3 x 9 = 45 per triangle, 4 x 6 + 6 x 9 = 78 per hinge
    nnz_adds = 45 * rec["triangles"] + 78 * rec["hinges"]
    rec["atomic_adds_per_hessian"] = int(nnz_adds)
    rec["atomic_adds_per_s"] = nnz_adds / (rec["membrane_plus_hinge_hessian_ms"] * 1e-3)
    rec["believed_bound"] = {"energy": "latency of a single small launch plus its one-workgroup reduction (1.2 MB read)",
                             "membrane": "fp64 issue of the 6 x 6 Jacobi sweeps at 3 waves per SIMD, then L2 atomics (45 adds per triangle)",
                             "hinge": "L2 fp64 atomics (78 adds per hinge, 12 more with the gradient): DESIGN.md section 4 puts them at ~30 G adds/s"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
