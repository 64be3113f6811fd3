"""Attachment kernels on hardware (not part of bench.py): HIP-event times of the energy, the gradient + Hessian and the state query on two cloths stitched
node to node (default: two 200 x 200-node cloths one above the other, 40 000 attachments, slightly perturbed).  Prints one JSON line (committed as
profiles/attach_bench.json).
  * events are recorded on the context's own stream (ipcgpu_ctx_get_stream) through torch.cuda.ExternalStream around ipcgpu_attach_energy /
    ipcgpu_assemble-style entry points; the entry points add up- and downloads of their arguments, which the event pair includes: the energy a few
    bytes, the state query two arrays of n doubles, the gradient entry point a vector of 3 nV doubles each way -- so the kernel is timed through
    ipcgpu_attach_hessian_add (no transfer beyond the 4-byte error flag) and through ipcgpu_assemble_newton with and without attachments;
  * medians of --reps.
usage: python tools/bench_attach.py [--side 200] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from ipc_amd import lib  # noqa: E402

H, YM, PR, RHO = 1e-3, 1e5, 0.3, 1000.0


def cloth(n, spacing, y):
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    V = np.column_stack([i.ravel() * spacing, np.full(i.size, y), j.ravel() * spacing])
    a = (i[:-1, :-1] + n * j[:-1, :-1]).ravel()
    tri = np.vstack([np.column_stack([a, a + 1, a + n + 1]), np.column_stack([a, a + n + 1, a + n])])
    return V, tri.astype(np.int32)


def context(V, tri, x, stitches, L):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    if stitches is not None:
        c.set_attachments(stitches[0], stitches[1], 100.0, L)
    c.opt_init(0.01, True)
    c.set_pattern()
    c.set_positions(x)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n = args.side
    Va, tri = cloth(n, 0.01, 1.0)
    Vb, _ = cloth(n, 0.01, 1.02)
    V = np.vstack([Va, Vb])
    tri2 = np.vstack([tri, tri + n * n]).astype(np.int32)
    x = V + 2e-4 * np.random.default_rng(0).standard_normal(V.shape)
    stitches = (np.arange(n * n, dtype=np.int32), np.arange(n * n, dtype=np.int32) + n * n)
    rec = {"tool": "bench_attach", "side": n, "nodes": int(len(V)), "attachments": int(n * n), "reps": args.reps}
    for name, L in (("stitch", 0.0), ("tether", 0.015)):
        c = context(V, tri2, x, stitches, L)
        rec[f"{name}_energy_ms"], _ = timed(c, lambda: c.attach_energy(1e-4), args.reps)
        rec[f"{name}_hessian_ms"], _ = timed(c, lambda: c.attach_hessian_add(1e-4, True), args.reps)
        rec[f"{name}_gradient_entry_point_ms"], _ = timed(c, lambda: c.attach_gradient_add(1e-4, True), args.reps)
        rec[f"{name}_state_ms"], _ = timed(c, lambda: c.attach_state(), args.reps)
        rec[f"{name}_assemble_newton_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
        del c
    c = context(V, tri2, x, None, 0.0)
    rec["assemble_newton_without_attachments_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    del c
    for name in ("stitch", "tether"):
        rec[f"{name}_gradient_plus_hessian_ms_by_difference"] = rec[f"{name}_assemble_newton_ms"] - rec["assemble_newton_without_attachments_ms"]
    # Atomic adds per Hessian of a node-to-node attachment: 2 diagonal blocks of 6 upper entries + 1 off-diagonal block of 9 = 21 (the rod's segment)
    adds = 21 * rec["attachments"]
    rec["atomic_adds_per_hessian"] = int(adds)
    for name in ("stitch", "tether"):
        rec[f"{name}_atomic_adds_per_s"] = adds / (rec[f"{name}_hessian_ms"] * 1e-3)
    rec["rod_stretch_atomic_adds_per_s_for_comparison"] = 21.5e9
    rec["believed_bound"] = {"energy": "latency of two small launches (the kernel and its one-workgroup reduction) and the read-back",
                             "hessian": "launch latency and the read-back of the error flag at this size; fp64 atomics beyond it (21 adds per attachment)",
                             "state": "the download of two arrays of n doubles"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
