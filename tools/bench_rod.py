"""Rod kernels on hardware (not part of bench.py): HIP-event times of the energy, stretch and bend kernels on a bundle of straight rods (default: 400
rods of 256 nodes side by side, slightly perturbed).  Prints one JSON line (committed as profiles/rod_bench.json).
  * events are recorded on the context's own stream (ipcgpu_ctx_get_stream) through torch.cuda.ExternalStream around ipcgpu_rod_energy /
    ipcgpu_rod_hessian_add; the entry points add a few-byte read-back each, which the event pair includes (tens of microseconds);
  * the stretch kernel alone is timed on the same bundle with bendScale = 0 (no triple reaches the kernels); the bend kernel is the difference to the
    bundle with bending on.
usage: python tools/bench_rod.py [--rods 400] [--nodes 256] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from ipc_amd import lib  # noqa: E402

R, YM, RHO = 2e-3, 1e7, 1000.0


def bundle(rods, nodes, spacing):
    """`rods` straight rods of `nodes` nodes along x, side by side in z"""
    i, j = np.meshgrid(np.arange(nodes), np.arange(rods))
    V = np.column_stack([i.ravel() * spacing, np.ones(i.size), -j.ravel() * 10 * spacing])
    a = (np.arange(nodes - 1)[None, :] + nodes * np.arange(rods)[:, None]).ravel()
    return V, np.column_stack([a, a + 1]).astype(np.int32)


def context(V, seg, bend):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=0.4, density=RHO)
    c.set_rod(seg, R, YM, RHO, bend_scale=bend)
    c.opt_init(0.01, True)
    c.set_pattern()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rods", type=int, default=400)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, seg = bundle(args.rods, args.nodes, 0.01)
    x = V + 2e-4 * np.random.default_rng(0).standard_normal(V.shape)
    c = context(V, seg, 1.0)
    c.set_positions(x)
    info = c.rod_get()
    rec = {"tool": "bench_rod", "rods": args.rods, "nodes": int(len(V)), "segments": int(info["nSeg"]), "triples": int(info["nBend"]), "reps": args.reps}
    rec["energy_ms"], _ = timed(c, lambda: c.rod_energy(1e-4), args.reps)
    rec["stretch_plus_bend_hessian_ms"], _ = timed(c, lambda: c.rod_hessian_add(1e-4, True), args.reps)
    rec["assemble_newton_with_rod_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=False), args.reps)
    del c
    s = context(V, seg, 0.0)
    s.set_positions(x)
    rec["stretch_hessian_ms"], _ = timed(s, lambda: s.rod_hessian_add(1e-4, True), args.reps)
    rec["bend_hessian_ms_by_difference"] = rec["stretch_plus_bend_hessian_ms"] - rec["stretch_hessian_ms"]
    del s
    # Atomic adds per Hessian: a diagonal block adds its 6 upper entries, an off-diagonal one 9: 2 x 6 + 9 = 21 per segment, 3 x 6 + 3 x 9 = 45 per triple
    adds = 21 * rec["segments"] + 45 * rec["triples"]
    rec["atomic_adds_per_hessian"] = int(adds)
    rec["atomic_adds_per_s"] = adds / (rec["stretch_plus_bend_hessian_ms"] * 1e-3)
    rec["stretch_atomic_adds_per_s"] = 21 * rec["segments"] / (rec["stretch_hessian_ms"] * 1e-3)
    rec["bend_atomic_adds_per_s"] = 45 * rec["triples"] / max(rec["bend_hessian_ms_by_difference"] * 1e-3, 1e-12)
    rec["atomic_ceiling_adds_per_s"] = 30e9  # the tet-parallel scatter
    rec["believed_bound"] = {"energy": "latency of two small launches (the kernel and its one-workgroup reduction) and the read-back",
                             "stretch": "launch latency and the read-back at this size; L2 fp64 atomics beyond it (21 adds per segment)",
                             "bend": "L2 fp64 atomics (45 adds per triple)"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
