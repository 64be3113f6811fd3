"""Pressure-chamber kernels on hardware (not part of bench.py): HIP-event times of the energy, the gradient + Hessian and the state query on one icosphere
chamber that is also a shell (default: 6 subdivisions, 81 920 triangles, 40 962 nodes, radius 0.1, slightly perturbed), and the Newton iterations per step
of a 20-step inflation of that sphere from rest.  Prints one JSON line (committed as profiles/chamber_bench.json).
  * events are recorded on the context's own stream around the C entry points, which add up- and downloads of their arguments (tools/bench_attach.py): the
    energy a few bytes, the state query three small arrays, the gradient entry point a vector of 3 nV doubles each way -- so the assemble kernel is timed
    through ipcgpu_chamber_hessian_add (no transfer beyond the 4-byte error flag) and through ipcgpu_assemble_newton with and without the chamber;
  * medians of --reps;
  * byte bound: what one pass has to read at least -- 3 node ids and 1 chamber id per triangle (16 B) and every node's position once (24 B) -- at the
    6.3 TB/s a copy kernel reaches on this part; the Hessian adds 54 fp64 atomic adds per triangle (3 diagonal blocks of 6, 3 off-diagonal blocks of 9)
    beside the 9 of the gradient.
usage: python tools/bench_chamber.py [--subdiv 6] [--reps 20] [--steps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from ipc_amd import lib  # noqa: E402

H, YM, PR, RHO, RADIUS = 1e-3, 1e5, 0.3, 1000.0, 0.1
ACHIEVABLE_BW = 6.3e12


def icosphere(subdiv, radius):
    """(nodes on the sphere, outward triangles): an icosahedron, every triangle split in four `subdiv` times"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    T = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
                  (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    V = np.array(V, dtype=np.float64)
    for _ in range(subdiv):
        n = len(V)
        e = np.sort(np.vstack([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = n + inv.reshape(3, -1).T  # per triangle the midpoints of (0,1), (1,2), (2,0)
        V = np.vstack([V, 0.5 * (V[ue[:, 0]] + V[ue[:, 1]])])
        a, b, c = T[:, 0], T[:, 1], T[:, 2]
        ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
        T = np.vstack([np.column_stack([a, ab, ca]), np.column_stack([b, bc, ab]), np.column_stack([c, ca, bc]), np.column_stack([ab, bc, ca])])
    V = radius * V / np.linalg.norm(V, axis=1)[:, None]
    y = V[T]
    if np.einsum("ti,ti->", y[:, 0], np.cross(y[:, 1], y[:, 2])) < 0:
        T = T[:, ::-1]
    return V, np.ascontiguousarray(T, dtype=np.int32)


def context(V, tri, x, p, dt=0.01, gravity=False):
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    if p is not None:
        c.set_chambers([tri], [p])
    c.opt_init(dt, gravity)
    c.set_pattern()
    c.set_positions(x)
    return c


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
    rec = {"tool": "bench_chamber", "subdiv": args.subdiv, "nodes": int(nV), "triangles": int(nTri), "reps": args.reps, "pressure": args.pressure}
    c = context(V, tri, x, args.pressure)
    rec["energy_ms"], _ = timed(c, lambda: c.chamber_energy(1e-4), args.reps)
    rec["hessian_ms"], _ = timed(c, lambda: c.chamber_hessian_add(1e-4, True), args.reps)
    rec["gradient_entry_point_ms"], _ = timed(c, lambda: c.chamber_gradient_add(1e-4, True), args.reps)
    rec["state_ms"], _ = timed(c, lambda: c.chamber_state(), args.reps)
    rec["assemble_newton_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    vol, area, _ = c.chamber_state()
    rec["volume_over_sphere"], rec["area_over_sphere"] = float(vol[0] / (4.0 / 3.0 * np.pi * RADIUS ** 3)), float(area[0] / (4.0 * np.pi * RADIUS ** 2))
    del c
    c = context(V, tri, x, None)
    rec["assemble_newton_without_chamber_ms"], _ = timed(c, lambda: c.assemble_newton(1e-4, True, with_gradient=True), args.reps)
    del c
    rec["gradient_plus_hessian_ms_by_difference"] = rec["assemble_newton_ms"] - rec["assemble_newton_without_chamber_ms"]
    read_bytes = 16 * nTri + 24 * nV
    rec["algorithmic_read_bytes"] = int(read_bytes)
    rec["byte_bound_ms"] = read_bytes / ACHIEVABLE_BW * 1e3
    for k in ("energy_ms", "hessian_ms", "state_ms"):
        rec[k.replace("_ms", "_over_byte_bound")] = rec[k] / rec["byte_bound_ms"]
    rec["state_reads_twice_byte_bound_ms"] = 2 * rec["byte_bound_ms"]
    rec["atomic_adds_per_hessian"] = int(54 * nTri)
    rec["hessian_atomic_adds_per_s"] = 54 * nTri / (rec["hessian_ms"] * 1e-3)
    # the inflation: the sphere at rest, free, no gravity, backward Euler, the constant pressure switched on at once
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    c.set_chambers([tri], [args.pressure])
    c.opt_init(0.01, False)
    c.set_time_integration("BE")
    c.set_rel_tol(1e-5)
    c.precompute()
    v0 = c.chamber_state()[0][0]
    its = [int(c.solve_timestep(200)) for _ in range(args.steps)]
    rec["inflation"] = {"steps": args.steps, "dt": 0.01, "rel_tol": 1e-5, "newton_iterations_per_step": its, "volume_over_rest": float(c.chamber_state()[0][0] / v0)}
    rec["believed_bound"] = {"energy": "latency of two small launches (the kernel and its one-workgroup reduction) and the read-back",
                             "hessian": "the Jacobi sweeps of the 9 x 9 projection at one wave per SIMD (compute), then 54 fp64 atomic adds per triangle",
                             "state": "one workgroup reads the whole chamber twice: latency of a single CU's loads, not bandwidth"}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
