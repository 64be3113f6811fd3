"""Woven-cloth kernels on hardware (not part of bench.py): on the 81 920-triangle icosphere the other shell tools use, scaled 1.1 and perturbed, three contexts
of the same run -- the StVK shell, the all-rubber shell and the woven shell (warp: the z axis projected into every triangle; a triangle it is normal to
would stay StVK: the level-6 sphere has none) -- and HIP-event medians of the woven energy, assemble (gradient; Hessian) and state query beside ipcgpu_shell_hessian_add of the StVK shell (the
membrane and hinge kernels) and ipcgpu_shell_rubber_hessian_add of the rubber shell.  Prints one JSON line (committed as profiles/shell_weave_bench.json).
  * events are recorded on the context's own stream (tools/_timing.py); the entry points add a few-byte read-back each, which the event pair includes, the same
    for the three terms; the state query downloads 6 doubles per triangle, which its figure includes;
  * the StVK kernels are untouched: on a woven triangle they read zeros for their two constants; "stvk_bend0" is the StVK shell with `bend 0` (the membrane
    kernel and a hinge kernel that adds zeros), beside "stvk" with bending on.
usage: python tools/bench_shell_weave.py [--level 6] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from _timing import timed  # noqa: E402
from ipc_amd import lib  # noqa: E402

H, YM, PR, RHO = 1e-3, 1e5, 0.3, 1000.0
AXIS = np.array([0.0, 0.0, 1.0])
NO_T = np.zeros((0, 4), dtype=np.int32)


def context(V, tri, kind, woven=None, bend=1.0):
    c = lib.Context(0)
    c.set_mesh(V, NO_T, YM=YM, PR=0.4, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO, bend_scale=bend)
    if kind == "rubber":
        c.set_shell_membrane(1, 0.1)
    elif kind == "weave":
        c.set_shell_weave(woven, AXIS, 1e5, 5e4, 2e3, 0.25, 10.0, 1.0)
    c.opt_init(0.01, True)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from chamber_gas_mp import icosphere
    V, tri = icosphere(args.level)
    n = np.cross(V[tri[:, 1]] - V[tri[:, 0]], V[tri[:, 2]] - V[tri[:, 0]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    woven = (np.sqrt(1.0 - (n @ AXIS) ** 2) >= 1e-3).astype(np.int32)  # (the plan refuses a projection below 1e-6; the margin keeps the poles' triangles out)
    x = V * 1.1 + 2e-4 * np.random.default_rng(0).standard_normal(V.shape)
    rec = {"tool": "bench_shell_weave", "nodes": int(len(V)), "triangles": int(len(tri)), "woven": int(woven.sum()), "reps": args.reps}
    for label, kind, bend in (("stvk", "stvk", 1.0), ("stvk_bend0", "stvk", 0.0), ("rubber", "rubber", 1.0), ("weave", "weave", 1.0)):
        c = context(V, tri, kind, woven, bend)
        c.set_pattern()
        c.set_positions(x)
        r = {}
        r["shell_energy_ms"], _ = timed(c, lambda: c.shell_energy(1e-4), args.reps)
        r["shell_gradient_ms"], _ = timed(c, lambda: c.shell_gradient_add(1e-4, True), args.reps)
        r["shell_hessian_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
        if kind == "rubber":
            r["term_energy_ms"], _ = timed(c, lambda: c.shell_rubber_energy(1e-4), args.reps)
            r["term_gradient_ms"], _ = timed(c, lambda: c.shell_rubber_gradient_add(1e-4, True), args.reps)
            r["term_hessian_ms"], _ = timed(c, lambda: c.shell_rubber_hessian_add(1e-4, True), args.reps)
        if kind == "weave":
            r["term_energy_ms"], _ = timed(c, lambda: c.shell_weave_energy(1e-4), args.reps)
            r["term_gradient_ms"], _ = timed(c, lambda: c.shell_weave_gradient_add(1e-4, True), args.reps)
            r["term_hessian_ms"], _ = timed(c, lambda: c.shell_weave_hessian_add(1e-4, True), args.reps)
            r["state_ms"], _ = timed(c, c.shell_weave_state, args.reps)
        rec[label] = r
        del c
    rec["weave_over_rubber_assemble"] = rec["weave"]["term_hessian_ms"] / rec["rubber"]["term_hessian_ms"]
    rec["weave_over_stvk_shell_assemble"] = rec["weave"]["term_hessian_ms"] / rec["stvk"]["shell_hessian_ms"]
    rec["weave_over_stvk_bend0_shell_assemble"] = rec["weave"]["term_hessian_ms"] / rec["stvk_bend0"]["shell_hessian_ms"]
    rec["weave_over_rubber_energy"] = rec["weave"]["term_energy_ms"] / rec["rubber"]["term_energy_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
