"""The shells' plastic-flow kernels on hardware (not part of bench.py): HIP-event times of the two flow kernels and of the state kernel on the icosphere of
tools/bench_chamber.py (default: 6 subdivisions, 81 920 triangles, 40 962 nodes, 122 880 hinges, radius 0.1), inflated by 2 % with a perturbation, all
triangles plastic with the yield strains at the medians of the mesh's own strains so that half of the triangles and half of the hinges yield; and -- the
yardstick, in the same run on the same mesh -- launch_shell_assemble through ipcgpu_shell_hessian_add.  Prints one JSON line and writes it to
profiles/shell_plastic_bench.json.
  * events are recorded on the context's own stream around the C entry points (tools/_timing.py): ipcgpu_shell_plastic_update adds a 16-byte memset and a
    16-byte read-back of the counters to the two launches; the membrane flow and the hinge flow are also timed alone (the other switched off by +inf);
    every repetition starts from the reset records, and the reset (two device copies, three memsets) is timed alone and subtracted;
  * the state kernel is timed with the totals alone (two launches, two read-backs) and with its 8 (nTri + nHinge) doubles of downloads;
  * medians of --reps;
  * byte bound at the 6.3 TB/s a copy kernel reaches on this part: per triangle 3 node ids (12 B), 6 + 4 doubles read (80 B), at most 5 written (40 B); per
    hinge 4 node ids (16 B), 2 + 4 doubles read (48 B), at most 2 written (16 B); every node's position once per kernel (24 B).
usage: python tools/bench_shell_plastic.py [--subdiv 6] [--reps 20]"""
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

DT = 0.01
INF = float("inf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, tri = icosphere(args.subdiv, RADIUS)
    x = 1.02 * V + 2e-4 * np.random.default_rng(0).standard_normal(V.shape)
    c = lib.Context(0)
    c.set_mesh(V, np.zeros((0, 4), dtype=np.int32), YM=YM, PR=PR, density=RHO)
    c.set_shell(tri, H, YM, PR, RHO)
    c.opt_init(DT, False)
    c.set_pattern()
    c.set_positions(x)
    nTri, nV, nH = len(tri), len(V), c.shell_get()["nHinge"]
    rec = {"tool": "bench_shell_plastic", "subdiv": args.subdiv, "nodes": int(nV), "triangles": int(nTri), "hinges": int(nH), "reps": args.reps}
    c.shell_set_plasticity((0, nTri), 1e3, 1e3)  # nothing yields: only to read n and eps
    pt, ph, _ = c.shell_plastic_state()
    yld, yb = float(np.median(pt[:, 0])), float(np.median(ph[:, 0]))
    rec["yield"], rec["bend_yield"] = yld, yb

    def flow():
        c.shell_plastic_reset()
        return c.shell_plastic_update(DT)
    rec["reset_ms"], _ = timed(c, c.shell_plastic_reset, args.reps)
    for name, par in (("both", (yld, yb)), ("tri", (yld, INF)), ("hinge", (INF, yb)), ("none_yielding", (1e3, 1e3))):
        c.shell_set_plasticity((0, nTri), *par, creep=5.0, harden=0.5)
        rec[f"flow_{name}_counts"] = list(flow())
        ms, _ = timed(c, flow, args.reps)
        rec[f"flow_{name}_ms"] = ms - rec["reset_ms"]
    c.shell_set_plasticity((0, nTri), yld, yb, creep=5.0, harden=0.5)
    flow()
    tot = np.zeros(7)
    rec["state_totals_only_ms"], _ = timed(c, lambda: c._chk(c._L.ipcgpu_shell_plastic_state(c.h, None, None, tot.ctypes.data_as(lib.c_dp))), args.reps)
    rec["state_ms"], _ = timed(c, c.shell_plastic_state, args.reps)
    rec["max_alpha"], rec["max_alphaB"], rec["sum_hA_alpha"] = float(tot[4]), float(tot[5]), float(tot[6])
    rec["shell_assemble_ms"], _ = timed(c, lambda: c.shell_hessian_add(1e-4, True), args.reps)
    tri_bytes = (12 + 80) * nTri + 24 * nV + 40 * rec["flow_both_counts"][0]
    hinge_bytes = (16 + 48) * nH + 24 * nV + 16 * rec["flow_both_counts"][2]
    rec["algorithmic_bytes_tri"], rec["algorithmic_bytes_hinge"] = int(tri_bytes), int(hinge_bytes)
    rec["byte_bound_tri_ms"], rec["byte_bound_hinge_ms"] = tri_bytes / ACHIEVABLE_BW * 1e3, hinge_bytes / ACHIEVABLE_BW * 1e3
    rec["flow_tri_over_byte_bound"] = rec["flow_tri_ms"] / rec["byte_bound_tri_ms"]
    rec["flow_hinge_over_byte_bound"] = rec["flow_hinge_ms"] / rec["byte_bound_hinge_ms"]
    rec["flow_both_over_byte_bound"] = rec["flow_both_ms"] / (rec["byte_bound_tri_ms"] + rec["byte_bound_hinge_ms"])
    rec["flow_both_over_shell_assemble"] = rec["flow_both_ms"] / rec["shell_assemble_ms"]
    line = json.dumps(rec)
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shell_plastic_bench.json")
    try:
        with open(out, "w") as f:
            f.write(line + "\n")
    except OSError:
        pass  # (a read-only tree: the printed line is the result)


if __name__ == "__main__":
    main()
