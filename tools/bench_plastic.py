"""The plastic-flow kernel on hardware (not part of bench.py): HIP-event times of k_plastic_flow on the mat150 mesh (scene.make_mat(150), the headline
workload's) with every element yielding and with none yielding, and -- the yardstick, in the same run on the same mesh -- launch_energy_per_elem.  Prints
one JSON line (committed as profiles/plastic_bench.json).
  * events are recorded on the context's own stream around the C entry points: ipcgpu_plastic_update adds a 8-byte memset and a 8-byte download of the two
    counters, ipcgpu_elastic_energy_per_elem an allocation and the download of nT doubles (reported as it is, and the download alone beside it);
  * "all yielding": yield 0 and a creep rate so small (r = 1e-5 per flow) that the state hardly moves, so that every repetition rewrites every element;
    "none yielding": a yield strain no element reaches, so that every element is evaluated (SVD, logarithms) and none is written;
  * medians of --reps;
  * byte bound: per element 16 B of node ids, four gathered positions (96 B), 72 B of A, the three parameters and alpha (32 B) read, and 80 B (A and alpha)
    written per element that yielded -- at the 6.3 TB/s a copy kernel reaches on this part.
usage: python tools/bench_plastic.py [--n 150] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timed  # noqa: E402
from bench_chamber import ACHIEVABLE_BW  # noqa: E402
from ipc_amd import lib, scene  # noqa: E402

DT = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    V, T = scene.make_mat(args.n)
    nV, nT = len(V), len(T)
    x = V * np.array([1.05, 0.98, 1.0]) + 1e-4 * float(np.ptp(V[:, 0]) / args.n) * np.random.default_rng(0).standard_normal(V.shape)
    c = lib.Context(0)
    c.set_mesh(V, T, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(DT, False)
    c.set_positions(x)
    rec = {"tool": "bench_plastic", "n": args.n, "nodes": int(nV), "tets": int(nT), "reps": args.reps}
    rec["energy_per_elem_ms"], _ = timed(c, c.elastic_energy_per_elem, args.reps)
    c.set_plasticity((0, nT), 1e3)
    rec["flow_none_yielding_ms"], _ = timed(c, lambda: c.plastic_update(DT), args.reps)
    rec["none_yielding_counts"] = list(c.plastic_update(DT))
    c.set_plasticity((0, nT), 0.0, creep=1e-5 / DT)
    rec["flow_all_yielding_ms"], _ = timed(c, lambda: c.plastic_update(DT), args.reps)
    rec["all_yielding_counts"] = list(c.plastic_update(DT))
    rec["state_totals_only_ms"], _ = timed(c, lambda: c.plastic_state(per_elem=False), args.reps)
    rec["max_alpha_after"] = float(c.plastic_state(per_elem=False)[1][2])
    read_bytes, write_bytes = (16 + 96 + 72 + 32) * nT, 80 * nT
    rec["algorithmic_read_bytes"], rec["algorithmic_write_bytes_all_yielding"] = int(read_bytes), int(write_bytes)
    rec["byte_bound_none_ms"] = read_bytes / ACHIEVABLE_BW * 1e3
    rec["byte_bound_all_ms"] = (read_bytes + write_bytes) / ACHIEVABLE_BW * 1e3
    rec["flow_none_over_byte_bound"] = rec["flow_none_yielding_ms"] / rec["byte_bound_none_ms"]
    rec["flow_all_over_byte_bound"] = rec["flow_all_yielding_ms"] / rec["byte_bound_all_ms"]
    rec["flow_all_over_energy_per_elem"] = rec["flow_all_yielding_ms"] / rec["energy_per_elem_ms"]
    rec["flow_none_over_energy_per_elem"] = rec["flow_none_yielding_ms"] / rec["energy_per_elem_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
