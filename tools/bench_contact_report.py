"""Cost of one `contact_report` call at the state of the contact bench (2 x mat100 stack, tools/bench_contact.py), beside one
`contact_gradient_add` call on the same sets -- the same stencil evaluation plus a deterministic scatter.  Both calls return synchronised, so each is timed
on the host around the call (median of 30); the sheets are two components.  Prints one JSON line.
usage: python tools/bench_contact_report.py [--n 100] [--steps 3] [--reps 30]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipc_amd import lib, scene  # noqa: E402


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(min(t))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    V, F, nA = scene.make_mat_stack(a.n, 2, gap=1.2e-3)
    SF = scene.surface_tris(F)
    c = lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_components([nA, V.shape[0]], [int((F < nA).all(1).sum()), F.shape[0]])
    c.set_positions(scene.jitter(V, F, rel=2e-3))
    c.opt_init(0.01, True)
    c.set_surface(SF)
    low = np.arange(nA)
    c.set_dbc(low[(np.abs(V[:nA, 0]) > 0.49) | (np.abs(V[:nA, 2]) > 0.49)].astype(np.int32), 1)
    c.enable_self_collision(1e-3)
    vel = np.zeros_like(V)
    vel[nA:, 1] = -0.05
    c.set_velocity(vel)
    c.precompute()
    for _ in range(a.steps):
        c.solve_timestep(12)
    st, cs = c.state(), c.contact_state()
    rows = c.contact_report(st["dHat"], st["kappa"])
    rep = median_ms(lambda: c.contact_report(st["dHat"], st["kappa"]), a.reps)
    grad = median_ms(lambda: c.contact_gradient_add(st["dHat"], st["kappa"], projectDBC=False), a.reps)
    print(json.dumps({"scene": f"2 x mat{a.n} stack after {a.steps} time steps", "n_active": cs["nActive"], "n_mollified": cs["nPara"], "rows": len(rows),
                      "tuples_below_dHat": int(sum(int(r[k]) for r in rows for k in ("nPP", "nPE", "nPT", "nEE", "nMollified"))),
                      "contact_report_ms_median": rep[0], "contact_report_ms_min": rep[1], "contact_gradient_add_ms_median": grad[0],
                      "contact_gradient_add_ms_min": grad[1], "reps": a.reps, "timing": "host clock around the synchronised call"}))
    c.close()
