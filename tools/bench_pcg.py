"""The iterative solver (solver type 2) beside the multifrontal factorisation, on the two matrices the project measures everything else on:
the headline workload's (mat150 twist, bench.py) and the contact bench's (tools/bench_contact.py).  One JSON record:

  per solve, on each matrix: type 0 factorise + solve; type 2 with each preconditioner at 1e-5 and at 1e-10 (iterations, ms, true residual)
  lagged factor: a Newton run of the headline workload with max_factor_age 1, 2, 4, 8, 16 (ms per Newton iteration, Newton count, CG iterations)
  the product kernel's achieved bytes/s against its algorithmic bytes (8 nnz values + 4 nnz columns + the two vectors, each once)

usage: python tools/bench_pcg.py [--n 150] [--contact-n 60] [--newton 40] [--out profiles/pcg_bench.json]
       python tools/bench_pcg.py --two-level [--n 150] [--contact-n 60] [--large-n 0] [--out profiles/pcg_two_level_bench.json]
--two-level: the two-level preconditioner (precond 2) beside block Jacobi and the multifrontal solve, per solve, on the same matrices (and on the
3 x mat<large-n> stack of contact_large when --large-n is given); per row iterations, ms per solve, ms per factorize(), aggregates, host synchronisations.
Times are HIP-event times around factorize() / solve() on device-resident vectors (ipcgpu_bench_factor_solve, ipcgpu_bench_multiply_sym)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipc_amd import lib, scene  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
BJ, LAG, TWO = lib.PRECOND_BLOCK_JACOBI, lib.PRECOND_LAGGED_CHOLESKY, lib.PRECOND_TWO_LEVEL


def twist_ctx(n, solver, iterative=None):
    V, F = scene.make_mat(n)
    left, right = scene.border_verts(V, 0.01)
    c = lib.Context(0, solver=solver)
    if iterative:
        c.set_iterative(*iterative)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.opt_init(dt=0.04, gravity=False)
    c.set_twist(left, right, 0.4 * np.pi)
    c.precompute()
    return c


def contact_ctx(n, solver, iterative=None, layers=2):
    V, F, nA = scene.make_mat_stack(n, layers, gap=1.2e-3)
    Vs = scene.jitter(V, F, rel=2e-3)
    SF = scene.surface_tris(F)
    c = lib.Context(0, solver=solver)
    if iterative:
        c.set_iterative(*iterative)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_positions(Vs)
    c.opt_init(0.01, True)
    c.set_surface(SF)
    border = np.nonzero((np.abs(V[:nA, 0]) > 0.49) | (np.abs(V[:nA, 2]) > 0.49))[0].astype(np.int32)
    c.set_dbc(border, 1)
    c.enable_self_collision(1e-3)
    vel = np.zeros_like(V)
    vel[nA:, 1] = -0.05
    c.set_velocity(vel)
    c.precompute()
    return c


def newton(c, iters):
    """`iters` Newton iterations across as many time steps as they take; returns (iterations done, CG iterations, wall seconds)"""
    done = cg = 0
    t0 = time.perf_counter()
    while done < iters:
        c.begin_timestep()
        for _ in range(iters - done):
            if c.newton_iter():
                break
            done += 1
            cg += c.iter_stats()["iterations"]
        c.end_timestep()
    return done, cg, time.perf_counter() - t0


def per_solve(make, warm_iters, reps):
    """the matrix the stepper holds after `warm_iters` Newton iterations with the exact solver = the one every variant is timed on: each context takes
    the same steps with the exact solver first, then switches"""
    out = {}
    variants = [("multifrontal", 0, None)]
    for tol in (1e-5, 1e-10):
        variants.append((f"pcg_block_jacobi_{tol:g}", 2, (tol, 100000, BJ, 8)))
        variants.append((f"pcg_lagged_cholesky_fresh_{tol:g}", 2, (tol, 1000, LAG, 1)))
    for name, solver, it in variants:
        c = make(0)
        newton(c, warm_iters)
        n_rows, nnz = c.get_dims()
        if solver == 2:
            c.set_solver(2)
            c.set_iterative(*it)
            c.analyze_pattern()
        c.bench_factor_solve(1)
        f_ms, s_ms = c.bench_factor_solve(reps)
        rec = {"factorize_ms": f_ms, "solve_ms": s_ms, "total_ms": f_ms + s_ms, "rows": n_rows, "nnz": nnz}
        if solver == 2:
            rec.update(c.iter_stats())
        else:
            rec["factor_nnzL"] = c.linsys_stats()["nnzL"]
        if name == "multifrontal":
            ms, by = c.bench_multiply_sym(50)
            out["product"] = {"kernel": "k_pcg_symv_blocks", "avg_launch_ms": ms, "algorithmic_bytes": by, "achieved_GBps": by / (ms * 1e-3) / 1e9,
                              "frac_of_hbm_peak": by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        out[name] = rec
        c.close()
        print(name, json.dumps(rec), flush=True)
    return out


def two_level(make, warm_iters, reps):
    """per_solve's protocol for the multifrontal solve, block Jacobi and the two-level preconditioner at 1e-5 and 1e-10"""
    out = {}
    variants = [("multifrontal", 0, None)]
    for tol in (1e-5, 1e-10):
        variants.append((f"pcg_block_jacobi_{tol:g}", 2, (tol, 100000, BJ, 1)))
        variants.append((f"pcg_two_level_{tol:g}", 2, (tol, 100000, TWO, 1)))
    for name, solver, it in variants:
        c = make(0)
        newton(c, warm_iters)
        n_rows, nnz = c.get_dims()
        t_analyze = None
        if solver == 2:
            c.set_solver(2)
            c.set_iterative(*it)
            t0 = time.perf_counter()
            c.analyze_pattern()
            t_analyze = 1e3 * (time.perf_counter() - t0)
        c.bench_factor_solve(1)
        f_ms, s_ms = c.bench_factor_solve(reps)
        rec = {"factorize_ms": f_ms, "solve_ms": s_ms, "total_ms": f_ms + s_ms, "rows": n_rows, "nnz": nnz}
        if solver == 2:
            rec.update(c.iter_stats())
            rec["analyze_pattern_wall_ms"] = t_analyze
            if it[2] == TWO:
                rec.update(c.coarse_stats())
        out[name] = rec
        c.close()
        print(name, json.dumps(rec), flush=True)
    return out


def lagged_ages(n, iters):
    out = {}
    c = twist_ctx(n, 0)
    newton(c, 5)
    d, _, w = newton(c, iters)
    out["multifrontal"] = {"newton_iterations": d, "ms_per_newton_iteration": 1e3 * w / d}
    c.close()
    for age in (1, 2, 4, 8, 16):
        c = twist_ctx(n, 2, (1e-5, 1000, LAG, age))
        newton(c, 5)
        f0 = c.iter_stats()["factorizations"]
        d, cg, w = newton(c, iters)
        out[f"age_{age}"] = {"newton_iterations": d, "ms_per_newton_iteration": 1e3 * w / d, "cg_iterations": cg, "cg_per_newton": cg / d,
                             "factorizations": c.iter_stats()["factorizations"] - f0}
        c.close()
        print("age", age, json.dumps(out[f"age_{age}"]), flush=True)
    best = min((k for k in out if k.startswith("age_")), key=lambda k: out[k]["ms_per_newton_iteration"])
    out["best"] = best
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150)
    ap.add_argument("--contact-n", type=int, default=60)
    ap.add_argument("--newton", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--two-level", action="store_true")
    ap.add_argument("--large-n", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.two_level:
        a.out = a.out or os.path.join("profiles", "pcg_two_level_bench.json")
        rec = {"device": "MI355X", "headline_matrix": {"workload": f"mat{a.n} twist after 10 Newton iterations", **two_level(lambda s: twist_ctx(a.n, s), 10, a.reps)},
               "contact_matrix": {"workload": f"2 x mat{a.contact_n} stack after 8 Newton iterations", **two_level(lambda s: contact_ctx(a.contact_n, s), 8, a.reps)}}
        if a.large_n:
            rec["contact_large_matrix"] = {"workload": f"3 x mat{a.large_n} stack after 2 Newton iterations", **two_level(lambda s: contact_ctx(a.large_n, s, layers=3), 2, a.reps)}
        else:
            rec["contact_large_matrix"] = "not measured"
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        sys.exit(0)
    a.out = a.out or os.path.join("profiles", "pcg_bench.json")
    rec = {"device": "MI355X", "headline_matrix": {"workload": f"mat{a.n} twist after 10 Newton iterations", **per_solve(lambda s: twist_ctx(a.n, s), 10, a.reps)},
           "contact_matrix": {"workload": f"2 x mat{a.contact_n} stack after 8 Newton iterations", **per_solve(lambda s: contact_ctx(a.contact_n, s), 8, a.reps)},
           "lagged_factor_newton_run": {"workload": f"mat{a.n} twist, {a.newton} Newton iterations, rel_tol 1e-5", **lagged_ages(a.n, a.newton)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
