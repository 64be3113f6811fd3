"""Golden of tests/test_gpu_codim_parity.py: one small scene in which every codimensional energy term (shell, strain limit, rod) is live, replayed through
the time stepper, recorded step by step.  It pins that a change to the plumbing around those terms changes no result.

Only the public lib.Context API (and scene.surface_tris) is used, so this file runs unchanged on a checkout of an earlier commit: the golden and its tolerance come from the commit
BEFORE the change under test, never from the code under test.

    python tools/make_codim_parity_golden.py --run OUT.npz             one replay of every case (needs the GPU)
    python tools/make_codim_parity_golden.py --combine R1.npz .. R5.npz  the golden (first run) + the run-to-run spread d per array -> tests/golden/codim_parity.npz
                                                                        and profiles/codim_refactor_parity.json (no GPU)

The scene: a five-tet cube 4 mm over the ground (it falls into the barrier of the half-space within the three steps), a 3 x 3-node cloth stretched by 1.06 between
two held columns with a strain limit 1.1 from onset 1.0 (the barrier is active in every step), a rod of 4 nodes held at one end and bent at rest
positions.  Gravity, lagged damping, dt = 0.01, 3 steps.  Cases: the direct solver, the iterative solver, and -- because damping and a half-space each
switch the stepper's speculative assembly off -- the direct solver once more without ground and damping, which is the only way into that call site.
Once, before precompute builds the pattern: the gradient, which then takes the atomic (tet-parallel) path.  Per step: positions, Newton iterations,
shell_energy, shell_limit_energy, rod_energy, and the CSR values after one assemble_newton(dt^2).  Together the five places where the stepper lets the
terms in: atomic and patch gradient, Newton system, damping matrix (inside it), speculative system (direct_fast)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT, STEPS = 0.01, 3
CASES = {"direct": dict(solver=0, ground=True, damping=True), "iterative": dict(solver=2, ground=True, damping=True),
         "direct_fast": dict(solver=0, ground=False, damping=False)}
FIELDS = ("g_no_pattern", "X", "shell_energy", "shell_limit_energy", "rod_energy", "a")  # compared within a tolerance; "iters" is compared exactly
FACTOR = 8.0  # on the five-run spread: the tail that five samples under-estimate


def five_tet_cube(size, lo):  # (a copy of tests/codim_common.py's on purpose: this file must run on a checkout that has no such module)
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64) * size + lo
    T = np.array([[1, 3, 4, 6], [0, 1, 3, 4], [2, 3, 1, 6], [5, 4, 6, 1], [7, 6, 4, 3]], dtype=np.int32)
    for t in T:  # positive volumes
        if np.linalg.det(P[t[1:]] - P[t[0]]) < 0:
            t[[2, 3]] = t[[3, 2]]
    return P, T


def build_scene():
    P, T = five_tet_cube(0.1, np.array([0.0, 0.004, 0.0]))
    s = 0.05
    Vc = np.array([[0.3 + s * i, 0.3, s * j] for j in range(3) for i in range(3)])
    tri = np.array([q for j in range(2) for i in range(2) for q in ((3 * j + i, 3 * j + i + 1, 3 * j + i + 4), (3 * j + i, 3 * j + i + 4, 3 * j + i + 3))], dtype=np.int32)
    Vr = np.array([[0.6 + s * i, 0.3, 0.0] for i in range(4)])
    seg = np.array([[i, i + 1] for i in range(3)], dtype=np.int32)
    V = np.vstack([P, Vc, Vr])
    tri, seg = tri + len(P), seg + len(P) + len(Vc)
    x = V.copy()
    cloth = np.arange(len(P), len(P) + len(Vc))
    x[cloth, 0] = 0.3 + (V[cloth, 0] - 0.3) * 1.06  # into the barrier's range: onset 1.0 < 1.06 < limit 1.1
    x[cloth[4], 1] += 0.004  # the middle node out of the plane: the hinges carry energy
    rod = np.arange(len(P) + len(Vc), len(V))
    x[rod[2], 1] += 0.004  # bent: both triples carry energy
    x[rod[3], 1] += 0.012
    held = np.concatenate([cloth[0::3], cloth[2::3], rod[:1]]).astype(np.int32)
    return dict(V=V, T=T, tri=tri, seg=seg, x=x, held=held)


def replay(ipc_amd, solver, ground, damping):
    from ipc_amd import scene
    S = build_scene()
    c = ipc_amd.Context(0, solver=solver)
    c.set_mesh(S["V"], S["T"], YM=1e6, PR=0.4, density=1000.0)
    c.set_shell(S["tri"], 1e-3, 1e5, 0.3, 1000.0)
    c.set_shell_strain_limit(1.1, 1.0, 1.0)
    c.set_rod(S["seg"], 2e-3, 1e7, 1000.0)
    c.set_positions(S["x"])
    c.opt_init(DT, True)
    c.set_time_integration("BE")
    c.add_dirichlet(S["held"])
    # before there is a pattern the gradient takes the tet-parallel atomic path: the only way into that call site beside a mesh without tetrahedra
    g_no_pattern = c.gradient(DT * DT, True)
    c.set_surface(np.vstack([scene.surface_tris(S["T"]), S["tri"]]).astype(np.int32), S["seg"])
    if ground:
        c.add_half_space((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1e-3)
    if damping:
        c.set_damping(0.05)
    c.set_rel_tol(1e-6)
    c.precompute()
    out = {k: [] for k in FIELDS[1:] + ("iters",)}
    for _ in range(STEPS):
        it = c.solve_timestep(200)
        assert it < 200
        out["iters"].append(it)
        out["X"].append(c.state()["V"].copy())
        out["shell_energy"].append(c.shell_energy())
        out["shell_limit_energy"].append(c.shell_limit_energy())
        out["rod_energy"].append(c.rod_energy())
        c.assemble_newton(DT * DT, True)
        out["a"].append(c.get_a())
    sigma, ratio = c.shell_stretch()
    c.close()
    res = {k: np.array(v) for k, v in out.items()}
    res["max_stretch"] = np.array(sigma[:, 0].max())
    res["g_no_pattern"] = g_no_pattern
    nP = len(S["V"]) - 13  # the cube's nodes come first; 9 cloth nodes and 4 rod nodes behind them
    assert np.abs(g_no_pattern[3 * nP:3 * (nP + 9)]).max() > 0.0 and np.abs(g_no_pattern[3 * (nP + 9):]).max() > 0.0
    assert np.all(res["shell_limit_energy"] > 0.0) and np.all(res["rod_energy"] > 0.0) and np.all(res["shell_energy"] > res["shell_limit_energy"])  # every term is live
    return res


def replay_all(ipc_amd):
    flat = {}
    for name, kw in CASES.items():
        for k, v in replay(ipc_amd, **kw).items():
            flat[f"{name}_{k}"] = v
    return flat


def rel_dev(a, b):
    """largest element-wise deviation relative to the largest magnitude of the array"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(a).max(), np.abs(b).max())
    return 0.0 if scale == 0.0 else float(np.abs(a - b).max() / scale)


def combine(paths, out_npz, out_json):
    runs = [dict(np.load(p)) for p in paths]
    gold = dict(runs[0])
    report = {"runs": len(runs), "factor": FACTOR, "arrays": {}}
    for name in CASES:
        its = [r[f"{name}_iters"].tolist() for r in runs]
        if any(i != its[0] for i in its):
            raise SystemExit(f"{name}: the Newton counts differ between the runs ({its}): choose a calmer state, do not loosen")
        for k in FIELDS:
            key = f"{name}_{k}"
            pair = [rel_dev(runs[i][key], runs[j][key]) for i in range(len(runs)) for j in range(i + 1, len(runs))]
            gold["d_" + key] = np.array(max(pair))
            gold["spread_" + key] = np.array(pair)
            report["arrays"][key] = {"d": max(pair), "pairwise": pair, "tolerance": FACTOR * max(pair), "scale": float(np.abs(runs[0][key]).max())}
        report["arrays"][f"{name}_iters"] = its[0]
        report["arrays"][f"{name}_max_stretch"] = float(runs[0][f"{name}_max_stretch"])
    np.savez_compressed(out_npz, **gold)
    with open(out_json, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["d"] if isinstance(v, dict) else v) for k, v in report["arrays"].items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", metavar="OUT.npz")
    ap.add_argument("--combine", nargs="+", metavar="RUN.npz")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "codim_parity.npz"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "codim_refactor_parity.json"))
    a = ap.parse_args()
    if a.run:
        import ipc_amd
        ipc_amd.load_library()
        res = replay_all(ipc_amd)
        np.savez_compressed(a.run, **res)
        for name in CASES:
            print(name, "iterations", res[f"{name}_iters"].tolist(), "limit energy", res[f"{name}_shell_limit_energy"].tolist(), "rod energy",
                  res[f"{name}_rod_energy"].tolist(), "largest stretch", float(res[f"{name}_max_stretch"]), "lowest cube node", res[f"{name}_X"][-1][:8, 1].min())
        print("wrote", a.run)
    elif a.combine:
        combine(a.combine, a.out, a.json)
