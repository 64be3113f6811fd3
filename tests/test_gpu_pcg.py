"""Solver type 2: preconditioned conjugate gradients behind the reference's `linearSolver AMGCL` (ipcgpu_linsys_set_iterative).

The matrices are those of tests/test_gpu_parity.py's twisted bar unless said otherwise; the host side of every check is the oracle's
symv or the plain numpy CG of tests/pcg_numpy.py.  Measured figures are printed before they are asserted (run with -s to see them).
"""
import os

import numpy as np
import pytest

from ipc_amd import scene
from ipc_amd.lib import IpcGpuError, NotPositiveDefinite

import pcg_numpy

pytestmark = pytest.mark.gpu

BJ, LAG = 0, 1
DTSQ = 0.025 ** 2


def make_ctx(gpu_lib, V, F, Vcur, dbc, solver=2):
    c = gpu_lib.Context(0, solver=solver)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(0.025, False)
    c.set_dbc(dbc, 2)
    c.set_positions(Vcur)
    return c


@pytest.fixture(scope="module")
def bar(orc):
    # the `bar` of tests/test_gpu_parity.py:36-43
    V, F = scene.make_bar(16, 3, 3, size=(6.0, 0.75, 1.0))
    Vt = scene.twist_state(scene.jitter(V, F), 0.25)
    left, right = scene.border_verts(V, 0.01)
    dbc = np.concatenate([left, right])
    m = orc.Mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    m.set_dbc(dbc, 2)
    m.set_V(Vt)
    ia, ja = m.pattern()
    return dict(V=V, F=F, Vt=Vt, m=m, dbc=dbc, ia=ia, ja=ja)


def assembled(gpu_lib, bar, Vcur=None):
    c = make_ctx(gpu_lib, bar["V"], bar["F"], bar["Vt"] if Vcur is None else Vcur, bar["dbc"])
    c.set_pattern()
    c.assemble_newton(DTSQ, True, with_gradient=False)
    return c


def rhs(bar, seed=14):
    return np.random.default_rng(seed).normal(size=len(bar["ia"]) - 1)


@pytest.mark.parametrize("precond", [BJ, LAG])
def test_residual_contract(bar, gpu_lib, precond):
    c = assembled(gpu_lib, bar)
    n = len(bar["ia"]) - 1
    c.set_iterative(1e-10, n, precond, 8)
    c.analyze_pattern()
    assert c.factorize()
    a, b = c.get_a(), rhs(bar)
    x = c.solve(b)
    st = c.iter_stats()
    res = np.linalg.norm(bar["m"].symv(a, x) - b) / np.linalg.norm(b)
    print("precond", precond, "host residual", res, st)
    assert res <= 2e-10
    assert st["converged"] == 1 and st["residual"] <= 1e-10
    c.close()


def graded(V, p=2.0):
    """node spacing growing along every axis: elements of very different sizes, hence diagonal blocks of very different magnitude"""
    V = V.copy()
    for ax in range(3):
        lo, hi = V[:, ax].min(), V[:, ax].max()
        V[:, ax] = lo + (hi - lo) * ((V[:, ax] - lo) / (hi - lo)) ** p
    return V


def test_the_preconditioner_is_applied(orc, gpu_lib):
    """On the uniform bar the numpy pair gives n_none = 78, n_bj = 43 at 1e-10 (ratio 1.8 < 2; stiffer -- YM 1e7, 1e9 -- and uniformly finer -- 24 x 4 x 4 --
    bars stay at 1.5), so the mesh is the same bar with its node spacing graded quadratically along each axis: n_none = 176, n_bj = 61 with the oracle's
    assemble_hessian on the CPU."""
    V, F = scene.make_bar(16, 3, 3, size=(6.0, 0.75, 1.0))
    V = graded(V)
    Vt = scene.twist_state(scene.jitter(V, F), 0.25)
    left, right = scene.border_verts(V, 0.01)
    dbc = np.concatenate([left, right])
    m = orc.Mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    m.set_dbc(dbc, 2)
    m.set_V(Vt)
    ia, ja = m.pattern()
    a = m.assemble_hessian(len(ja), DTSQ, projectDBC=True)
    n = len(ia) - 1
    b = np.random.default_rng(14).normal(size=n)
    _, n_none = pcg_numpy.cg(ia, ja, a, b, 1e-10, n)
    _, n_bj = pcg_numpy.cg(ia, ja, a, b, 1e-10, n, block_jacobi=True)
    c = make_ctx(gpu_lib, V, F, Vt, dbc)
    c.set_pattern()
    c.assemble_newton(DTSQ, True, with_gradient=False)
    c.set_iterative(1e-10, n, BJ, 8)
    c.analyze_pattern()
    assert c.factorize()
    x = c.solve(b)
    n_gpu = c.iter_stats()["iterations"]
    print("n_none", n_none, "n_bj", n_bj, "gpu block Jacobi", n_gpu)
    assert n_none >= 2 * n_bj
    assert n_gpu <= np.sqrt(n_none * n_bj)
    assert np.linalg.norm(m.symv(c.get_a(), x) - b) <= 2e-10 * np.linalg.norm(b)
    c.close()


def test_fresh_factor_is_a_direct_solve(bar, gpu_lib):
    c = assembled(gpu_lib, bar)
    c.set_iterative(1e-8, 1000, LAG, 1)
    c.analyze_pattern()
    assert c.factorize()
    b = rhs(bar)
    x = c.solve(b)
    st = c.iter_stats()
    print(st)
    assert st["iterations"] == 1 and st["factorizations"] == 1 and st["converged"] == 1 and st["factor_age"] == 0
    assert np.linalg.norm(bar["m"].symv(c.get_a(), x) - b) <= 2e-8 * np.linalg.norm(b)
    c.close()


def test_stale_factor(bar, gpu_lib):
    c = assembled(gpu_lib, bar)
    n = len(bar["ia"]) - 1
    c.set_iterative(1e-10, n, LAG, 8)
    c.analyze_pattern()
    assert c.factorize()
    V2 = scene.twist_state(scene.jitter(bar["V"], bar["F"]), 0.27)
    c.set_positions(V2)
    c.assemble_newton(DTSQ, True, with_gradient=False)
    assert c.factorize()  # keeps the factor of the 0.25 state
    a, b = c.get_a(), rhs(bar)
    x = c.solve(b)
    st = c.iter_stats()
    res = np.linalg.norm(bar["m"].symv(a, x) - b) / np.linalg.norm(b)
    print("stale factor:", st, "host residual", res)
    assert res <= 2e-10 and st["converged"] == 1 and st["residual"] <= 1e-10
    assert st["factorizations"] == 1 and st["factor_age"] == 1 and st["iterations"] > 1
    # one iteration is not enough with the stale factor: the solve refactorises by itself, once
    c.set_iterative(1e-8, 1, LAG, 8)
    x = c.solve(b)
    st = c.iter_stats()
    print("after the refactorisation inside solve:", st)
    assert st["factorizations"] == 2 and st["converged"] == 1 and st["factor_age"] == 0
    assert np.linalg.norm(bar["m"].symv(a, x) - b) <= 2e-8 * np.linalg.norm(b)
    c.close()


def test_product(bar, orc, gpu_lib):
    m = bar["m"]
    c = assembled(gpu_lib, bar)
    x = np.random.default_rng(12).normal(size=len(bar["ia"]) - 1)

    def check(ctx, a, ia, ja):
        y0, y1 = ctx.multiply_sym(x[:len(ia) - 1]), ctx.multiply_sym(x[:len(ia) - 1])
        ref = pcg_numpy.symv(ia, ja, a, x[:len(ia) - 1])
        err = np.abs(y0 - ref).max() / np.abs(ref).max()
        print("product error", err)
        assert err < 1e-12
        assert np.array_equal(y0, y1)
        return y0

    a = c.get_a()
    y = check(c, a, bar["ia"], bar["ja"])
    assert np.abs(y - m.symv(a, x)).max() / np.abs(y).max() < 1e-12  # the oracle's product, as tests/test_gpu_parity.py:111
    # the pattern with the four extra pairs of tests/test_gpu_parity.py:76, every entry filled
    extra = np.array([[0, bar["V"].shape[0] - 1], [5, 200], [200, 5], [17, 18]], dtype=np.int32)
    c.set_pattern(extra)
    ia, ja = c.get_pattern()
    a2 = np.random.default_rng(3).normal(size=len(ja))
    c.set_a(a2)
    check(c, a2, ia, ja)
    c.close()
    # a set_pattern_csr pattern: scalar rows of uneven length
    rng = np.random.default_rng(4)
    n = 30
    rows = [[r] + sorted(rng.choice(np.arange(r + 1, n), size=min(n - 1 - r, int(rng.integers(0, 6))), replace=False).tolist()) for r in range(n)]
    ia = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ja = np.concatenate(rows).astype(np.int32)
    c = gpu_lib.Context(0, solver=2)
    c.set_pattern_csr(ia, ja)
    a3 = rng.normal(size=len(ja))
    c.set_a(a3)
    check(c, a3, ia, ja)
    c.close()


@pytest.mark.parametrize("precond", [BJ, LAG])
def test_determinism(bar, gpu_lib, precond):
    c = assembled(gpu_lib, bar)
    c.set_iterative(1e-10, len(bar["ia"]) - 1, precond, 8)
    c.analyze_pattern()
    assert c.factorize()
    if precond == LAG:  # a stale factor, so that there is more than one iteration to repeat
        c.set_positions(scene.twist_state(scene.jitter(bar["V"], bar["F"]), 0.27))
        c.assemble_newton(DTSQ, True, with_gradient=False)
        assert c.factorize()
    b = rhs(bar)
    x0, n0 = c.solve(b), c.iter_stats()["iterations"]
    x1, n1 = c.solve(b), c.iter_stats()["iterations"]
    assert n0 == n1 and n0 > 1
    assert np.array_equal(x0, x1)
    c.close()


@pytest.mark.parametrize("precond,age", [(BJ, 8), (LAG, 1)])
def test_negative_diagonal_fails_factorize(bar, gpu_lib, precond, age):
    c = assembled(gpu_lib, bar)
    c.set_iterative(1e-10, 1000, precond, age)
    c.analyze_pattern()
    assert c.factorize()
    a, ia = c.get_a(), bar["ia"]
    k = ia[3 * 40]
    c.set_coeff(3 * 40, 3 * 40, -abs(a[k]))
    assert not c.factorize()
    b = rhs(bar)
    a2 = c.get_a()
    assert np.allclose(c.precondition_diag(b), b / a2[ia[:-1]], rtol=1e-15)
    c.close()


def test_indefinite_with_definite_blocks_breaks_down_in_solve(gpu_lib):
    # [[I, 2 I], [2 I, I]]: the diagonal blocks are identities, A b = -b for b = (1, 1, 1, -1, -1, -1)
    rows = [[0, 3], [1, 4], [2, 5], [3], [4], [5]]
    ia = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ja = np.concatenate(rows).astype(np.int32)
    a = np.array([1, 2, 1, 2, 1, 2, 1, 1, 1], dtype=float)
    c = gpu_lib.Context(0, solver=2)
    c.set_pattern_csr(ia, ja)
    c.set_a(a)
    c.analyze_pattern()
    assert c.factorize()
    b = np.array([1, 1, 1, -1, -1, -1], dtype=float)
    with pytest.raises(NotPositiveDefinite):
        c.solve(b)
    assert np.array_equal(c.precondition_diag(b), b)
    c.close()


def test_known_answer(gpu_lib):
    # Diagnostic.cpp:367-392 as in tests/test_gpu_parity.py: 10 isolated nodes, diagonal 10, rhs 1 => x = 0.1
    ja, ptr = [], [0]
    for v in range(10):
        for r in range(3):
            ja += [3 * v + k for k in range(r, 3)]
            ptr.append(len(ja))
    ia, ja = np.array(ptr, dtype=np.int32), np.array(ja, dtype=np.int32)
    c = gpu_lib.Context(0, solver=2)
    c.set_pattern_csr(ia, ja)
    c.set_zero()
    for r in range(30):
        c.add_coeff(r, r, 10.0)
    c.analyze_pattern()
    assert c.factorize()
    assert np.allclose(c.solve(np.ones(30)), 0.1, rtol=0, atol=1e-15)
    assert c.iter_stats()["iterations"] == 1
    c.close()


# ---- Newton loops ----------------------------------------------------------------------------------------------------------------------
def twisted_bar_run(gpu_lib, solver, iterative=None, steps=3):
    """the GPU side of tests/test_gpu_parity.py:186-201; returns per step (Newton count, positions, energies of the iterates)"""
    V, F = scene.make_bar(12, 2, 2, size=(5.0, 0.5, 1.0))
    left, right = scene.border_verts(V, 0.01)
    Vs = scene.twist_state(scene.jitter(V, F, rel=2e-2), 0.15)
    c = gpu_lib.Context(0, solver=solver)
    if iterative:
        c.set_iterative(*iterative)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.set_positions(Vs)
    c.opt_init(0.025, False)
    c.set_twist(left, right)
    c.precompute()
    out = run_steps(c, steps, 100)
    c.close()
    return out, float(np.linalg.norm(V.max(0) - V.min(0)))


def run_steps(c, steps, max_iter):
    out = []
    for _ in range(steps):
        c.begin_timestep()
        energies, n, converged = [], 0, False
        for _ in range(max_iter):
            if c.newton_iter():
                converged = True
                break
            n += 1
            s = c.state()
            energies.append((s["E"], s["kappa"], s["dHat"]))
        c.end_timestep()
        out.append(dict(n=n, converged=converged, V=c.state()["V"].copy(), E=energies))
    return out


def mat_stack_run(gpu_lib, solver, iterative=None, steps=8):
    """the contact bench's construction (tools/bench_contact.py) in small, the upper sheet starting outside the barrier's reach: touch-down inside the run"""
    V, F, nA = scene.make_mat_stack(14, 2, gap=2.5e-3)
    Vs = scene.jitter(V, F, rel=2e-3)
    SF = scene.surface_tris(F)
    border = np.nonzero((np.abs(V[:nA, 0]) > 0.49) | (np.abs(V[:nA, 2]) > 0.49))[0].astype(np.int32)
    c = gpu_lib.Context(0, solver=solver)
    if iterative:
        c.set_iterative(*iterative)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.set_positions(Vs)
    c.opt_init(0.01, True)
    c.set_surface(SF)
    c.set_dbc(border, 1)
    c.enable_self_collision(1e-3)
    vel = np.zeros_like(V)
    vel[nA:, 1] = -0.05
    c.set_velocity(vel)
    c.precompute()
    active0 = c.contact_state()["nActive"]
    out = run_steps(c, steps, 60)
    info = dict(active0=active0, contact=c.contact_state(), intersected=c.is_intersected(), stats=c.iter_stats(), nnzL=c.linsys_stats()["nnzL"])
    c.close()
    return out, info, float(np.linalg.norm(V.max(0) - V.min(0)))


def record(line):
    print(line)
    path = os.environ.get("IPCGPU_PCG_PARITY_FILE")  # tools/ and the committed profiles/pcg_parity.txt: the printed figures, appended
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_newton_loop_contact_free(gpu_lib):
    r0, diag = twisted_bar_run(gpu_lib, 0)
    r1, _ = twisted_bar_run(gpu_lib, 1)
    d01 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r1))
    bound = 10 * max(d01, 1e-12 * diag)
    record(f"twisted bar, 3 steps: Newton counts solver 0 {[s['n'] for s in r0]}, d01 = {d01:.3e}, bound = {bound:.3e}")
    for name, precond in (("block Jacobi", BJ), ("lagged Cholesky", LAG)):
        r2, _ = twisted_bar_run(gpu_lib, 2, (1e-10, 1000, precond, 8))
        d02 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r2))
        record(f"  solver 2 {name}: Newton counts {[s['n'] for s in r2]}, max|x_0 - x_2| = {d02:.3e}")
        assert [s["n"] for s in r2] == [s["n"] for s in r0]
        assert d02 <= bound


def test_newton_loop_with_contact_block_jacobi(gpu_lib):
    r0, i0, diag = mat_stack_run(gpu_lib, 0)
    r1, i1, _ = mat_stack_run(gpu_lib, 1)
    r2, i2, _ = mat_stack_run(gpu_lib, 2, (1e-10, 1000, BJ, 8))
    d01 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r1))
    d02 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r2))
    bound = 10 * max(d01, 1e-12 * diag)
    record(f"2 x mat14 stack, 8 steps: Newton counts solver 0 {[s['n'] for s in r0]}, solver 2 block Jacobi {[s['n'] for s in r2]}, d01 = {d01:.3e}, "
           f"max|x_0 - x_2| = {d02:.3e}, bound = {bound:.3e}; active pairs {i2['active0']} -> {i2['contact']['nActive']}, pattern changes {i2['contact']['nPatternChanges']}")
    assert i2["active0"] == 0 and i2["contact"]["nActive"] > 0 and i2["contact"]["nPatternChanges"] > 0  # touch-down happened inside the run
    assert [s["n"] for s in r2] == [s["n"] for s in r0]
    assert d02 <= bound
    assert not i2["intersected"]
    assert i2["stats"]["factorizations"] == 0 and i2["nnzL"] == 0  # neither a numeric nor a symbolic factorisation ever happened


def energy_non_increasing(run):
    """over the accepted steps of a time step, while the barrier's stiffness and reach stay what they were (a change of either changes the function)"""
    for s in run:
        for (e0, k0, h0), (e1, k1, h1) in zip(s["E"], s["E"][1:]):
            if (k0, h0) == (k1, h1) and e1 > e0 + 1e-12 * abs(e0):
                return False
    return True


def test_reference_defaults(gpu_lib):
    for name, precond in (("block Jacobi", BJ), ("lagged Cholesky", LAG)):
        r0, _ = twisted_bar_run(gpu_lib, 0)
        r2, _ = twisted_bar_run(gpu_lib, 2, (1e-5, 1000, precond, 8))
        print(f"twisted bar, {name} at 1e-5: Newton counts {[s['n'] for s in r2]} (solver 0: {[s['n'] for s in r0]})")
        assert all(s["converged"] for s in r2)
        assert energy_non_increasing(r2)
        s0, i0, _ = mat_stack_run(gpu_lib, 0)
        s2, i2, _ = mat_stack_run(gpu_lib, 2, (1e-5, 1000, precond, 8))
        print(f"mat stack, {name} at 1e-5: Newton counts {[s['n'] for s in s2]} (solver 0: {[s['n'] for s in s0]}), solver 0 energies monotone: {energy_non_increasing(s0)}")
        assert all(s["converged"] for s in s2)
        assert not i2["intersected"]
        assert energy_non_increasing(s2)


def test_sharding_is_unsupported(gpu_lib):
    c = gpu_lib.Context(0)
    c.set_solver(2)
    with pytest.raises(IpcGpuError, match="ipcgpu error -4"):
        c.set_solver_shard(0, 2)
    c.close()
