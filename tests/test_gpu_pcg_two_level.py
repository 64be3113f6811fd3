"""Preconditioner 2 of solver type 2 (IPCGPU_PRECOND_TWO_LEVEL): block Jacobi plus an exact coarse solve on six rigid-body modes per node aggregate.
The host side of every check is the numpy model tests/pcg_two_level_numpy.py fed with the library's own aggregates (ipcgpu_linsys_coarse_get) and the
oracle's symv.  Shapes: tests/pcg_two_level_cases.py.  Measured figures are printed before they are asserted (run with -s to see them)."""
import numpy as np
import pytest

from ipc_amd.lib import IpcGpuError, NotPositiveDefinite

import pcg_numpy
import pcg_two_level_cases as cases
import pcg_two_level_numpy as model
from test_gpu_pcg import make_ctx, twisted_bar_run

pytestmark = pytest.mark.gpu

BJ, TWO = 0, 2


@pytest.fixture(scope="module")
def shapes(orc):
    return dict(bar=cases.make(orc, "bar"), sheet=cases.make(orc, "sheet"))


def assembled(gpu_lib, s, rel_tol=1e-10, precond=TWO):
    c = make_ctx(gpu_lib, s["V"], s["F"], s["Vt"], s["dbc"])
    c.set_pattern()
    c.assemble_newton(cases.DTSQ, True, with_gradient=False)
    c.set_iterative(rel_tol, len(s["ia"]) - 1, precond, 1)
    c.analyze_pattern()
    return c


def dense_from_upper(cia, cja, ca):
    n = len(cia) - 1
    r, c, v = pcg_numpy.upper_csr_to_full(cia, cja, ca)
    A = np.zeros((n, n))
    np.add.at(A, (r, c), v)
    return A


def test_kind_2_is_accepted(gpu_lib):
    c = gpu_lib.Context(0, solver=2)
    c.set_iterative(1e-5, 1000, TWO, 1)
    with pytest.raises(IpcGpuError, match="ipcgpu error -1"):
        c.set_iterative(1e-5, 1000, 3, 1)
    c.close()


@pytest.mark.parametrize("name", ["bar", "sheet"])
def test_coarse_matrix(shapes, gpu_lib, name):
    s = shapes[name]
    c = assembled(gpu_lib, s)
    assert c.factorize()
    agg, cia, cja, ca = c.coarse_get()
    st = c.coarse_stats()
    print(name, st)
    assert st["aggregates"] == agg.max() + 1 and st["coarse_rows"] == 6 * st["aggregates"] == len(cia) - 1 and st["coarse_nnz"] == len(cja)
    assert st["coarse_factorizations"] == 1 and st["jacobi_fallbacks"] == 0
    ia, ja = c.get_pattern()
    assert np.array_equal(ia, s["ia"]) and np.array_equal(ja, s["ja"])
    ref = model.galerkin(ia, ja, c.get_a(), agg, s["Vt"], s["fixed"])
    err = np.abs(dense_from_upper(cia, cja, ca) - ref).max() / np.abs(ref).max()
    print(name, "coarse matrix against numpy's P^T A P:", err)
    assert err <= 1e-12
    c.close()


@pytest.mark.parametrize("name", ["bar", "sheet"])
def test_residual_contract(shapes, gpu_lib, name):
    s = shapes[name]
    c = assembled(gpu_lib, s, 1e-10)
    assert c.factorize()
    a, b = c.get_a(), cases.rhs(s)
    x = c.solve(b)
    st = c.iter_stats()
    res = np.linalg.norm(s["m"].symv(a, x) - b) / np.linalg.norm(b)
    print(name, "host residual", res, st, c.coarse_stats())
    assert res <= 2e-10
    assert st["converged"] == 1
    c.close()


def test_the_coarse_space_is_applied(shapes, gpu_lib):
    s = shapes["sheet"]
    c = assembled(gpu_lib, s, 1e-5)
    assert c.factorize()
    a, b = c.get_a(), cases.rhs(s)
    agg = c.coarse_get(values=False)[0]
    n = len(b)
    _, n_bj = model.cg(s["ia"], s["ja"], a, b, 1e-5, n)
    _, n_tl = model.cg(s["ia"], s["ja"], a, b, 1e-5, n, agg, s["Vt"], s["fixed"])
    x = c.solve(b)
    st = c.iter_stats()
    print("sheet at 1e-5: model block Jacobi", n_bj, "model two-level", n_tl, "gpu", st, c.coarse_stats())
    assert st["converged"] == 1
    assert st["iterations"] <= n_tl + max(2, 0.1 * n_tl)
    assert st["iterations"] <= np.sqrt(n_bj * n_tl)
    assert np.linalg.norm(s["m"].symv(a, x) - b) <= 2e-5 * np.linalg.norm(b)
    # two solves of the same system: the same bits
    x1 = c.solve(b)
    assert c.iter_stats()["iterations"] == st["iterations"] and st["iterations"] > 1
    assert np.array_equal(x, x1)
    c.close()


def test_reproducible_across_factorizations(shapes, gpu_lib):
    s = shapes["bar"]
    b = cases.rhs(s)
    out = []
    for _ in range(2):
        c = assembled(gpu_lib, s, 1e-10)
        assert c.factorize()
        out.append((c.solve(b), c.coarse_get()[3], c.iter_stats()["iterations"]))
        c.close()
    assert out[0][2] == out[1][2] > 1
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])


def test_pattern_change(shapes, gpu_lib):
    s = shapes["bar"]
    c = assembled(gpu_lib, s, 1e-10)
    assert c.factorize()
    b = cases.rhs(s)
    a = c.get_a()
    x = c.solve(b)
    assert np.linalg.norm(s["m"].symv(a, x) - b) <= 2e-10 * np.linalg.norm(b) and c.iter_stats()["converged"] == 1
    dims0 = c.coarse_dims()
    # a grown pattern: four extra node pairs (one given in descending order), their blocks filled with small values
    nV = s["V"].shape[0]
    extra = np.array([[0, nV - 1], [5, 200], [230, 40], [17, 150]], dtype=np.int32)
    c.set_pattern(extra)
    c.assemble_newton(cases.DTSQ, True, with_gradient=False)
    ia, ja = c.get_pattern()
    a2 = c.get_a()
    rng = np.random.default_rng(5)
    scale = 1e-3 * np.abs(a2[ia[:-1]]).min()
    for u, w in np.sort(extra, axis=1):
        for r in range(3):
            k = ia[3 * u + r] + np.searchsorted(ja[ia[3 * u + r]:ia[3 * u + r + 1]], 3 * w)
            assert ja[k] == 3 * w
            a2[k:k + 3] = scale * rng.normal(size=3)
    c.set_a(a2)
    assert c.coarse_dims() == (0, 0, 0)  # the analysis of the old pattern is gone
    c.analyze_pattern()
    assert c.factorize()
    dims1 = c.coarse_dims()
    print("coarse dims", dims0, "->", dims1)
    assert dims1 != dims0 and dims1[0] > 0
    agg, cia, cja, ca = c.coarse_get()
    ref = model.galerkin(ia, ja, a2, agg, s["Vt"], s["fixed"])
    err = np.abs(dense_from_upper(cia, cja, ca) - ref).max() / np.abs(ref).max()
    print("coarse matrix of the grown pattern against numpy's P^T A P:", err)
    assert err <= 1e-12
    x = c.solve(b)
    res = np.linalg.norm(pcg_numpy.symv(ia, ja, a2, x) - b) / np.linalg.norm(b)
    print("grown pattern: host residual", res, c.iter_stats())
    assert res <= 2e-10 and c.iter_stats()["converged"] == 1
    c.close()


def test_not_positive_definite(shapes, gpu_lib):
    s = shapes["bar"]
    ia = s["ia"]
    # a negated diagonal block entry: factorize says so
    c = assembled(gpu_lib, s, 1e-10)
    assert c.factorize()
    a = c.get_a()
    c.set_coeff(3 * 40, 3 * 40, -abs(a[ia[3 * 40]]))
    assert not c.factorize()
    # every diagonal block positive definite, the matrix indefinite (the blocks off the diagonal scaled up): factorize succeeds, solve meets p.Ap <= 0
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    off = rows // 3 != s["ja"] // 3
    a2 = a.copy()
    a2[off] *= 50.0
    assert np.linalg.eigvalsh(dense_from_upper(ia, s["ja"], a2)).min() < 0
    c.set_a(a2)
    assert c.factorize()
    print("indefinite matrix with definite blocks:", c.coarse_stats())
    with pytest.raises(NotPositiveDefinite):
        c.solve(cases.rhs(s))
    c.close()


def test_unsupported(gpu_lib):
    # a set_pattern_csr pattern has no nodes
    ja, ptr = [], [0]
    for v in range(10):
        for r in range(3):
            ja += [3 * v + k for k in range(r, 3)]
            ptr.append(len(ja))
    c = gpu_lib.Context(0, solver=2)
    c.set_pattern_csr(np.array(ptr, dtype=np.int32), np.array(ja, dtype=np.int32))
    c.set_iterative(1e-5, 1000, TWO, 1)
    with pytest.raises(IpcGpuError, match="ipcgpu error -4"):
        c.analyze_pattern()
    c.close()
    c = gpu_lib.Context(0, solver=2)
    c.set_iterative(1e-5, 1000, TWO, 1)
    with pytest.raises(IpcGpuError, match="ipcgpu error -4"):
        c.set_solver_shard(0, 2)
    c.close()


def test_through_the_stepper(gpu_lib):
    """the bar twist of tests/test_gpu_pcg.py, three time steps: the same Newton counts as the multifrontal solver, positions within that file's bound"""
    r0, diag = twisted_bar_run(gpu_lib, 0)
    r1, _ = twisted_bar_run(gpu_lib, 1)
    r2, _ = twisted_bar_run(gpu_lib, 2, (1e-10, 1000, TWO, 1))
    d01 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r1))
    d02 = max(np.abs(a["V"] - b["V"]).max() for a, b in zip(r0, r2))
    bound = 10 * max(d01, 1e-12 * diag)
    print(f"twisted bar, 3 steps: Newton counts solver 0 {[s['n'] for s in r0]}, two-level {[s['n'] for s in r2]}, d01 = {d01:.3e}, max|x_0 - x_2| = {d02:.3e}, bound = {bound:.3e}")
    assert [s["n"] for s in r2] == [s["n"] for s in r0]
    assert d02 <= bound
