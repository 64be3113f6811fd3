"""The edges of MfNumeric::factorizeSolve: the data movement that used to be launches of its own (the gather of A into front order, the sign of the
right-hand side, the publication of the pivot flag) now rides in the kernels that produce or consume the data; the un-permutation of x can (MF_BWD_DIRECT_X in
mf_sweeps.hip; measured slower and left off, the checks here hold for either setting).

What could go wrong with that, and what is checked here on two small trees: an entry of x no kernel writes any more (x is pre-filled with NaN), a wrong sign
or permutation (host residual in the SciPy matrix and the difference to SciPy's own solve), a pivot flag that is stale or cleared too late (not-PD and PD
matrices on one context in orders that reuse every slot of the flag with the opposite outcome, published flag against the flag in device memory), run-to-run differences (bits of two calls), and the callers that
do not take the overlapped path (factorize() + solve(), the lagged-Cholesky preconditioner of PCG).

mat12 (864 rows) has single-workgroup fronts only: the flag clear rides in k_front_fused alone and every entry of x comes from k_bwd_level.  mat32 (6144
rows) is the smallest sheet of the scan 12, 20, 24, 28, 30, 32 whose plan has 32-column step launches, blocked triangles AND an explicit-inverse front
(30 still has none of the last); the plan of both is asserted below with the host planner, read the way tests/test_mf_plan.py reads it.
Figures are printed before they are asserted (run with -s to see them).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from ipc_amd import scene

pytestmark = pytest.mark.gpu

RESIDUAL = 1e-10  # the solver tolerance of tools/check_solver.py and tests/test_gpu_schur_tail.py
SIZES = (12, 32)


def _mesh(n):
    V, F = scene.make_mat(n)
    Vt = scene.twist_state(scene.jitter(V, F), 0.5)
    left, right = scene.border_verts(V, 0.01)
    return V, F, Vt, left, right


def _assembled(gpu_lib, n, solver=0):
    """the Newton matrix of the twisted sheet, analysed"""
    V, F, Vt, left, right = _mesh(n)
    c = gpu_lib.Context(0, solver=solver) if solver else gpu_lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.opt_init(0.04, False)
    c.set_dbc(np.concatenate([left, right]), 2)
    c.set_positions(Vt)
    c.set_pattern()
    c.assemble_newton(0.04 ** 2, True, with_gradient=False)
    return c, V


def _host_matrix(c):
    """the full symmetric matrix from the stored upper triangle"""
    ia, ja = c.get_pattern()
    a = c.get_a()
    n = len(ia) - 1
    U = sp.csr_matrix((a, ja, ia), shape=(n, n))
    return (U + sp.triu(U, 1).T).tocsc()


def _factorize_solve(c, b, negate=False, wait=True, fill=np.nan):
    """ipcgpu_linsys_factorize_solve: x pre-filled with `fill`; returns (positive definite?, x, published flag, device flag)"""
    b = np.ascontiguousarray(b, np.float64)
    x = np.full_like(b, fill)
    flags = (C.c_int * 2)(-1, -1)
    dp = C.POINTER(C.c_double)
    rc = c._L.ipcgpu_linsys_factorize_solve(c.h, b.ctypes.data_as(dp), x.ctypes.data_as(dp), C.c_int(int(negate)), C.c_int(int(wait)), flags)
    assert rc in (0, 1), rc  # IPCGPU_OK / IPCGPU_NOT_PD
    return rc == 0, x, flags[0], flags[1]


def _break(c):
    """a negative diagonal entry in the middle of the matrix; returns the values to restore"""
    a0 = c.get_a()
    ia, _ = c.get_pattern()
    k = 3 * ((len(ia) - 1) // 6)
    c.set_coeff(k, k, -abs(a0[ia[k]]))
    return a0


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.fixture(scope="module")
def ctxs(gpu_lib):
    """one analysed context per size, its host matrix and SciPy's own solve of one right-hand side -- computed once, shared, never changed"""
    out = {}
    for n in SIZES:
        c, V = _assembled(gpu_lib, n)
        c.analyze_pattern()
        A = _host_matrix(c)
        b = np.random.default_rng(100 + n).normal(size=A.shape[0])
        xref = spla.splu(A).solve(b)
        out[n] = dict(c=c, V=V, A=A, b=b, xref=xref, res_ref=np.linalg.norm(A @ xref - b) / np.linalg.norm(b))
    yield out
    for d in out.values():
        d["c"].close()


def test_the_two_trees_take_the_paths_they_stand_for(ctxs):
    from solver_plan_helpers import host_plan
    for n in SIZES:
        p = host_plan(ctxs[n]["c"], ctxs[n]["V"])
        tot = {k: sum(L[k][1] for L in p["levels"]) for k in ("small", "bigFronts", "bigTri", "xinvBwd")}
        tot["steps"] = sum(len(L["step"]) for L in p["levels"])
        print(f"mat{n}: {tot}")
        assert tot["small"] > 0 and p["levels"][0]["small"][1] > 1  # the first launch is a fused one with more than one workgroup
        if n == 12:
            assert tot["bigFronts"] == 0 and tot["steps"] == 0 and tot["bigTri"] == 0 and tot["xinvBwd"] == 0
        else:
            assert tot["steps"] > 0 and tot["bigTri"] > 0 and tot["xinvBwd"] > 0


@pytest.mark.parametrize("n", SIZES)
def test_every_entry_of_x_is_written_and_solves_the_system(ctxs, n):
    d = ctxs[n]
    ok, x, pub, dev = _factorize_solve(d["c"], d["b"])
    assert ok and pub == 0 and dev == 0
    assert np.isfinite(x).all(), f"{np.count_nonzero(~np.isfinite(x))} entries of x were not written"
    nb = np.linalg.norm(d["b"])
    res = np.linalg.norm(d["A"] @ x - d["b"]) / nb
    gap = np.linalg.norm(d["A"] @ (x - d["xref"])) / nb  # = |r_gpu - r_ref| / |b|
    print(f"mat{n}: residual {res:.2e}, SciPy's own {d['res_ref']:.2e}, |A (x - x_scipy)| / |b| {gap:.2e}")
    assert res <= RESIDUAL
    assert gap <= RESIDUAL + d["res_ref"]
    # the sign taken inside the solver's permutation pass: exact, so -x bit for bit (and again every entry written)
    ok, xn, pub, dev = _factorize_solve(d["c"], d["b"], negate=True)
    assert ok and pub == dev == 0 and np.array_equal(_bits(xn), _bits(-x))


@pytest.mark.parametrize("n", SIZES)
def test_the_stepper_gets_minus_the_newton_direction(gpu_lib, n):
    """p = -H^-1 g through HipOptimizer::computeSearchDir, which no longer forms -g on the multifrontal path"""
    V, F, _, left, right = _mesh(n)
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
    c.opt_init(0.04, False)
    c.set_twist(left, right, 0.4 * np.pi)
    c.precompute()
    c.begin_timestep()
    assert not c.newton_iter()  # (the first pass of a time step that moves the handles does not converge)
    st = c.state()  # the gradient and the matrix the pass solved with stay until the next pass swaps its own in
    A = _host_matrix(c)
    p, g = st["searchDir"], st["gradient"]
    c.close()
    assert np.isfinite(p).all() and np.linalg.norm(g) > 0
    res = np.linalg.norm(A @ p + g) / np.linalg.norm(g)
    print(f"mat{n}: |H p + g| / |g| = {res:.2e}, p.g = {p @ g:.3e}")
    assert res <= RESIDUAL
    assert p @ g < 0  # a descent direction


# The pivot flag has two slots that consecutive factorisations take in turn, each clearing the other's for its successor.  In these sequences call k and call
# k + 2 (the same slot) differ in outcome for every k, whichever slot the first call meets: a PD call finds the slot a not-PD one set two calls before (a
# missing, misplaced or late clear fails it), a not-PD call finds a slot a PD one left clear, and with a single slot the same is met where consecutive calls differ
# (the first, third and fifth pair).  Nothing depends on how many factorisations the shared context has behind it.
FLAG_SEQUENCES = {"bad_first": (True, False, False, True, True, False), "good_first": (False, True, True, False, False, True)}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order", sorted(FLAG_SEQUENCES))
@pytest.mark.parametrize("wait", [True, False])
def test_flag_life_cycle(ctxs, n, order, wait):
    """not-PD and PD matrices on one context, every slot of the flag reused with the opposite outcome; ok, published and device flag asserted on every call"""
    d = ctxs[n]
    c = d["c"]
    a0 = c.get_a()
    seq = FLAG_SEQUENCES[order]
    assert all(seq[k] != seq[k + 2] for k in range(len(seq) - 2))
    try:
        for bad in seq:
            if bad:
                _break(c)
            else:
                c.set_a(a0)
            ok, x, pub, dev = _factorize_solve(c, d["b"], wait=wait)
            print(f"mat{n} wait={wait} bad={bad}: ok={ok} published={pub} device={dev}")
            assert ok == (not bad)
            assert pub == dev == (1 if bad else 0)  # what reached the host is what the device holds
            if not bad:
                assert np.linalg.norm(d["A"] @ x - d["b"]) / np.linalg.norm(d["b"]) <= RESIDUAL
    finally:
        c.set_a(a0)


@pytest.mark.parametrize("n", SIZES)
def test_two_calls_give_the_same_bits(ctxs, n):
    d = ctxs[n]
    ok, x1, pub, dev = _factorize_solve(d["c"], d["b"])
    assert ok and pub == dev == 0
    ok, x2, pub, dev = _factorize_solve(d["c"], d["b"], wait=False)
    assert ok and pub == dev == 0
    assert np.array_equal(_bits(x1), _bits(x2))


def test_factorize_then_solve_as_two_calls(ctxs):
    d = ctxs[12]
    c = d["c"]
    assert c.factorize()
    x = c.solve(d["b"])  # (node order: the residual is taken in the caller's numbering)
    res = np.linalg.norm(d["A"] @ x - d["b"]) / np.linalg.norm(d["b"])
    print(f"factorize() + solve(): residual {res:.2e}")
    assert res <= RESIDUAL
    ok, x2, pub, dev = _factorize_solve(c, d["b"])
    assert ok and pub == dev == 0
    assert np.array_equal(_bits(x), _bits(x2))  # the overlapped call runs the same kernels on the same data
    a0 = _break(c)
    try:
        assert not c.factorize()
        c.set_a(a0)
        assert c.factorize()
    finally:
        c.set_a(a0)


def test_pcg_with_the_lagged_factor(gpu_lib):
    """MfNumeric::solve as the preconditioner of the iterative solver (tests/test_gpu_pcg.py's contract: 1e-10 asked, 2e-10 on the host)"""
    c, _ = _assembled(gpu_lib, 12, solver=2)
    A = _host_matrix(c)
    n = A.shape[0]
    c.set_iterative(1e-10, n, 1, 8)
    c.analyze_pattern()
    assert c.factorize()
    b = np.random.default_rng(7).normal(size=n)
    x = c.solve(b)
    st = c.iter_stats()
    c.close()
    res = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    print(f"PCG, lagged factor: residual {res:.2e}, {st}")
    assert np.isfinite(x).all() and res <= 2e-10
    assert st["converged"] == 1 and st["iterations"] <= 3  # the exact factor of the same matrix: a wrong permutation of z would take many
