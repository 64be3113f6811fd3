"""k_extend_add and k_big_schur64_ea (ipc_amd/csrc/mf_numeric.hip) read the children of a tile from the host plan's row maps and tile records
(tests/test_mf_child_maps.py checks those on the host).  Through the solver's C API, on three matrices:

  * `stack`: two mat13 sheets with the contact pairs of `test_mf_symbolic.stacked_pattern(13)` -- the pattern the host test reads.  With the default tuning no
    level has 512 Schur tiles, so EVERY level of batched fronts goes through k_extend_add with ownOnly = 0 (the whole lower triangle of each front gathered
    there) and k_big_schur;
  * `mat40`: one twisted sheet, the level structure of the benchmark at 1/14 of its size.  Its levels stay below 512 Schur tiles as well (the planner says so
    below), so it is a second, larger matrix on the path of `stack`;
  * `mat60`: the smallest sheet of the suite whose middle levels reach 512 Schur tiles (tests/test_gpu_schur_tail.py): three levels take k_extend_add with
    ownOnly = 1 and k_big_schur64_ea, the top levels the path of `stack`.

Which levels take which path is asserted from the host planner on the solver's own pattern.  (fusedLds and schur64Min are not settable through the C API --
only the two parameters of the two-level blocking are -- so the path without the fused extend-add is reached by the choice of the matrices, not by an override.)
Bounds: DESIGN.md section 0 row a17 -- residual 1e-10, against the oracle's Cholesky 1e-9, a non-positive-definite matrix reported."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from ipc_amd import scene

pytestmark = pytest.mark.gpu

RESIDUAL = 1e-10
VS_ORACLE = 1e-9


def _context(gpu_lib, case):
    c = gpu_lib.Context(0)
    if case == "stack":
        n = 13
        V, F, nA = scene.make_mat_stack(n, 2, gap=1.2e-3)
        nn = V.shape[0]
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.opt_init(0.01, False)
        top = np.where((np.arange(nn) < nA) & (V[:, 1] > V[:nA, 1].mean()))[0]  # the pairs of stacked_pattern(13)
        bot = np.where((np.arange(nn) >= nA) & (V[:, 1] < V[nA:, 1].mean()))[0]
        near = cKDTree(V[top][:, [0, 2]]).query_ball_point(V[bot][:, [0, 2]], 1.6 / (n - 1))
        pairs = np.array([(bot[i], top[j]) for i, x in enumerate(near) for j in x], np.int32)
        c.set_pattern(pairs)
        c.assemble_newton(0.01 ** 2, True, with_gradient=False)
    else:
        V, F = scene.make_mat(int(case[3:]))
        Vt = scene.twist_state(scene.jitter(V, F), 0.5)
        left, right = scene.border_verts(V, 0.01)
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.opt_init(0.04, False)
        c.set_dbc(np.concatenate([left, right]), 2)
        c.set_positions(Vt)
        c.set_pattern()
        c.assemble_newton(0.04 ** 2, True, with_gradient=False)
    c.analyze_pattern()
    return c, np.ascontiguousarray(V, np.float64)


@pytest.fixture(scope="module", params=["stack", "mat40", "mat60"])
def solved(request, gpu_lib):
    c, V = _context(gpu_lib, request.param)
    rows, _ = c.get_dims()
    b = np.random.default_rng(23).normal(size=rows)
    assert c.factorize()
    x = c.solve(b)
    yield dict(case=request.param, c=c, V=V, b=b, x=x)
    c.close()


def test_levels_take_the_paths_the_docstring_names(solved):
    from test_mf_plan import make_plan
    from test_mf_symbolic import analyze
    from test_sharding_gloo import _shim_lib
    shim, c = _shim_lib(), solved["c"]
    ia, ja = c.get_pattern()
    o = analyze(shim, np.ascontiguousarray(ia, np.int32), np.ascontiguousarray(ja, np.int32), solved["V"], leaf=12)
    assert np.array_equal(c.entry_destinations(), o["aDst"])  # the same analysis as the device's
    p = make_plan(shim, o)
    fusedEA = [L["fuseEA"] for L in p["levels"] if L["ea"][1]]
    print(f"case {solved['case']}: extend-add levels, fused into the Schur kernel: {fusedEA}")
    assert not all(fusedEA)  # k_extend_add with ownOnly = 0
    assert any(fusedEA) == (solved["case"] == "mat60")  # k_extend_add with ownOnly = 1 + k_big_schur64_ea


def test_residual_and_oracle(solved, orc):
    c, b, x = solved["c"], solved["b"], solved["x"]
    res = np.linalg.norm(c.multiply(x) - b) / np.linalg.norm(b)
    ia, ja = c.get_pattern()
    ch = orc.Chol(ia, ja, 4)
    assert ch.factorize(c.get_a())
    xo = ch.solve(b)
    err = np.abs(x - xo).max() / np.abs(xo).max()
    print(f"case {solved['case']}: {len(b)} rows, residual {res:.2e}, against the oracle {err:.2e}")
    assert res <= RESIDUAL
    assert err < VS_ORACLE


def test_same_bits_from_two_calls_and_two_contexts(solved, gpu_lib):
    c, b, x = solved["c"], solved["b"], solved["x"]
    assert c.factorize()
    assert np.array_equal(c.solve(b).view(np.uint64), x.view(np.uint64))
    c2, _ = _context(gpu_lib, solved["case"])
    assert c2.factorize()
    x2 = c2.solve(b)
    c2.close()
    assert np.array_equal(x2.view(np.uint64), x.view(np.uint64))


def test_not_positive_definite_is_reported(solved, gpu_lib):
    c, _ = _context(gpu_lib, solved["case"])  # (a context of its own: the fixture's matrix stays as it is)
    rows, _ = c.get_dims()
    ia, _ = c.get_pattern()
    k = 3 * (rows // 6)
    c.set_coeff(k, k, -abs(c.get_a()[ia[k]]))
    assert not c.factorize()
    c.close()
