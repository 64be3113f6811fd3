"""The product loop of the 64 x 64 Schur kernels (`schur_tile64_core` in ipc_amd/csrc/mf_numeric.hip: k_big_schur64_ea, k_big_schur64, k_big_bulk) runs its
full 16-column chunks without column clamps and operand selects and finishes with a clamped, masked tail of at most three chunks.  Through the solver's C API:

  * the residual of the CSR product is at round-off (the bound of test_gpu_parity.test_two_level_blocking_of_wide_fronts, 1e-12),
  * two factorisations of the same matrix give the same solution bit for bit,
  * a negated diagonal entry still raises the not-positive-definite flag.

Which nc reach which kernel.  A front's nc is three times its number of nodes, and the separators of a sheet of two node layers have an even number of nodes:
sheets alone give nc = 30, 36, 42, 48, ... on the multi-workgroup path.  The case "bars" therefore adds, to a mat47 sheet, seven loose bars whose cross-section
-- a zig-zag strip of P points, every one a separator of the dissection -- has P = 4, 5, 6, 7, 10, 11 and 16 nodes: nc = 12, 15, 18, 21, 30, 33, 48.  Their
fronts fit the single-workgroup kernel, but they sit on levels of the tree where the sheet's fronts do not, and a level's few fitting fronts join its batched
launches (classifyFronts, mf_plan.cpp).  With the default tuning these levels (3, 4 and 5 of the tree) have more than 512 Schur tiles and take k_big_schur64_ea, so
that kernel's loop meets, on ONE level each, fronts of

    nc = 12 and 15              no full chunk: the tail alone (the widths 16 and below; 16 itself is no multiple of 3)
    nc = 18 and 21              one full chunk and a tail of two and five columns (for 17)
    nc = 30, 33, 36, 48         (for 31, 32, 33, 48: two full chunks less two columns, two full chunks plus one column, three full chunks)
    nc = 165 and 198            the main loop more than once

with update blocks N - nc of 12 .. 399 rows, most of them no multiple of 32 or 64.  The test asserts this list on the host: the solver's analysis is repeated
through tests/mf_symbolic/shim.cpp (pinned to the device's by the entry destinations) and the launch plan is read the way tests/test_mf_plan.py reads it.
`forced` factors the own columns in outer blocks of 64 (k_big_bulk: every pass is exactly 64 columns, chunks [cLo / 16, cLo / 16 + 4), one round of the main
loop and a tail of two full chunks).  The sheets (29, 47, 60) and the stacked sheets with contact pairs are the plain cases: 60 takes k_big_schur64_ea on
three levels, the others k_big_schur (whose loop is the one it was) and, forced, k_big_bulk.  k_big_schur64 itself is launched by no single-device plan."""
import numpy as np
import pytest

from ipc_amd import scene

pytestmark = pytest.mark.gpu

RESIDUAL = 1e-12
BAR_POINTS = (4, 5, 6, 7, 10, 11, 16)
NC_ON_SCHUR64_EA = {12, 15, 18, 21, 30, 33, 36, 48, 165, 198}


def strip_bar(P, nx, h=0.02, origin=(0.0, 0.0, 0.0)):
    """a bar whose cross-section is a zig-zag strip of P points in two rows, extruded over nx layers of nodes; three tets per prism, oriented positively"""
    top = (P + 1) // 2
    yz = np.array([[0.0, k * h] for k in range(top)] + [[0.866 * h, (k + 0.5) * h] for k in range(P - top)])
    tri = []
    for k in range(P - top):
        tri.append((k, k + 1, top + k))
        if k + 1 < P - top:
            tri.append((k + 1, top + k + 1, top + k))
    if P - top < top - 1:
        tri.append((top - 2, top - 1, P - 1))  # P odd: the last point of the longer row
    V = np.array([[origin[0] + i * h, origin[1] + y, origin[2] + z] for i in range(nx) for y, z in yz])
    T = []
    for i in range(nx - 1):
        for a, b, c in tri:
            a0, b0, c0, a1, b1, c1 = [i * P + q for q in (a, b, c)] + [(i + 1) * P + q for q in (a, b, c)]
            T += [(a0, b0, c0, a1), (b0, c0, a1, b1), (c0, a1, b1, c1)]
    T = np.array(T, np.int32)
    vol = np.einsum("ij,ij->i", np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]), V[T[:, 3]] - V[T[:, 0]])
    T[vol < 0] = T[vol < 0][:, [0, 2, 1, 3]]
    assert np.abs(vol).min() > 1e-12 and len(np.unique(T)) == len(V)
    return V, T


def sheet_and_bars():
    V, F = scene.make_mat(47)
    Vs, Fs, off = [V], [F], V.shape[0]
    for k, P in enumerate(BAR_POINTS):
        Vb, Tb = strip_bar(P, (32 * 12) // P, origin=(0.0, 1.0 + 0.3 * k, 0.0))
        Vs.append(Vb)
        Fs.append(Tb + off)
        off += Vb.shape[0]
    return np.ascontiguousarray(np.concatenate(Vs), np.float64), np.concatenate(Fs).astype(F.dtype)


def _context(gpu_lib, case, forced):
    c = gpu_lib.Context(0)
    c.set_solver_tuning(0.0, 64) if forced else c.set_solver_tuning(1e9, 256)
    V = None
    if case == "stack":
        V, F, nA = scene.make_mat_stack(24, 2, gap=1.2e-3)
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.opt_init(0.01, False)
        top = np.where((np.arange(V.shape[0]) < nA) & (V[:, 1] > V[:nA, 1].mean()))[0]
        bot = np.where((np.arange(V.shape[0]) >= nA) & (V[:, 1] < V[nA:, 1].mean()))[0]
        k = min(len(top), len(bot))
        c.set_pattern(np.stack([top[:k], bot[:k]], 1).astype(np.int32))
        c.assemble_newton(0.01 ** 2, True, with_gradient=False)
    elif case == "bars":
        V, F = sheet_and_bars()
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.opt_init(0.04, False)
        # rest state, no Dirichlet nodes: the mass term makes every loose body's block positive definite
        c.set_pattern()
        c.assemble_newton(0.04 ** 2, True, with_gradient=False)
    else:
        V, F = scene.make_mat(case)
        Vt = scene.twist_state(scene.jitter(V, F), 0.5)
        left, right = scene.border_verts(V, 0.01)
        c.set_mesh(V, F, YM=2e4, PR=0.4, density=1000.0)
        c.opt_init(0.04, False)
        c.set_dbc(np.concatenate([left, right]), 2)
        c.set_positions(Vt)
        c.set_pattern()
        c.assemble_newton(0.04 ** 2, True, with_gradient=False)
    c.analyze_pattern()  # (the tuning is read by the set-up of the numeric phase, here)
    return c, V


def _nc_by_kernel(c, V):
    """the fronts of the multi-workgroup path by the Schur kernel of their level, from the host planner on the solver's own pattern"""
    from test_mf_plan import big_of, make_plan
    from test_mf_symbolic import analyze
    from test_sharding_gloo import _shim_lib
    shim = _shim_lib()
    ia, ja = c.get_pattern()
    o = analyze(shim, np.ascontiguousarray(ia, np.int32), np.ascontiguousarray(ja, np.int32), V, leaf=12)
    assert np.array_equal(c.entry_destinations(), o["aDst"])  # the same analysis as the device's
    o["N"], o["nc"] = 3 * np.diff(o["idxPtr"]), 3 * np.diff(o["firstNode"])
    p = make_plan(shim, o)
    out = {"k_big_schur64_ea": [], "k_big_schur": []}
    for L in p["levels"]:
        big = big_of(p, L)
        assert L["fuseEA"] == L["schur64"]
        out["k_big_schur64_ea" if L["fuseEA"] else "k_big_schur"].append([(int(o["nc"][s]), int(o["N"][s])) for s in big if o["N"][s] > o["nc"][s]])
    return out


def test_the_bars_put_the_short_fronts_on_the_64_x_64_kernel(gpu_lib):
    c, V = _context(gpu_lib, "bars", False)
    levels = [lv for lv in _nc_by_kernel(c, V)["k_big_schur64_ea"] if lv]
    c.close()
    print("k_big_schur64_ea levels (nc/N):", [" ".join(f"{a}/{b}" for a, b in lv) for lv in levels])
    assert NC_ON_SCHUR64_EA <= {nc for lv in levels for nc, _ in lv}
    assert any({12, 15, 18, 21} <= {nc for nc, _ in lv} and max(nc for nc, _ in lv) >= 48 for lv in levels)  # one launch mixes them
    m = [N - nc for lv in levels for nc, N in lv]
    assert any(x % 32 for x in m) and any(x % 64 for x in m) and any(x < 32 for x in m) and any(x > 64 for x in m)


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("case", ["bars", 29, 47, 60, "stack"])
def test_schur_main_loop_and_tail(gpu_lib, case, forced):
    c, _ = _context(gpu_lib, case, forced)
    rows, _ = c.get_dims()
    b = np.random.default_rng(11).normal(size=rows)
    assert c.factorize()
    x1 = c.solve(b)
    res = np.linalg.norm(c.multiply(x1) - b) / np.linalg.norm(b)
    print(f"case {case} forced {forced}: {rows} rows, residual {res:.2e}")
    assert res <= RESIDUAL
    assert c.factorize()
    x2 = c.solve(b)
    assert np.array_equal(x1.view(np.uint64), x2.view(np.uint64))  # the same bits from two factorisations
    ia, _ = c.get_pattern()
    k = 3 * (rows // 6)
    c.set_coeff(k, k, -abs(c.get_a()[ia[k]]))
    assert not c.factorize()
    c.close()
