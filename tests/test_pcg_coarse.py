"""The host side of the two-level preconditioner (IPCGPU_PRECOND_TWO_LEVEL): the aggregation unit ipc_amd/csrc/pcg_coarse.cpp read through
tests/pcg_coarse/shim.cpp, against the numpy model tests/pcg_two_level_numpy.py.  No GPU.  Measured figures are printed before they are asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ipc_amd import scene

import pcg_numpy
import pcg_two_level_cases as cases
import pcg_two_level_numpy as model

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNIT = [os.path.join(ROOT, "ipc_amd", "csrc", "pcg_coarse.cpp"), os.path.join(ROOT, "ipc_amd", "csrc", "pcg_coarse.h")]


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "pcg_coarse", "_build", "libpcgcoarse.so")
    srcs = [os.path.join(HERE, "pcg_coarse", "shim.cpp")] + UNIT
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + srcs[:2] + ["-o", so])
    return C.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def node_rows(ia):
    ia = np.asarray(ia, np.int32)
    return np.ascontiguousarray(ia[0:-1:3]), np.ascontiguousarray(ia[1::3] - ia[0:-1:3])


def aggregate(shim, ia, ja, fixed):
    """everything the unit emits, as a dict of int32 arrays"""
    row_base, row_len = node_rows(ia)
    n = len(row_base)
    ja = np.ascontiguousarray(ja, np.int32)
    fx = np.ascontiguousarray(fixed, np.uint8)
    shim.shim_build(n, ptr(ja), ptr(row_base), ptr(row_len), ptr(fx))
    d = np.zeros(4, np.int32)
    shim.shim_dims(ptr(d))
    n_agg, cnnz, n_pairs, n_ent = (int(x) for x in d)

    def z(k):
        return np.zeros(k, np.int32)

    o = dict(n=n, n_agg=n_agg, agg_of=z(n), agg_ptr=z(n_agg + 1), agg_nodes=z(n), agg_free=z(n_agg), cia=z(6 * n_agg + 1), cja=z(cnnz), c_row_base=z(2 * n_agg),
             c_row_len=z(2 * n_agg), pair_i=z(n_pairs), pair_j=z(n_pairs), pair_ptr=z(n_pairs + 1), pair_slot=z(4 * n_pairs), ent_slot=z(n_ent), ent_row=z(n_ent),
             ent_col=z(n_ent), ent_trans=z(n_ent), row_base=row_base, row_len=row_len)
    shim.shim_aggregates(ptr(o["agg_of"]), ptr(o["agg_ptr"]), ptr(o["agg_nodes"]), ptr(o["agg_free"]))
    shim.shim_coarse_pattern(ptr(o["cia"]), ptr(o["cja"]), ptr(o["c_row_base"]), ptr(o["c_row_len"]))
    shim.shim_pairs(ptr(o["pair_i"]), ptr(o["pair_j"]), ptr(o["pair_ptr"]), ptr(o["pair_slot"]))
    shim.shim_entries(ptr(o["ent_slot"]), ptr(o["ent_row"]), ptr(o["ent_col"]), ptr(o["ent_trans"]))
    return o


def two_bars(orc):
    """two bars without any coupling: a pattern of two components"""
    V, F = scene.make_bar(6, 2, 2, size=(3.0, 0.5, 0.5))
    V2 = np.vstack([V, V + np.array([0.0, 2.0, 0.0])])
    F2 = np.vstack([F, F + V.shape[0]]).astype(np.int32)
    m = orc.Mesh(V2, F2, **cases.MATERIAL)
    fixed = np.zeros(V2.shape[0], dtype=bool)
    fixed[scene.border_verts(V2, 0.01)[0]] = True
    m.set_dbc(np.nonzero(fixed)[0].astype(np.int32), 2)
    ia, ja = m.pattern()
    comp = (np.arange(V2.shape[0]) >= V.shape[0]).astype(int)
    return dict(V=V2, F=F2, Vt=V2, m=m, ia=ia, ja=ja, fixed=fixed, comp=comp)


@pytest.fixture(scope="module")
def shapes(orc):
    return dict(bar=cases.make(orc, "bar"), sheet=cases.make(orc, "sheet"), two_bars=two_bars(orc))


def adjacency(ia, ja):
    n = (len(ia) - 1) // 3
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia)) // 3
    cols = np.asarray(ja) // 3
    nb = [set() for _ in range(n)]
    for u, w in set(zip(rows.tolist(), cols.tolist())):
        if u != w:
            nb[u].add(w), nb[w].add(u)
    return nb


@pytest.mark.parametrize("name", ["bar", "sheet", "two_bars"])
def test_aggregation_and_lists(shim, shapes, name):
    s = shapes[name]
    o = aggregate(shim, s["ia"], s["ja"], s["fixed"])
    n, n_agg, agg = o["n"], o["n_agg"], o["agg_of"]
    print(name, "nodes", n, "aggregates", n_agg, "pairs", len(o["pair_i"]), "coarse nnz", len(o["cja"]))
    # every node in exactly one aggregate; the sorted list says the same
    assert agg.min() == 0 and agg.max() == n_agg - 1 and len(np.unique(agg)) == n_agg
    assert sorted(o["agg_nodes"].tolist()) == list(range(n))
    for I in range(n_agg):
        mine = o["agg_nodes"][o["agg_ptr"][I]:o["agg_ptr"][I + 1]]
        assert len(mine) > 0 and np.all(agg[mine] == I) and np.all(np.diff(mine) > 0)
        assert o["agg_free"][I] == np.count_nonzero(~s["fixed"][mine])
    # connected in the node graph (hence inside one component)
    nb = adjacency(s["ia"], s["ja"])
    for I in range(n_agg):
        mine = set(o["agg_nodes"][o["agg_ptr"][I]:o["agg_ptr"][I + 1]].tolist())
        seen, todo = set(), [min(mine)]
        while todo:
            v = todo.pop()
            if v in seen:
                continue
            seen.add(v)
            todo += [w for w in nb[v] if w in mine and w not in seen]
        assert seen == mine, I
    if "comp" in s:
        for I in range(n_agg):
            assert len(set(s["comp"][agg == I].tolist())) == 1
    # deterministic
    o2 = aggregate(shim, s["ia"], s["ja"], s["fixed"])
    assert all(np.array_equal(o[k], o2[k]) for k in o if isinstance(o[k], np.ndarray))
    # the coarse pattern: 6 nAgg rows, upper, diagonal first, columns ascending, node-block rows
    cia, cja = o["cia"], o["cja"]
    assert len(cia) == 6 * n_agg + 1 and cia[0] == 0 and cia[-1] == len(cja)
    for r in range(6 * n_agg):
        row = cja[cia[r]:cia[r + 1]]
        assert row[0] == r and np.all(np.diff(row) > 0) and row[-1] < 6 * n_agg
    assert np.array_equal(o["c_row_base"], cia[0:-1:3]) and np.array_equal(o["c_row_len"], cia[1::3] - cia[0:-1:3])
    assert np.all(cia[2::3] - cia[1::3] == o["c_row_len"] - 1) and np.all(cia[3::3] - cia[2::3] == o["c_row_len"] - 2)
    # the lists: every stored block of the upper storage exactly once, in the pair of its two aggregates; sorted pairs; fixed order inside a pair
    row_base, row_len = o["row_base"], o["row_len"]
    stored = {}
    for u in range(n):
        stored[int(row_base[u])] = (u, u)
        for k in range(row_base[u] + 3, row_base[u] + row_len[u], 3):
            stored[k] = (u, int(s["ja"][k]) // 3)
    assert sorted(o["ent_slot"].tolist()) == sorted(stored)
    keys = list(zip(o["pair_i"].tolist(), o["pair_j"].tolist()))
    assert keys == sorted(set(keys)) and all(i <= j for i, j in keys)
    assert o["pair_ptr"][0] == 0 and o["pair_ptr"][-1] == len(o["ent_slot"]) and np.all(np.diff(o["pair_ptr"]) > 0)
    for p, (I, J) in enumerate(keys):
        e = slice(o["pair_ptr"][p], o["pair_ptr"][p + 1])
        assert np.all(np.diff(o["ent_slot"][e]) > 0)
        for k, u, w, t in zip(o["ent_slot"][e], o["ent_row"][e], o["ent_col"][e], o["ent_trans"][e]):
            assert stored[int(k)] == (u, w)
            assert (agg[w], agg[u]) == (I, J) if t else (agg[u], agg[w]) == (I, J)
            assert t == (1 if agg[u] > agg[w] else 0)
    # the slots of a pair's coarse blocks are where the coarse pattern holds them
    for p, (I, J) in enumerate(keys):
        tt, tr, rt, rr = o["pair_slot"][4 * p:4 * p + 4]
        assert cja[tt] == 6 * J and cia[6 * I] <= tt < cia[6 * I + 1]
        assert cja[tr] == 6 * J + 3 and cia[6 * I] <= tr < cia[6 * I + 1]
        assert cja[rr] == 6 * J + 3 and cia[6 * I + 3] <= rr < cia[6 * I + 4]
        assert rt == -1 if I == J else (cja[rt] == 6 * J and cia[6 * I + 3] <= rt < cia[6 * I + 4])
    # and the coarse pattern holds nothing else: 3 blocks per diagonal pair, 4 per off-diagonal one
    n_diag = sum(1 for i, j in keys if i == j)
    assert n_diag == n_agg
    assert len(cja) == 12 * n_agg + 9 * n_agg + 36 * (len(keys) - n_agg)


def galerkin_through_lists(o, a, X, fixed):
    """P^T A P evaluated the way the device does: per pair, over its list, into the coarse CSR slots"""
    P, cnt = model.node_blocks(o["agg_of"], X, fixed)
    assert np.array_equal(cnt, o["agg_free"])
    slot, u, w, t = o["ent_slot"], o["ent_row"], o["ent_col"], o["ent_trans"].astype(bool)
    ln = o["row_len"][u]
    B = np.zeros((len(slot), 3, 3))
    diag = u == w
    for r, off in enumerate((0 * ln, ln - 1, 2 * ln - 3)):
        for c in range(3):
            B[~diag, r, c] = a[(slot + off + c)[~diag]]
    d = slot[diag]
    dl = ln[diag]
    D = np.zeros((len(d), 3, 3))
    for (r, c), k in {(0, 0): d, (0, 1): d + 1, (0, 2): d + 2, (1, 1): d + dl, (1, 2): d + dl + 1, (2, 2): d + 2 * dl - 1}.items():
        D[:, r, c] = D[:, c, r] = a[k]
    B[diag] = D
    B[t] = B[t].transpose(0, 2, 1)
    i, j = np.where(t, w, u), np.where(t, u, w)
    M = np.einsum("nki,nkl,nlj->nij", P[i], B, P[j])
    pair_of = np.repeat(np.arange(len(o["pair_i"])), np.diff(o["pair_ptr"]))
    same = (o["pair_i"] == o["pair_j"])[pair_of] & ~diag
    M[same] += M[same].transpose(0, 2, 1)
    G = np.zeros((len(o["pair_i"]), 6, 6))
    np.add.at(G, pair_of, M)
    ca = np.zeros(len(o["cja"]))
    for p, (I, J) in enumerate(zip(o["pair_i"], o["pair_j"])):
        g = G[p].copy()
        if I == J:
            if cnt[I] < 4:
                g[3:, 3:] = np.eye(3)
            if cnt[I] < 1:
                g[:3, :3] = np.eye(3)
        for q, (r0, c0) in enumerate(((0, 0), (0, 3), (3, 0), (3, 3))):
            s0 = o["pair_slot"][4 * p + q]
            if s0 < 0:
                continue
            cn = 2 * I + (r0 // 3)
            L = o["c_row_len"][cn]
            if I == J and r0 == c0:
                ca[s0:s0 + 3], ca[s0 + L:s0 + L + 2], ca[s0 + 2 * L - 1] = g[r0, c0:c0 + 3], g[r0 + 1, c0 + 1:c0 + 3], g[r0 + 2, c0 + 2]
            else:
                for r, off in enumerate((0, L - 1, 2 * L - 3)):
                    ca[s0 + off:s0 + off + 3] = g[r0 + r, c0:c0 + 3]
    return ca


def random_spd_values(ia, ja, rng):
    """random values on the pattern, every off-diagonal entry filled, strictly diagonally dominant"""
    a = rng.normal(size=len(ja))
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    off = rows != ja
    s = np.zeros(len(ia) - 1)
    np.add.at(s, rows[off], np.abs(a[off]))
    np.add.at(s, ja[off], np.abs(a[off]))
    a[~off] = s[rows[~off]] + 1.0
    return a


@pytest.mark.parametrize("name", ["bar", "sheet", "two_bars"])
def test_galerkin_through_the_lists(shim, shapes, name):
    s = shapes[name]
    o = aggregate(shim, s["ia"], s["ja"], s["fixed"])
    rng = np.random.default_rng(7)
    a = random_spd_values(np.asarray(s["ia"]), np.asarray(s["ja"]), rng)
    X = rng.normal(size=s["V"].shape)
    ref = model.upper_csr_values(o["cia"], o["cja"], model.galerkin(s["ia"], s["ja"], a, o["agg_of"], X, s["fixed"]))
    got = galerkin_through_lists(o, a, X, s["fixed"])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(name, "Galerkin through the lists against numpy's P^T A P:", err)
    assert err <= 1e-13


def test_small_aggregate_gets_identity_rotation_block(shim, shapes):
    """all but three nodes of an aggregate fixed: translations only, an identity in its rotation block, zeros beside it"""
    s = shapes["bar"]
    o = aggregate(shim, s["ia"], s["ja"], s["fixed"])
    I = int(np.argmax(np.diff(o["agg_ptr"])))
    mine = o["agg_nodes"][o["agg_ptr"][I]:o["agg_ptr"][I + 1]]
    fixed = s["fixed"].copy()
    fixed[mine[3:]] = True
    o = aggregate(shim, s["ia"], s["ja"], fixed)
    assert o["agg_free"][I] == 3
    rng = np.random.default_rng(8)
    a = random_spd_values(np.asarray(s["ia"]), np.asarray(s["ja"]), rng)
    X = rng.normal(size=s["V"].shape)
    ca = galerkin_through_lists(o, a, X, fixed)
    r, up = pcg_numpy.upper_csr_to_full(o["cia"], o["cja"], ca), None
    Ac = np.zeros((6 * o["n_agg"], 6 * o["n_agg"]))
    np.add.at(Ac, (r[0], r[1]), r[2])
    rot = slice(6 * I + 3, 6 * I + 6)
    assert np.array_equal(Ac[rot, rot], np.eye(3))
    rest = Ac[rot].copy()
    rest[:, rot] = 0.0
    assert not rest.any()
    assert np.abs(Ac[6 * I:6 * I + 3, 6 * I:6 * I + 3]).min() > 0
    ref = model.galerkin(s["ia"], s["ja"], a, o["agg_of"], X, fixed)
    assert np.abs(Ac - ref).max() <= 1e-13 * np.abs(ref).max()
    np.linalg.cholesky(Ac)


def test_sanitized_run_of_the_unit(shapes, tmp_path):
    """the unit on the sheet pattern inside a stand-alone program built with the address and undefined-behaviour sanitizers"""
    s = shapes["sheet"]
    row_base, row_len = node_rows(s["ia"])
    inp = tmp_path / "sheet.txt"
    with open(inp, "w") as f:
        f.write(f"{len(row_base)} {len(s['ja'])}\n")
        for arr in (s["ja"], row_base, row_len, s["fixed"].astype(int)):
            f.write(" ".join(str(int(x)) for x in arr) + "\n")
    exe = tmp_path / "asan_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "pcg_coarse", "asan_main.cpp"),
                           UNIT[0], "-o", str(exe)])
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == "ok"


def test_the_coarse_space_pays_on_the_sheet(shim, shapes):
    """the model with the library's aggregation, sheet, 1e-5: block Jacobi needs at least 2.5 x the two-level iterations (measured with the greedy rule of the
    issue: 215 / 54 = 4.0 x; the margin allows for another visiting order)"""
    s = shapes["sheet"]
    o = aggregate(shim, s["ia"], s["ja"], s["fixed"])
    a = s["m"].assemble_hessian(len(s["ja"]), cases.DTSQ, projectDBC=True)
    b = cases.rhs(s)
    n = len(b)
    _, n_bj = pcg_numpy.cg(s["ia"], s["ja"], a, b, 1e-5, n, block_jacobi=True)
    _, n_tl = model.cg(s["ia"], s["ja"], a, b, 1e-5, n, o["agg_of"], s["Vt"], s["fixed"])
    print("sheet, 1e-5: aggregates", o["n_agg"], "block Jacobi", n_bj, "two-level", n_tl, "ratio", n_bj / n_tl)
    assert n_bj >= 2.5 * n_tl
