"""The children of the batched fronts as the tile kernels of the extend-add read them (`ipc_amd/csrc/mf_plan.cpp`: childMaps, pushTileRecord): per child one map
parent scalar row -> child scalar row, per tile one 16-int record with the front, the tile and the first two children inline, further children in `kidRec`.
Run on the host through `tests/mf_symbolic/shim_child_maps.cpp` (shim.cpp plus a fetch for the new arrays) and checked against a restatement from the front
index lists.  No GPU.

`stacked_pattern(13)` is the smallest case with two or more multi-workgroup fronts on a level and a front with nc >= 192 (tests/test_mf_plan.py).  The second
input, `bridged_sheets`, is four sheets that touch only through a few contact pairs at their corners: its batched fronts include fronts with three and more
children (asserted below), so the records behind the two inline ones are walked."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from ipc_amd import scene
from test_mf_plan import big_of, make_plan, off64, span
from test_mf_symbolic import analyze, stacked_pattern

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TS = 64


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "mf_symbolic", "_build", "libmfsym_maps.so")
    srcs = [os.path.join(HERE, "mf_symbolic", "shim_child_maps.cpp"), os.path.join(ROOT, "ipc_amd", "csrc", "mf_symbolic.cpp"),
            os.path.join(ROOT, "ipc_amd", "csrc", "mf_plan.cpp")]
    deps = srcs + [os.path.join(HERE, "mf_symbolic", "shim.cpp"), os.path.join(ROOT, "ipc_amd", "csrc", "mf_plan.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread"] + srcs + ["-o", so])
    return C.CDLL(so)


def scalar_upper_csr(A):
    """block-structured upper scalar CSR of a symmetric node matrix (as test_mf_symbolic.stacked_pattern builds it)"""
    nn = A.shape[0]
    U = sp.triu(A, format="csr")
    rows = []
    for u in range(nn):
        cols = (3 * U.indices[U.indptr[u]:U.indptr[u + 1]][:, None] + np.arange(3)[None, :]).ravel()
        rows += [cols, cols[1:], cols[2:]]
    ia = np.zeros(3 * nn + 1, np.int32)
    ia[1:] = np.cumsum([len(r) for r in rows])
    return ia, np.concatenate(rows).astype(np.int32)


def bridged_sheets(n, layers=4):
    """`layers` matN sheets whose only connection is one contact pair per neighbouring pair of sheets, at alternating corners"""
    V, F, nA = scene.make_mat_stack(n, layers, gap=1.2e-3)
    nn = V.shape[0]
    I = np.concatenate([F[:, a] for a in range(4) for b in range(4)])
    J = np.concatenate([F[:, b] for a in range(4) for b in range(4)])
    ci, cj = [], []
    for k in range(layers - 1):
        corner = 0 if k % 2 == 0 else nA - 1
        ci.append(k * nA + corner)
        cj.append((k + 1) * nA + corner)
    I, J = np.concatenate([I, ci, cj]), np.concatenate([J, cj, ci])
    A = sp.coo_matrix((np.ones(len(I)), (I, J)), shape=(nn, nn)).tocsr()
    A.sum_duplicates()
    ia, ja = scalar_upper_csr(A)
    return np.ascontiguousarray(V, np.float64), ia, ja


def analysed(shim, ia, ja, V):
    o = analyze(shim, ia, ja, V, leaf=8)
    o["N"] = 3 * np.diff(o["idxPtr"])
    o["nc"] = 3 * np.diff(o["firstNode"])
    o["kids"] = [o["child"][o["childPtr"][s]:o["childPtr"][s + 1]].tolist() for s in range(o["ns"])]
    return o


def fetch_maps(shim, p):
    shim.shim_plan_fetch_maps.restype = C.c_longlong

    def fetch(name):
        n = shim.shim_plan_fetch_maps(name.encode(), None)
        assert n >= 0, name
        a = np.zeros(max(n, 1), np.int64)
        shim.shim_plan_fetch_maps(name.encode(), a.ctypes.data_as(C.c_void_p))
        return a[:n]
    for k in ("childMap", "kidBase", "eaTile", "schurTile", "schurTileOff"):
        p[k] = fetch(k)
    p["kidRec"] = fetch("kidRec").reshape(-1, 4)
    p["TILE_REC"], p["PAD"] = (int(x) for x in fetch("geometry"))
    return p


def nodes_of(sym, s):
    return sym["idx"][sym["idxPtr"][s]:sym["idxPtr"][s + 1]]


def check_maps(sym, p):
    """every batched front, child and parent row: the map against the index lists.  Returns the largest number of children of a batched front."""
    PAD = p["PAD"]
    maxN = max([sym["N"][s] for L in p["levels"] for s in big_of(p, L)] + [0])
    assert np.all(p["childMap"][:maxN + PAD] == -1)  # the map of an absent child
    at, mostKids, used = maxN + PAD, 0, 0
    for L in p["levels"]:
        for s in big_of(p, L):
            pn, N = nodes_of(sym, s), int(sym["N"][s])
            base = int(p["kidBase"][s])
            assert base == used
            used += len(sym["kids"][s])
            mostKids = max(mostKids, len(sym["kids"][s]))
            for q, c in enumerate(sym["kids"][s]):  # ascending order, as the sums are formed
                lo, hi, Nc, mo = (int(x) for x in p["kidRec"][base + q])
                assert off64(lo, hi) == sym["frontOff"][c] and Nc == sym["N"][c] and mo == at
                m = p["childMap"][mo:mo + N + PAD]
                at += N + PAD
                cn = nodes_of(sym, c)
                pos = np.searchsorted(cn, pn)
                has = (pos < len(cn)) & (cn[np.minimum(pos, len(cn) - 1)] == pn)
                want = np.where(np.repeat(has, 3), np.repeat(3 * pos, 3) + np.tile(np.arange(3), len(pn)), -1)
                assert np.array_equal(m[:N], want)  # -1 exactly where the child's structure lacks the parent's row
                assert np.all(m[N:] == -1)
                I = np.nonzero(m[:N] >= 0)[0]
                assert np.array_equal(cn[m[I] // 3], pn[I // 3]) and np.array_equal(m[I] % 3, I % 3)  # the child-local row holds that parent row
                assert np.all(m[I] >= sym["nc"][c])  # ... in the child's update block
    assert at == len(p["childMap"])
    assert all(p["kidBase"][s] == -1 for s in range(sym["ns"]) if s not in {s for L in p["levels"] for s in big_of(p, L)})
    return mostKids


def check_tile(sym, p, rec, s, ti, tj):
    T = p["TILE_REC"]
    assert T == 16 and len(rec) == T
    kids = sym["kids"][s]
    assert (rec[0], rec[1], off64(rec[2], rec[3])) == (sym["N"][s], sym["nc"][s], sym["frontOff"][s])
    assert (rec[4], rec[5], rec[6], rec[7]) == (ti, tj, len(kids), p["kidBase"][s])
    for q in range(2):
        k = rec[8 + 4 * q:12 + 4 * q]
        if q < len(kids):
            assert np.array_equal(k, p["kidRec"][p["kidBase"][s] + q])  # the front's children in ascending order (check_maps pins kidRec on them)
        else:
            assert np.all(k == 0)  # absent: the map of -1s at offset 0, every slot unselected


def check_tiles(sym, p):
    """every tile record of both kernels: the front, the tile and the inline children.  Returns (extend-add tiles, Schur tiles with the extend-add fused in)."""
    T = p["TILE_REC"]
    front_at = {int(sym["frontOff"][s]): s for L in p["levels"] for s in big_of(p, L)}
    nEa = nSchur = 0
    for l, L in enumerate(p["levels"]):
        for i in span(p, L["ea"]):
            r, ti, tj, no = (int(x) for x in p["ea"][i])
            d = p["bigFd"][64 * r:64 * r + 64]
            check_tile(sym, p, p["eaTile"][T * i:T * i + T], front_at[off64(d[0], d[1])], ti, tj)
            assert no == i  # (the kernel takes the tile's entries of A from aPtr[i])
            nEa += 1
        if L["fuseEA"]:
            assert p["schurTileOff"][l] == nSchur
            for w in range(L["schur"][1]):
                a = p["desc"][L["schur"][0] + 2 * w]
                i = nSchur + w
                check_tile(sym, p, p["schurTile"][T * i:T * i + T], int(a[0]), int(a[1]), int(a[2]))
            nSchur += L["schur"][1]
    assert len(p["eaTile"]) == T * max(nEa, 1) and len(p["schurTile"]) == T * max(nSchur, 1)
    return nEa, nSchur


@pytest.fixture(scope="module")
def sym13(shim):
    V, G, ia, ja = stacked_pattern(13)
    return analysed(shim, ia, ja, V)


@pytest.mark.parametrize("tune", [{}, {"schur64Min": 1}, {"fusedLds": 4096, "schur64Min": 1}], ids=["default", "fuseEA", "small-fronts-batched"])
def test_stacked_13(shim, sym13, tune):
    p = fetch_maps(shim, make_plan(shim, sym13, **tune))
    check_maps(sym13, p)
    nEa, nSchur = check_tiles(sym13, p)
    assert nEa > 0 and (nSchur > 0) == ("schur64Min" in tune)


def test_fronts_with_three_and_more_children(shim):
    V, ia, ja = bridged_sheets(9)
    sym = analysed(shim, ia, ja, V)
    p = fetch_maps(shim, make_plan(shim, sym, fusedLds=4096, schur64Min=1))  # (small fronts batched too)
    assert check_maps(sym, p) >= 3
    nEa, nSchur = check_tiles(sym, p)
    assert nEa > 0 and nSchur > 0
