"""Growth rules of the contact pattern (`ipc_amd/csrc/contact_pattern.cpp`: which node pairs of the contact sets join the solver's pattern, when a new
pattern is needed, when the accumulated union is dropped) on hand-made pairs over a path graph of 8 nodes.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_PATH = 8  # mesh edges i -- i + 1
N_NODES = 20000  # the ids beyond the path have no mesh neighbour: synthetic pairs of the drop rule


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "contact_pattern", "_build", "libcontactpattern.so")
    srcs = [os.path.join(HERE, "contact_pattern", "shim.cpp"), os.path.join(ROOT, "ipc_amd", "csrc", "contact_pattern.cpp"),
            os.path.join(ROOT, "ipc_amd", "csrc", "contact_pattern.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + srcs[:2] + ["-o", so])
    return C.CDLL(so)


def adjacency():
    nb = [[v for v in (i - 1, i + 1) if 0 <= v < N_PATH] for i in range(N_PATH)] + [[] for _ in range(N_NODES - N_PATH)]
    ptr = np.zeros(N_NODES + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in nb])
    return ptr, np.array([v for x in nb for v in x], np.int32)


def ints(pairs):
    return np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def non_mesh(shim, pairs):
    nbPtr, nb = adjacency()
    a = ints(pairs)
    out = np.zeros((max(len(a), 1), 2), np.int32)
    n = shim.shim_non_mesh_pairs(len(a), ptr(a), ptr(nbPtr), ptr(nb), ptr(out))
    return [tuple(p) for p in out[:n].tolist()]


def grow(shim, live, ahead):
    """live None: "not formed, the device already said the pattern lacks a block".  Returns (grown, look-ahead asked for)."""
    l, a = ints(live if live is not None else []), ints(ahead)
    asked = C.c_int(-1)
    g = shim.shim_grow(-1 if live is None else len(l), ptr(l), len(a), ptr(a), C.byref(asked))
    return bool(g), bool(asked.value)


def current(shim):
    n = shim.shim_size()
    pairs, flat = np.zeros((max(n, 1), 2), np.int32), np.full(2 * n + 1, -7, np.int32)
    assert shim.shim_fetch(ptr(pairs), ptr(flat)) == 2 * n
    assert flat[2 * n] == -7
    return [tuple(p) for p in pairs[:n].tolist()], flat[:2 * n].tolist()


def test_mesh_edges_leave_duplicates_collapse_output_sorted(shim):
    pairs = [(5, 7), (2, 3), (0, 2), (5, 7), (3, 2), (0, 7), (6, 0), (0, 2), (4, 4), (7, 6)]
    want = [(0, 2), (0, 7), (4, 4), (5, 7), (6, 0)]  # (2, 3), (3, 2), (7, 6) are mesh edges; a node is no neighbour of itself
    assert non_mesh(shim, pairs) == want
    assert non_mesh(shim, pairs[::-1]) == want
    assert non_mesh(shim, want) == want  # sorted input takes the branch without a sort
    assert non_mesh(shim, [(1, 2), (2, 1)]) == [] and non_mesh(shim, []) == []


def test_included_live_pairs_do_not_grow(shim):
    shim.shim_clear()
    assert grow(shim, [(0, 2), (0, 5), (3, 6)], []) == (True, True)
    before = current(shim)
    assert before == ([(0, 2), (0, 5), (3, 6)], [0, 2, 0, 5, 3, 6])
    for live in ([(0, 5)], [(0, 2), (3, 6)], [(0, 2), (0, 5), (3, 6)], []):
        assert grow(shim, live, [(1, 7)]) == (False, False)  # the look-ahead sets are not even asked for
        assert current(shim) == before
    assert grow(shim, [(0, 2), (1, 3)], []) == (True, True)  # one pair missing
    assert current(shim)[0] == [(0, 2), (0, 5), (1, 3), (3, 6)]


def test_unformed_live_pairs_always_grow(shim):
    shim.shim_clear()
    assert grow(shim, None, [(0, 2), (0, 5), (3, 6)]) == (True, True)
    before = current(shim)
    assert before[0] == [(0, 2), (0, 5), (3, 6)]
    assert grow(shim, None, [(0, 5)]) == (True, True)  # a subset of the current list: the device's answer is trusted
    assert current(shim) == before
    assert grow(shim, None, []) == (True, True)
    assert current(shim) == before


def test_growth_is_the_union_of_current_and_padded(shim):
    shim.shim_clear()
    grow(shim, [(0, 2), (3, 6)], [])
    # look-ahead >= 1: live pairs and look-ahead pairs together
    assert grow(shim, [(0, 2), (1, 4)], [(1, 4), (1, 5), (2, 7)]) == (True, True)
    pairs, flat = current(shim)
    assert pairs == [(0, 2), (1, 4), (1, 5), (2, 7), (3, 6)]
    assert flat == [v for p in pairs for v in p]  # the pair list, interleaved
    # look-ahead < 1 (no look-ahead pairs): current and live
    assert grow(shim, [(0, 3), (0, 7)], []) == (True, True)
    pairs, flat = current(shim)
    assert pairs == [(0, 2), (0, 3), (0, 7), (1, 4), (1, 5), (2, 7), (3, 6)]
    assert flat == [v for p in pairs for v in p]
    # live pairs not formed: current and look-ahead
    assert grow(shim, None, [(4, 6)]) == (True, True)
    assert current(shim)[0] == [(0, 2), (0, 3), (0, 7), (1, 4), (1, 5), (2, 7), (3, 6), (4, 6)]


@pytest.mark.parametrize("n_old,kept", [(4098, True), (4099, False)])
def test_union_dropped_beyond_three_times_padded_plus_4096(shim, n_old, kept):
    old = [(N_PATH + i, N_PATH + i + 2) for i in range(n_old)]
    assert non_mesh(shim, old[::-1]) == old  # nodes beyond the path graph: no mesh edge among them
    for live, ahead in (([(0, 2)], []), (None, [(0, 2)])):
        shim.shim_clear()
        assert grow(shim, old, [])[0] and shim.shim_size() == n_old  # (from an empty list: n_old <= 3 n_old + 4096)
        assert grow(shim, live, ahead) == (True, True)
        pairs, flat = current(shim)
        assert pairs == ([(0, 2)] + old if kept else [(0, 2)])  # merged size n_old + 1 against 3 * 1 + 4096
        assert flat == [v for p in pairs for v in p]
