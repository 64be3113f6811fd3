"""Host side of the nodal stress pass (`ipcgpu_elastic_stress`): the node -> element incidence list of `ipc_amd/csrc/stress_plan.cpp`, run as a stand-alone
program (`tests/stress_plan/main.cpp`) and compared with a NumPy construction; the same program once more under the address and undefined-behaviour
sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import elastic_mp as emp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "stress_plan", "main.cpp"), os.path.join(CSRC, "stress_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "stress_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "stress_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, meshes):
    """meshes: [(nV, F[nT, 4])] -> per mesh None (rejected) or (ptr[nV + 1], elems[4 nT])"""
    text = "".join(f"{nV} {len(F)} {' '.join(str(int(x)) for x in np.asarray(F, dtype=np.int64).reshape(-1, 4).T.ravel())}\n" for nV, F in meshes)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(meshes)
    res = []
    for line, (nV, F) in zip(out, meshes):
        a = np.array(line.split(), dtype=np.int64)
        if a[0] == 0:
            res.append(None)
            continue
        assert len(a) == 1 + nV + 1 + 4 * len(F)
        res.append((a[1:nV + 2], a[nV + 2:]))
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("stress_plan_main", [])
    return lambda meshes: _run(exe, meshes)


def incidence_numpy(nV, F):
    F = np.asarray(F, dtype=np.int64).reshape(-1, 4)
    rows = [np.sort(np.repeat(np.arange(len(F)), 4)[F.ravel() == v]) for v in range(nV)]  # a node counted once per slot it fills
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int64)


def meshes():
    Vb, Fb, _ = emp.block_mesh()
    nb = Vb.shape[0]
    rng = np.random.default_rng(11)
    hub = np.array([[k, k + 1, k + 2, 40] for k in range(0, 36, 3)] + [[0, 5, 9, 40], [1, 2, 3, 4]])  # node 40, the last one, is in 13 of 14 elements
    return {"single tet": (4, np.array([[0, 1, 2, 3]])),
            "single tet, reversed ids": (4, np.array([[3, 1, 2, 0]])),
            "block_mesh": (nb, Fb),
            "block_mesh + 300 isolated nodes": (nb + 300, Fb),
            "isolated nodes first and between": (12, np.array([[3, 5, 7, 9], [9, 7, 5, 4]])),
            "last node has the most neighbours": (41, hub),
            "random, unsorted": (50, np.array([rng.permutation(50)[:4] for _ in range(257)])),
            "no element": (5, np.zeros((0, 4), dtype=np.int64))}


def check(nV, F, got):
    assert got is not None
    ptr, elems = got
    want_ptr, want_elems = incidence_numpy(nV, F)
    assert ptr[0] == 0 and ptr[nV] == 4 * len(F)
    assert np.array_equal(ptr, want_ptr) and np.array_equal(elems, want_elems)
    for v in range(nV):
        row = elems[ptr[v]:ptr[v + 1]]
        assert np.all(np.diff(row) > 0)  # ascending: the order the kernel sums in
        assert all(v in F[e] for e in row)


def test_incidence_list_matches_numpy(planner):
    M = meshes()
    for (name, (nV, F)), got in zip(M.items(), planner(list(M.values()))):
        check(nV, np.asarray(F).reshape(-1, 4), got)
    nV, F = M["last node has the most neighbours"]
    ptr, _ = planner([(nV, F)])[0]
    assert np.argmax(np.diff(ptr)) == nV - 1 and np.diff(ptr)[-1] == 13
    nV, F = M["block_mesh + 300 isolated nodes"]
    ptr, _ = planner([(nV, F)])[0]
    assert np.all(ptr[-301:] == 4 * len(F))  # empty rows at the end


def test_out_of_range_tables_are_rejected(planner):
    bad = [(4, np.array([[0, 1, 2, 4]])), (4, np.array([[0, -1, 2, 3]])), (0, np.array([[0, 0, 0, 0]]))]
    assert planner(bad) == [None] * len(bad)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("stress_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    M = meshes()
    res = _run(exe, list(M.values()) + [(4, np.array([[0, 1, 2, 4]]))])
    assert res[-1] is None
    for (nV, F), got in zip(M.values(), res):
        check(nV, np.asarray(F).reshape(-1, 4), got)
