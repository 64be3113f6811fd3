"""Host side of the aerodynamic surfaces (`ipcgpu_set_aero`): `ipc_amd/csrc/aero_plan.cpp` run as a stand-alone program (`tests/aero_plan/main.cpp`) and
compared with the Python restatement of its records (tests/aero_mp.py), to the bit; every rejection; the neighbour pairs; the same program once more under
the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import aero_mp as am
import chamber_mp as cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "aero_plan", "main.cpp"), os.path.join(CSRC, "aero_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "aero_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "aero_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _set(x, tris, cn, ct, one, triEnd=None):
    """x: nV x 3; tris: one m x 3 list per surface; cn, ct, one: one value per surface; triEnd: given instead of the cumulative sizes (for the rejections)"""
    tris = [np.asarray(t, dtype=np.int64).reshape(-1, 3) for t in tris]
    return {"x": np.asarray(x, dtype=np.float64).reshape(-1, 3), "tris": tris, "cn": [float(v) for v in cn], "ct": [float(v) for v in ct], "one": [int(v) for v in one],
            "triEnd": [int(v) for v in (np.cumsum([len(t) for t in tris]) if triEnd is None else triEnd)]}


def _run(exe, sets):
    text = []
    for c in sets:
        nums = [repr(float(v)) for v in c["x"].ravel()] + [str(v) for v in c["triEnd"]] + [str(int(v)) for t in c["tris"] for v in t.ravel()]
        nums += [repr(v) for v in c["cn"]] + [repr(v) for v in c["ct"]] + [str(v) for v in c["one"]]
        text.append(f"{len(c['x'])} {len(c['cn'])} {sum(len(t) for t in c['tris'])} " + " ".join(nums))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(sets)
    res = []
    for line in out:
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        n, nTri, nP = int(a[1]), int(a[2]), int(a[3])
        pos = [4]

        def take(m, dtype=np.float64):
            v = np.array(a[pos[0]:pos[0] + m], dtype=dtype)
            pos[0] += m
            return v
        d = {"triEnd": take(n, np.int64), "tri": take(3 * nTri, np.int64).reshape(3, nTri).T, "surfOf": take(nTri, np.int64), "coef": take(4 * n).reshape(n, 4),
             "rec": take(8 * nTri).reshape(nTri, 8), "pairs": take(2 * nP, np.int64).reshape(-1, 2)}
        assert pos[0] == len(a)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("aero_plan_main", [])
    return lambda sets: _run(exe, sets)


SHEET_X = np.array([[0.1 * i, 1.0, 0.1 * j] for i in range(3) for j in range(3)])
SHEET_T = np.array([t for i in range(2) for j in range(2) for t in ((3 * i + j, 3 * i + 3 + j, 3 * i + 4 + j), (3 * i + j, 3 * i + 4 + j, 3 * i + 1 + j))])


def good_sets():
    G = {}
    cs = am.cases()
    for c in cs:
        G[c["name"]] = _set(c["X"], [c["tri"]], [c["cn"]], [c["ct"]], [c["one"]])
    off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cs])])
    G["all cases side by side"] = _set(np.vstack([c["X"] for c in cs]), [c["tri"] + o for c, o in zip(cs, off)], [c["cn"] for c in cs], [c["ct"] for c in cs], [c["one"] for c in cs])
    G["an open sheet in two surfaces"] = _set(SHEET_X, [SHEET_T[:3], SHEET_T[3:]], [1.28, 0.0], [0.0, 0.7], [0, 1])
    G["a closed cube, descending order"] = _set(cm.CUBE_X, [cm.CUBE_TRI[::-1]], [0.5], [0.25], [1])
    G["no surface"] = _set(cm.CUBE_X, [], [], [], [])
    return G


def check(c, got):
    assert isinstance(got, dict), got
    n = len(c["cn"])
    assert got["triEnd"].tolist() == c["triEnd"]
    tri = np.vstack(c["tris"]) if n else np.zeros((0, 3), dtype=np.int64)
    assert np.array_equal(got["tri"], tri)  # as given: order and orientation
    assert got["surfOf"].tolist() == [i for i, t in enumerate(c["tris"]) for _ in range(len(t))]
    assert np.array_equal(got["coef"], np.array([[a, b, float(bool(o)), 0.0] for a, b, o in zip(c["cn"], c["ct"], c["one"])]).reshape(n, 4))
    pairs = {(min(a, b), max(a, b)) for t in tri for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert got["pairs"].tolist() == [list(p) for p in sorted(pairs)]  # sorted, unique, lo < hi: the three edges of every triangle
    assert np.array_equal(got["rec"], am.rest_records(c["x"], tri) if n else np.zeros((0, 8)))  # the documented order, to the bit


def test_plans_match_the_python_restatement(planner):
    G = good_sets()
    res = planner(list(G.values()))
    for (name, c), got in zip(G.items(), res):
        check(c, got)
    by = dict(zip(G, res))
    two = by["an open sheet in two surfaces"]
    assert two["triEnd"].tolist() == [3, 8] and len(two["pairs"]) == 16  # 12 grid edges and 4 diagonals
    assert np.all(np.abs(two["rec"][:, 1]) == 1.0) and np.all(two["rec"][:, [0, 2]] == 0.0) and np.all(np.abs(two["rec"][:, 3] - 0.005) < 1e-17)
    assert len(by["a closed cube, descending order"]["pairs"]) == 18 and len(by["no surface"]["triEnd"]) == 0 and len(by["no surface"]["pairs"]) == 0
    assert len(by["all cases side by side"]["triEnd"]) == len(am.cases())
    for c in am.cases():  # the stored lagged records are these records
        assert np.array_equal(by[c["name"]]["rec"], c["lag"])


def bad_sets():
    """every set has a good surface 0 (the first sheet triangles) and a bad surface 1"""
    T0, C = SHEET_T[:2], SHEET_T[2:]
    one = lambda tri, cn=1.0, ct=0.0, **kw: _set(SHEET_X, [T0, tri], [1.0, cn], [0.0, ct], [0, 1], **kw)
    nan, inf = float("nan"), float("inf")
    last = lambda v: np.vstack([C[:-1], [[C[-1][0], C[-1][1], v]]])
    return {"out of range": one(last(9)), "out of range, negative": one(last(-1)),
            "repeats a node": one(np.vstack([C[:-1], [[5, 5, 7]]])),
            "zero rest area": one(np.vstack([C, [[0, 1, 2]]])),  # three nodes on one line
            "listed twice": one(np.vstack([C, C[1:2]])), "listed twice, rotated": one(np.vstack([C, C[1:2, [2, 0, 1]]])), "listed twice, flipped": one(np.vstack([C, C[1:2, ::-1]])),
            "listed twice, in the other surface": one(np.vstack([C, T0[:1, [1, 0, 2]]])),
            "is empty": one(np.zeros((0, 3))), "not ascending": one(C, triEnd=[2, 1]), "not ascending, negative": _set(SHEET_X, [T0], [1.0], [0.0], [0], triEnd=[-1]),
            "negative coefficient": one(C, cn=-0.5), "negative coefficient, ct": one(C, ct=-1e-300),
            "not finite": one(C, cn=nan), "not finite, inf": one(C, ct=inf), "not finite, -inf": one(C, cn=-inf)}


def test_rejections(planner):
    B = bad_sets()
    by = dict(zip(B, planner(list(B.values()))))
    for name, got in by.items():
        assert isinstance(got, str), name
        assert name.split(",")[0] in got, (name, got)
        assert ("surface 0" if "negative" in name and "ascending" in name else "surface 1") in got, (name, got)
    assert "triangle 7" in by["out of range"] and "triangle 7" in by["repeats a node"]  # surface 1's last triangle, counted over the whole list
    assert "triangle 8" in by["zero rest area"] and "triangle 8" in by["listed twice, flipped"] and "triangle 3" in by["listed twice, flipped"]
    assert "triangle 0" in by["listed twice, in the other surface"]


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("aero_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_sets(), bad_sets()
    res = _run(exe, list(G.values()) + list(B.values()))
    for c, got in zip(G.values(), res):
        check(c, got)
    assert all(isinstance(r, str) for r in res[len(G):])
