"""Host side of the pressure chambers (`ipcgpu_set_chambers`): `ipc_amd/csrc/chamber_plan.cpp` run as a stand-alone program
(`tests/chamber_plan/main.cpp`) and compared with the Python restatement of its sums (tests/chamber_mp.py); the same program once more under the address
and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import chamber_mp as cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "chamber_plan", "main.cpp"), os.path.join(CSRC, "chamber_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "chamber_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "chamber_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _set(x, tris, p, triEnd=None):
    """x: nV x 3; tris: one m x 3 list per chamber; p: one pressure per chamber; triEnd: given instead of the cumulative sizes (for the rejections)"""
    tris = [np.asarray(t, dtype=np.int64).reshape(-1, 3) for t in tris]
    return {"x": np.asarray(x, dtype=np.float64).reshape(-1, 3), "tris": tris, "p": [float(v) for v in p],
            "triEnd": [int(v) for v in (np.cumsum([len(t) for t in tris]) if triEnd is None else triEnd)]}


def _run(exe, sets):
    text = []
    for c in sets:
        nums = [repr(float(v)) for v in c["x"].ravel()] + [str(v) for v in c["triEnd"]]
        nums += [str(int(v)) for t in c["tris"] for v in t.ravel()] + [repr(v) for v in c["p"]]
        text.append(f"{len(c['x'])} {len(c['p'])} {sum(len(t) for t in c['tris'])} " + " ".join(nums))
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
        d = {"triEnd": take(n, np.int64), "tri": take(3 * nTri, np.int64).reshape(3, nTri).T, "chamberOf": take(nTri, np.int64), "p": take(n),
             "restVolume": take(n), "restRef": take(3 * n).reshape(n, 3), "pairs": take(2 * nP, np.int64).reshape(-1, 2)}
        assert pos[0] == len(a)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("chamber_plan_main", [])
    return lambda sets: _run(exe, sets)


def good_sets():
    G = {}
    cs = cm.cases()
    for c in cs:
        G[c["name"]] = _set(c["x"], [c["tri"]], [c["p"]])
    off = np.concatenate([[0], np.cumsum([len(c["x"]) for c in cs])])
    G["all cases side by side"] = _set(np.vstack([c["x"] for c in cs]), [c["tri"] + o for c, o in zip(cs, off)], [c["p"] for c in cs])
    G["two chambers of different sizes"] = _set(np.vstack([cm.CUBE_X, cm.TET_X + 3.0]), [cm.CUBE_TRI, cm.TET_TRI + 8], [2.0, -1.0])
    G["a tiny chamber first, descending node ids"] = _set(np.vstack([cm.CUBE_X, cm.TET_X + 3.0]), [(cm.TET_TRI + 8)[::-1], cm.CUBE_TRI[::-1]], [0.0, 5.0])
    G["one surface in two chambers"] = _set(cm.CUBE_X, [cm.CUBE_TRI, cm.CUBE_TRI], [1.0, 2.0])
    G["no chamber"] = _set(cm.CUBE_X, [], [])
    return G


def check(c, got):
    assert isinstance(got, dict), got
    n = len(c["p"])
    assert got["triEnd"].tolist() == c["triEnd"] and np.array_equal(got["p"], c["p"])
    tri = np.vstack(c["tris"]) if n else np.zeros((0, 3), dtype=np.int64)
    assert np.array_equal(got["tri"], tri)  # as given: order and orientation
    assert got["chamberOf"].tolist() == [i for i, t in enumerate(c["tris"]) for _ in range(len(t))]
    pairs = {(min(a, b), max(a, b)) for t in tri for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert got["pairs"].tolist() == [list(p) for p in sorted(pairs)]  # sorted, unique, lo < hi: the three edges of every triangle
    for i, t in enumerate(c["tris"]):
        r = cm.ref_point(c["x"], t)
        assert np.array_equal(got["restRef"][i], r)  # the documented order, to the bit
        assert got["restVolume"][i] == cm.rest_volume(c["x"], t, r) and got["restVolume"][i] > 0
        assert np.abs(r - c["x"][np.unique(t)].mean(axis=0)).max() <= 0.5 * np.ptp(c["x"][np.unique(t)], axis=0).max()


def test_plans_match_the_python_restatement(planner):
    G = good_sets()
    res = planner(list(G.values()))
    for (name, c), got in zip(G.items(), res):
        check(c, got)
    by = dict(zip(G, res))
    two = by["two chambers of different sizes"]
    assert two["triEnd"].tolist() == [12, 16] and two["restVolume"].tolist() == [1.0, cm.rest_volume(cm.TET_X + 3.0, cm.TET_TRI, cm.ref_point(cm.TET_X + 3.0, cm.TET_TRI))]
    assert abs(two["restVolume"][1] - 1 / 6) <= 1e-15 and np.array_equal(two["restRef"][0], [0.5, 0.5, 0.5])
    assert len(two["pairs"]) == 18 + 6  # a cube's 12 edges and 6 face diagonals, a tetrahedron's 6 edges
    assert by["a tiny chamber first, descending node ids"]["triEnd"].tolist() == [4, 16]
    assert len(by["one surface in two chambers"]["pairs"]) == 18 and by["one surface in two chambers"]["chamberOf"].tolist() == [0] * 12 + [1] * 12
    assert len(by["no chamber"]["triEnd"]) == 0 and len(by["no chamber"]["pairs"]) == 0
    assert len(by["all cases side by side"]["triEnd"]) == len(cm.cases())
    assert by["two cubes in one chamber"]["triEnd"].tolist() == [24]


def bad_sets():
    """every set has a good chamber 0 (a tetrahedron) and a bad chamber 1 (from a cube)"""
    X = np.vstack([cm.TET_X + 3.0, cm.CUBE_X])
    T0, C = cm.TET_TRI, cm.CUBE_TRI + 4
    one = lambda tri, p=1.0, **kw: _set(X, [T0, tri], [1.0, p], **kw)
    nan, inf = float("nan"), float("inf")
    swapped = C.copy()
    swapped[-1] = swapped[-1][::-1]
    last = lambda v: np.vstack([C[:-1], [[C[-1][0], C[-1][1], v]]])
    return {"out of range": one(last(12)), "out of range, negative": one(last(-1)),
            "repeats a node": one(np.vstack([C[:-1], [[5, 5, 9]]])),
            "not by two": one(C[:-1]), "not by two, three times": one(np.vstack([C, C[:1]])), "not by two, a lone triangle": one(C[:1]),
            "same direction": one(swapped),
            "is empty": one(np.zeros((0, 3))), "not ascending": one(C, triEnd=[4, 2]), "not ascending, negative": _set(X, [T0], [1.0], triEnd=[-1]),
            "not finite": one(C, p=nan), "not finite, inf": one(C, p=inf), "not finite, -inf": one(C, p=-inf),
            "oriented inward": one(C[:, ::-1])}


def test_rejections(planner):
    B = bad_sets()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        assert name.split(",")[0] in got, (name, got)
        assert ("chamber 0" if "negative" in name and "ascending" in name else "chamber 1") in got, (name, got)
    by = dict(zip(B, planner(list(B.values()))))
    assert "triangle 15" in by["out of range"] and "triangle 15" in by["repeats a node"]  # chamber 1's last triangle, counted over the whole list
    assert "edge (" in by["not by two"] and "used by 1" in by["not by two"] and "used by 3" in by["not by two, three times"]
    assert "triangles" in by["same direction"] and "edge (" in by["same direction"]


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("chamber_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_sets(), bad_sets()
    res = _run(exe, list(G.values()) + list(B.values()))
    for c, got in zip(G.values(), res):
        check(c, got)
    assert all(isinstance(r, str) for r in res[len(G):])
