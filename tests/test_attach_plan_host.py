"""Host side of the attachments (`ipcgpu_set_attachments`): `ipc_amd/csrc/attach_plan.cpp` run as a stand-alone program (`tests/attach_plan/main.cpp`) and
compared with the Python restatement of its merge (tests/attach_mp.py); the same program once more under the address and undefined-behaviour sanitizers.
No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import attach_mp as amp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "attach_plan", "main.cpp"), os.path.join(CSRC, "attach_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "attach_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "attach_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, sets):
    """sets: [case dict of attach_mp (x, nA, wA, nB, wB, k, L)] -> per set the reason of the rejection (str) or a dict"""
    text = []
    for c in sets:
        x = np.asarray(c["x"], dtype=np.float64).reshape(-1, 3)
        n = len(c["k"])
        nums = [repr(float(v)) for v in x.ravel()]
        for i in range(n):
            nums += ([str(int(v)) for v in c["nA"][i]] + [repr(float(v)) for v in c["wA"][i]] + [str(int(v)) for v in c["nB"][i]]
                     + [repr(float(v)) for v in c["wB"][i]] + [repr(float(c["k"][i])), repr(float(c["L"][i]))])
        text.append(f"{len(x)} {n} " + " ".join(nums))
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
        n, nP = int(a[1]), int(a[2])
        pos = [3]

        def take(m, dtype=np.float64):
            v = np.array(a[pos[0]:pos[0] + m], dtype=dtype)
            pos[0] += m
            return v
        d = {"count": take(n, np.int64), "node": take(6 * n, np.int64).reshape(6, n).T, "coef": take(6 * n).reshape(6, n).T, "k": take(n), "L": take(n),
             "restDist": take(n), "pairs": take(2 * nP, np.int64).reshape(-1, 2)}
        assert pos[0] == len(a)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("attach_plan_main", [])
    return lambda sets: _run(exe, sets)


def good_sets():
    G = {c["name"]: c for c in amp.cases()}
    # every stored case in one set, node ranges side by side
    off, parts = 0, {k: [] for k in ("x", "nA", "wA", "nB", "wB", "k", "L")}
    for c in amp.cases():
        parts["x"].append(c["x"])
        for k in ("nA", "nB"):
            parts[k].append(np.where(c[k] >= 0, c[k] + off, -1))
        for k in ("wA", "wB", "k", "L"):
            parts[k].append(c[k])
        off += len(c["x"])
    G["all cases side by side"] = {k: np.concatenate(v) for k, v in parts.items()}
    pt = amp._pt
    G["a node twice in one point, a gap in the slots"] = amp._case("", np.eye(3), [(([1, 1, -1], [0.5, 0.5, 0.0]), ([-1, 2, -1], [0.0, 1.0, 0.0]), 10.0, 0.5)])
    G["the same pair twice, reversed"] = amp._case("", np.eye(3), [(pt((0, 1)), pt((2, 1)), 1.0, 0.0), (pt((2, 1)), pt((0, 1)), 2.0, 0.25)])
    G["no attachment"] = amp._case("", np.eye(3), [])
    for c in G.values():
        for k in ("nA", "nB"):
            c[k] = np.asarray(c[k]).reshape(-1, 3)
        for k in ("wA", "wB"):
            c[k] = np.asarray(c[k], dtype=np.float64).reshape(-1, 3)
    return G


def check(c, got):
    assert isinstance(got, dict), got
    n = len(c["k"])
    want = amp.stencils(c)
    pairs = set()
    for i, (ids, coef) in enumerate(want):
        m = len(ids)
        assert 2 <= m <= 6 and got["count"][i] == m
        assert got["node"][i, :m].tolist() == ids and got["coef"][i, :m].tolist() == coef  # merged, in the order of first appearance, to the bit
        assert np.all(got["node"][i, m:] == ids[0]) and np.all(got["coef"][i, m:] == 0.0)  # padding: the first node, coefficient 0
        assert len(set(ids)) == m and abs(sum(coef)) <= 4e-12
        pairs |= {(min(a, b), max(a, b)) for a in ids for b in ids if a != b}
        d = (np.asarray(coef)[:, None] * np.asarray(c["x"], dtype=np.float64).reshape(-1, 3)[ids]).sum(axis=0)
        assert abs(got["restDist"][i] - np.linalg.norm(d)) <= 1e-14 * (1 + np.abs(c["x"]).max())
    assert got["pairs"].tolist() == [list(p) for p in sorted(pairs)]  # sorted, unique, lo < hi
    assert np.array_equal(got["k"], c["k"]) and np.array_equal(got["L"], c["L"]) and len(got["count"]) == n


def test_plans_match_the_python_merge(planner):
    G = good_sets()
    res = planner(list(G.values()))
    for (name, c), got in zip(G.items(), res):
        check(c, got)
    by = dict(zip(G, res))
    assert by["one node in both points"]["count"].tolist() == [3] and by["one node in both points"]["coef"][0].tolist() == [0.5, 0.25, -0.75, 0.0, 0.0, 0.0]
    assert by["triangle point - triangle point"]["count"].tolist() == [6] and len(by["triangle point - triangle point"]["pairs"]) == 15
    assert by["node ids descending"]["node"][0, :3].tolist() == [3, 2, 0]
    twice = by["a node twice in one point, a gap in the slots"]
    assert twice["count"].tolist() == [2] and twice["node"][0].tolist() == [1, 2, 1, 1, 1, 1] and twice["coef"][0, :2].tolist() == [1.0, -1.0]
    assert by["the same pair twice, reversed"]["pairs"].tolist() == [[0, 2]]
    assert abs(by["node - node, stretched"]["restDist"][0] - 0.15) <= 1e-15
    assert len(by["no attachment"]["count"]) == 0 and len(by["no attachment"]["pairs"]) == 0
    assert len(by["all cases side by side"]["count"]) == sum(len(c["k"]) for c in amp.cases())


def bad_sets():
    pt = amp._pt
    X = np.eye(4)[:, :3]
    one = lambda A, B, k=10.0, L=0.0: amp._case("", X, [(pt((0, 1)), pt((1, 1)), 5.0, 0.1), (A, B, k, L)])
    nan, inf = float("nan"), float("inf")
    return {"out of range": one(pt((0, 1)), pt((4, 1))), "out of range, negative": one(pt((-2, 1)), pt((1, 1))),
            "has no node": one(([-1, -1, -1], [0.0, 0.0, 0.0]), pt((1, 1))), "negative weight": one(pt((0, 1.5), (1, -0.5)), pt((2, 1))),
            "not finite": one(pt((0, nan)), pt((2, 1))), "not finite, inf": one(pt((0, 1)), pt((2, inf))),
            "unused slot": one(([0, -1, -1], [0.5, 0.5, 0.0]), pt((2, 1))),
            "do not sum to 1": one(pt((0, 0.5), (1, 0.4)), pt((2, 1))), "do not sum to 1, by 1e-11": one(pt((0, 0.5), (1, 0.5 + 1e-11)), pt((2, 1))),
            "k > 0": one(pt((0, 1)), pt((2, 1)), k=0.0), "k > 0, negative": one(pt((0, 1)), pt((2, 1)), k=-1.0), "k > 0, nan": one(pt((0, 1)), pt((2, 1)), k=nan),
            "k > 0, inf": one(pt((0, 1)), pt((2, 1)), k=inf), "L >= 0": one(pt((0, 1)), pt((2, 1)), L=-0.1), "L >= 0, nan": one(pt((0, 1)), pt((2, 1)), L=nan),
            "L >= 0, inf": one(pt((0, 1)), pt((2, 1)), L=inf),
            "same point": one(pt((3, 1)), pt((3, 1))), "same point, an edge point": one(pt((2, 0.5), (3, 0.5)), pt((3, 0.5), (2, 0.5)))}


def test_rejections(planner):
    B = bad_sets()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        assert name.split(",")[0] in got and "attachment 1" in got, (name, got)


def test_weights_within_the_sum_tolerance_are_accepted(planner):
    pt = amp._pt
    c = amp._case("", np.eye(3), [(pt((0, 0.5), (1, 0.5 + 5e-13)), pt((2, 1)), 1.0, 0.0)])
    assert isinstance(planner([c])[0], dict)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("attach_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_sets(), bad_sets()
    res = _run(exe, list(G.values()) + list(B.values()))
    for c, got in zip(G.values(), res):
        check(c, got)
    assert all(isinstance(r, str) for r in res[len(G):])
