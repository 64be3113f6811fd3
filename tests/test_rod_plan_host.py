"""Host side of the elastic rods (`ipcgpu_set_rod`): `ipc_amd/csrc/rod_plan.cpp` run as a stand-alone program (`tests/rod_plan/main.cpp`) and compared with
NumPy constructions; the same program once more under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import rod_mp as rmp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "rod_plan", "main.cpp"), os.path.join(CSRC, "rod_plan.cpp")]
MAT = (0.002, 1e7, 1000.0)


def _build(name, extra):
    exe = os.path.join(HERE, "rod_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "rod_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _mat(seg, mat):
    return np.tile(MAT, (len(seg), 1)) if mat is None else np.asarray(mat, dtype=np.float64)


def _run(exe, meshes):
    """meshes: [(V[nV, 3], seg[nSeg, 2], mat[nSeg, 3] or None, tets or None, shell triangles or None)] -> per mesh the reason of the rejection (str) or a dict"""
    text = []
    for V, seg, mat, tets, tris in meshes:
        V, seg = np.asarray(V, dtype=np.float64).reshape(-1, 3), np.asarray(seg, dtype=np.int64).reshape(-1, 2)
        tets = np.zeros((0, 4), dtype=np.int64) if tets is None else np.asarray(tets, dtype=np.int64)
        tris = np.zeros((0, 3), dtype=np.int64) if tris is None else np.asarray(tris, dtype=np.int64)
        nums = ([repr(float(v)) for v in V.ravel()] + [str(int(v)) for v in seg.ravel()] + [repr(float(v)) for v in _mat(seg, mat).ravel()]
                + [str(int(v)) for v in tets.ravel()] + [str(int(v)) for v in tris.ravel()])
        text.append(f"{len(V)} {len(seg)} {len(tets)} {len(tris)} " + " ".join(nums))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(meshes)
    res = []
    for line, (V, seg, *_rest) in zip(out, meshes):
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        nV, nSeg, nB, nP = len(np.asarray(V).reshape(-1, 3)), len(np.asarray(seg).reshape(-1, 2)), int(a[1]), int(a[2])
        pos = [3]

        def take(n, dtype=np.float64):
            v = np.array(a[pos[0]:pos[0] + n], dtype=dtype)
            pos[0] += n
            return v
        d = {"bend": take(3 * nB, np.int64).reshape(-1, 3), "kb": take(nB), "restKb": take(nB), "L": take(nSeg), "ks": take(nSeg), "mass": take(nV),
             "isRodNode": take(nV, np.int64), "pairs": take(2 * nP, np.int64).reshape(-1, 2), "lenSum": take(1)[0]}
        assert pos[0] == len(a)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("rod_plan_main", [])
    return lambda meshes: _run(exe, meshes)


TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])


def good_meshes():
    by = {c["name"]: c for c in rmp.cases()}
    G = {}
    for name in ("segment at rest", "three nodes at 0", "five-node polyline, Dirichlet nodes", "three-armed junction", "closed six-node ring"):
        c = by[name]
        G[name] = (c["X"], c["seg"], np.column_stack([c["r"], c["YM"], c["rho"]]), None, None)
    Vc, seg = rmp.chain(7, axis=(0.0, -1.0, 0.0))
    G["chain given backwards and shuffled"] = (Vc, seg[[3, 0, 5, 1, 4, 2]][:, ::-1], None, None, None)
    G["curved rest polyline"] = (rmp.elbow(60), [[0, 1], [1, 2]], None, None, None)
    G["chain beside a tetrahedron and a shell triangle"] = (np.vstack([Vc, TET_V + 5.0, TET_V[:3] - 5.0]), seg, None, [[7, 8, 9, 10]], [[11, 12, 13]])
    G["no segment"] = (TET_V, np.zeros((0, 2), dtype=np.int64), None, None, None)
    return G


def check(V, seg, mat, got):
    assert isinstance(got, dict), got
    V, seg = np.asarray(V, dtype=np.float64).reshape(-1, 3), np.asarray(seg).reshape(-1, 2)
    r, E, rho = _mat(seg, mat).T if len(seg) else (np.zeros(0),) * 3
    want = rmp.triples_of(seg, len(V))
    assert np.array_equal(got["bend"], np.array([w[:3] for w in want], dtype=np.int64).reshape(-1, 3))
    assert got["bend"][:, 1].tolist() == sorted(got["bend"][:, 1].tolist())  # ascending by the interior node
    # interior nodes by a NumPy count: every node that appears exactly twice
    deg = np.bincount(seg.ravel(), minlength=len(V)) if len(seg) else np.zeros(len(V), dtype=int)
    assert got["bend"][:, 1].tolist() == np.flatnonzero(deg == 2).tolist()
    assert np.array_equal(got["isRodNode"], (deg > 0).astype(np.int64))
    if len(seg):
        outer = np.sort(got["bend"][:, [0, 2]], axis=1)
        pairs = np.unique(np.vstack([np.sort(seg, axis=1), outer]), axis=0)
        assert np.array_equal(got["pairs"], pairs)  # segments and the outer pairs, sorted, unique
    else:
        assert len(got["pairs"]) == 0
    L = np.linalg.norm(V[seg[:, 1]] - V[seg[:, 0]], axis=1)
    assert np.allclose(got["L"], L, rtol=1e-15, atol=0) and abs(got["lenSum"] - L.sum()) <= 1e-14 * max(L.sum(), 1e-300)
    assert np.allclose(got["ks"], E * np.pi * r * r / L, rtol=1e-14, atol=0)
    mass = np.zeros(len(V))
    for k in range(2):
        np.add.at(mass, seg[:, k], rho * np.pi * r * r * L / 2)
    assert np.allclose(got["mass"], mass, rtol=1e-13, atol=0)
    assert abs(got["mass"].sum() - (rho * np.pi * r * r * L).sum()) <= 1e-13 * max(mass.sum(), 1e-300)
    X = V.tolist()
    for (a, b, c, s0, s1), kb, rest in zip(want, got["kb"], got["restKb"]):
        k0 = rmp.bend_stiffness(rmp.NP, [X[a], X[b], X[c]], ((r[s0], E[s0]), (r[s1], E[s1])))
        k2 = rmp.curvature(rmp.NP, [X[a], X[b], X[c]])[0]
        assert abs(kb - k0) <= 1e-13 * k0 and abs(rest - np.sqrt(k2)) <= 1e-14 * (1 + np.sqrt(k2))


def test_plans_match_numpy(planner):
    G = good_meshes()
    res = planner(list(G.values()))
    for (name, (V, seg, mat, _, _)), got in zip(G.items(), res):
        check(V, seg, mat, got)
    by = dict(zip(G, res))
    assert len(by["segment at rest"]["bend"]) == 0 and by["segment at rest"]["pairs"].tolist() == [[0, 1]]
    assert by["three nodes at 0"]["bend"].tolist() == [[0, 1, 2]] and [0, 2] in by["three nodes at 0"]["pairs"].tolist()
    assert 0.0 <= by["three nodes at 0"]["restKb"][0] <= 1e-7  # straight at rest (sqrt of a rounding of |e0||e1| - e0 . e1; never NaN)
    assert by["three-armed junction"]["bend"].tolist() == [[0, 1, 4]]  # the hub has three segments: no bending there
    assert by["closed six-node ring"]["bend"][:, 1].tolist() == list(range(6))
    assert np.allclose(by["closed six-node ring"]["restKb"], 2 * np.tan(np.radians(60) / 2), rtol=1e-14)
    assert abs(by["curved rest polyline"]["restKb"][0] - 2 * np.tan(np.radians(30))) <= 1e-14
    shuffled = by["chain given backwards and shuffled"]
    assert shuffled["bend"][:, 1].tolist() == [1, 2, 3, 4, 5] and len(shuffled["pairs"]) == 6 + 5
    assert by["no segment"]["mass"].tolist() == [0.0] * 4 and len(by["no segment"]["bend"]) == 0


def bad_meshes():
    Vc, seg = rmp.chain(4)
    def mat(col, val):
        m = np.tile(MAT, (len(seg), 1))
        m[1, col] = val
        return m
    return {"out of range": (Vc, np.vstack([seg, [[0, 4]]]), None, None, None), "negative id": (Vc, np.vstack([seg, [[-1, 2]]]), None, None, None),
            "repeats a node": (Vc, np.vstack([seg, [[2, 2]]]), None, None, None), "is repeated": (Vc, np.vstack([seg, [[1, 2]]]), None, None, None),
            "is repeated, reversed": (Vc, np.vstack([seg, [[2, 1]]]), None, None, None),
            "zero rest length": (np.vstack([Vc, Vc[:1]]), np.vstack([seg, [[0, 4]]]), None, None, None),
            "belongs to a tetrahedron": (np.vstack([Vc, TET_V + 5.0]), seg, None, [[4, 5, 6, 2]], None),
            "belongs to a shell triangle": (np.vstack([Vc, TET_V + 5.0]), seg, None, [[4, 5, 6, 7]], [[4, 5, 3]]),
            "radius": (Vc, seg, mat(0, 0.0), None, None), "radius, negative": (Vc, seg, mat(0, -1.0), None, None), "E": (Vc, seg, mat(1, 0.0), None, None),
            "rho": (Vc, seg, mat(2, 0.0), None, None), "rho, nan": (Vc, seg, mat(2, float("nan")), None, None)}


def test_rejections(planner):
    B = bad_meshes()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        key = {"negative id": "out of range", "is repeated, reversed": "is repeated", "radius": "radius > 0", "radius, negative": "radius > 0", "E": "E > 0",
               "rho": "rho > 0", "rho, nan": "rho > 0"}.get(name, name)
        assert key in got, (name, got)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("rod_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_meshes(), bad_meshes()
    res = _run(exe, list(G.values()) + list(B.values()))
    for (V, seg, mat, _, _), got in zip(G.values(), res):
        check(V, seg, mat, got)
    assert all(isinstance(r, str) for r in res[len(G):])
