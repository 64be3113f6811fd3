"""Host side of the elastic shells (`ipcgpu_set_shell`): `ipc_amd/csrc/shell_plan.cpp` run as a stand-alone program (`tests/shell_plan/main.cpp`) and compared
with NumPy constructions; the same program once more under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import shell_mp as smp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "shell_plan", "main.cpp"), os.path.join(CSRC, "shell_plan.cpp")]
MAT = (0.01, 1e5, 0.3, 1000.0)


def _build(name, extra):
    exe = os.path.join(HERE, "shell_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "shell_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, meshes):
    """meshes: [(V[nV, 3], tri[nTri, 3], mat[nTri, 4] or None, tets[nTet, 4] or None)] -> per mesh the reason of the rejection (str) or a dict"""
    text = []
    for V, tri, mat, tets in meshes:
        V, tri = np.asarray(V, dtype=np.float64).reshape(-1, 3), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
        mat = np.tile(MAT, (len(tri), 1)) if mat is None else np.asarray(mat, dtype=np.float64)
        tets = np.zeros((0, 4), dtype=np.int64) if tets is None else np.asarray(tets, dtype=np.int64)
        nums = [repr(float(v)) for v in V.ravel()] + [str(int(v)) for v in tri.ravel()] + [repr(float(v)) for v in mat.ravel()] + [str(int(v)) for v in tets.ravel()]
        text.append(f"{len(V)} {len(tri)} {len(tets)} " + " ".join(nums))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(meshes)
    res = []
    for line, (V, tri, _, _) in zip(out, meshes):
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        nV, nTri, nH, nP = len(np.asarray(V).reshape(-1, 3)), len(np.asarray(tri).reshape(-1, 3)), int(a[1]), int(a[2])
        pos = [3]

        def take(n, dtype=np.float64):
            v = np.array(a[pos[0]:pos[0] + n], dtype=dtype)
            pos[0] += n
            return v
        d = {"hinges": take(4 * nH, np.int64).reshape(-1, 4), "restAngle": take(nH), "weight": take(nH), "kb": take(nH), "area": take(nTri),
             "const": take(6 * nTri).reshape(-1, 6), "mass": take(nV), "pairs": take(2 * nP, np.int64).reshape(-1, 2), "edgeLenSum": take(1)[0]}
        assert pos[0] == len(a)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("shell_plan_main", [])
    return lambda meshes: _run(exe, meshes)


def folded_strip(deg):
    return smp.hinge_nodes(deg), np.array(smp.HINGE_TRI)


TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
TET_SURFACE = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])  # outward normals


def good_meshes():
    Vg, Tg = smp.grid(5, 4)
    return {"strip": folded_strip(0) + (None, None), "strip folded 60": folded_strip(60) + (None, None), "strip folded -120": folded_strip(-120) + (None, None),
            "grid 5 x 4": (Vg, Tg, None, None), "tetrahedron surface": (TET_V, TET_SURFACE, None, None),
            "grid beside a tetrahedron": (np.vstack([Vg, TET_V + 5.0]), Tg, None, [[20, 21, 22, 23]]),
            "no triangle": (TET_V, np.zeros((0, 3), dtype=np.int64), None, None)}


def check(V, tri, got):
    assert isinstance(got, dict), got
    V, tri = np.asarray(V, dtype=np.float64), np.asarray(tri).reshape(-1, 3)
    want = smp.hinges_of(tri)
    assert np.array_equal(got["hinges"], np.array([w[:4] for w in want], dtype=np.int64).reshape(-1, 4))
    keys = [tuple(h[:2]) for h in got["hinges"].tolist()]
    assert keys == sorted(keys) and all(a < b for a, b in keys)
    # interior edges by a NumPy count: every undirected edge that appears twice
    if len(tri):
        e = np.sort(np.vstack([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
        uniq, cnt = np.unique(e, axis=0, return_counts=True)
        assert len(got["hinges"]) == int(np.sum(cnt == 2)) and np.all(cnt <= 2)
        opp = np.sort(got["hinges"][:, 2:], axis=1)
        pairs = np.unique(np.vstack([uniq, opp]), axis=0)
        assert np.array_equal(got["pairs"], pairs)  # triangle edges and the opposite pairs, sorted, unique
        for row in opp:
            assert any(np.array_equal(row, p) for p in got["pairs"])
    X = V.tolist()
    h, E, nu, rho = MAT
    area = np.array([smp.rest_triangle(smp.NP, [X[v] for v in t])[1] for t in tri])
    assert np.allclose(got["area"], area, rtol=1e-14, atol=0)
    assert abs(got["mass"].sum() - rho * h * area.sum()) <= 1e-13 * rho * h * max(area.sum(), 1e-300)
    mass = np.zeros(len(V))
    for t, a in zip(tri, area):
        mass[t] += rho * h * a / 3
    assert np.allclose(got["mass"], mass, rtol=1e-13, atol=0)
    for t, c in zip(tri, got["const"]):
        B, A = smp.rest_triangle(smp.NP, [X[v] for v in t])
        mu, lam = smp.lame(E, nu)
        assert np.allclose(c, [B[0][0], B[1][0], B[0][1], B[1][1], h * A * mu, h * A * lam], rtol=1e-13, atol=1e-18)
    for hg, th, w, kb in zip(want, got["restAngle"], got["weight"], got["kb"]):
        t0, w0, k0 = smp.hinge_constants(smp.NP, [X[v] for v in hg[:4]], [(h, E, nu)] * 2)
        assert abs(th - t0) <= 1e-14 and abs(w - w0) <= 1e-13 * w0 and abs(kb - k0) <= 1e-13 * k0


def test_plans_match_numpy(planner):
    G = good_meshes()
    res = planner(list(G.values()))
    for (name, (V, tri, _, _)), got in zip(G.items(), res):
        check(V, tri, got)
    by = dict(zip(G, res))
    assert len(by["strip"]["hinges"]) == 1 and by["strip"]["hinges"][0].tolist() == [0, 1, 2, 3] and [2, 3] in by["strip"]["pairs"].tolist()
    assert abs(by["strip"]["restAngle"][0]) <= 1e-15
    assert abs(by["strip folded 60"]["restAngle"][0] - np.radians(60)) <= 1e-14 and abs(by["strip folded -120"]["restAngle"][0] + np.radians(120)) <= 1e-14
    n, m = 5, 4
    assert len(by["grid 5 x 4"]["hinges"]) == (n - 1) * m + n * (m - 1) + (n - 1) * (m - 1) - 2 * ((n - 1) + (m - 1))  # all edges minus the boundary
    assert np.all(np.abs(by["grid 5 x 4"]["restAngle"]) <= 1e-15)
    tet = by["tetrahedron surface"]
    assert len(tet["hinges"]) == 6 and len(tet["pairs"]) == 6  # closed: every edge a hinge, every opposite pair an edge
    assert np.all(tet["restAngle"] * tet["restAngle"][0] > 0)  # a convex closed surface folds the same way at every edge
    assert by["no triangle"]["mass"].tolist() == [0.0] * 4 and len(by["no triangle"]["hinges"]) == 0


def bad_meshes():
    Vg, Tg = smp.grid(3)
    fan = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1.0]])
    bad_mat = np.tile(MAT, (len(Tg), 1))
    bad_mat[3, 0] = 0.0
    return {"out of range": (Vg, np.vstack([Tg, [[0, 1, 9]]]), None, None), "negative id": (Vg, np.vstack([Tg, [[0, -1, 2]]]), None, None),
            "repeats a node": (Vg, np.vstack([Tg, [[0, 1, 1]]]), None, None), "zero rest area": (np.vstack([Vg, [[0.05, 0.0, 0.0]]]), [[0, 9, 1]], None, None),
            "more than two triangles": (fan, [[0, 1, 2], [1, 0, 3], [0, 1, 4]], None, None),
            "same direction": (smp.hinge_nodes(0), [[0, 1, 2], [0, 1, 3]], None, None),
            "belongs to a tetrahedron": (np.vstack([Vg, TET_V + 5.0]), Tg, None, [[9, 10, 11, 4]]),
            "thickness": (Vg, Tg, bad_mat, None)}


def test_rejections(planner):
    B = bad_meshes()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        key = {"negative id": "out of range", "thickness": "thickness"}.get(name, name)
        assert key in got, (name, got)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("shell_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_meshes(), bad_meshes()
    res = _run(exe, list(G.values()) + list(B.values()))
    for (V, tri, _, _), got in zip(G.values(), res):
        check(V, tri, got)
    assert all(isinstance(r, str) for r in res[len(G):])
