"""Host side of the shells' woven cloth (`ipcgpu_shell_set_weave`): `ipc_amd/csrc/shell_weave_plan.cpp` run as a stand-alone program
(`tests/shell_weave_plan/main.cpp`, over the shell plan of a small tilted sheet) and compared with NumPy constructions; the same program once more under the
address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import shell_mp as smp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "shell_weave_plan", "main.cpp"), os.path.join(CSRC, "shell_weave_plan.cpp"), os.path.join(CSRC, "shell_plan.cpp")]

R = smp.rot([1, 2, 3], 50)  # the sheet lies in no coordinate plane
V0, TRI = smp.grid(3)  # 3 x 3 nodes, 8 triangles, 8 interior edges: 2 along x, 2 along y, 4 diagonal
V = V0 @ R.T + [0.3, -0.2, 0.1]
NT = len(TRI)
H = np.linspace(0.01, 0.02, NT)
EX, EY, NORMAL = R @ [1.0, 0.0, 0.0], R @ [0.0, 1.0, 0.0], R @ [0.0, 0.0, 1.0]
FAB = {"E1": 1e5, "E2": 5e4, "G12": 2e3}


def _build(name, extra):
    exe = os.path.join(HERE, "shell_weave_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "shell_weave_plan.h"), os.path.join(CSRC, "shell_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def req(woven=1, d=None, nu12=None, bend_warp=None, bend_weft=None, bend_scale=1.0, **fab):
    """one request over the sheet: scalars are broadcast over the triangles"""
    per = lambda v: None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (NT,)).copy()
    f = dict(FAB, **fab)
    return {"woven": per(woven), "dir": np.broadcast_to(np.asarray(EX if d is None else d, dtype=np.float64), (NT, 3)).copy(), "E1": per(f["E1"]), "E2": per(f["E2"]),
            "G12": per(f["G12"]), "nu12": per(nu12), "bw": per(bend_warp), "bf": per(bend_weft), "bendScale": bend_scale}


def _run(exe, requests):
    text = []
    for q in requests:
        opt = [q[k] for k in ("woven",)] + [q["dir"].ravel(), q["E1"], q["E2"], q["G12"]] + [q[k] for k in ("nu12", "bw", "bf")]
        vals = [V.ravel(order="F"), TRI.ravel(order="F").astype(np.float64), H] + [a for a in opt if a is not None]
        head = f"{len(V)} {NT} {int(q['woven'] is not None)} {int(q['nu12'] is not None)} {int(q['bw'] is not None)} {int(q['bf'] is not None)} {q['bendScale']!r}"
        text.append(head + " " + " ".join(repr(float(v)) for a in vals for v in a))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(requests)
    res = []
    for line in out:
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        n, nH = int(a[1]), int(a[2])
        per = NT if n else 0
        p = 3
        take = lambda k, dt=np.float64: np.array(a[p:p + k], dtype=dt)
        d = {}
        for key, k, dt in (("tri", n, np.int64), ("const", 6 * n, np.float64), ("woven", per, np.int64), ("a", 2 * per, np.float64), ("const4", 4 * per, np.float64),
                           ("hinge", 3 * nH, np.float64), ("same", 1, np.int64), ("stvk", 2 * NT, np.float64)):
            d[key] = take(k, dt)
            p += k
        assert p == len(a)
        d["const"], d["a"], d["const4"], d["hinge"] = d["const"].reshape(6, n), d["a"].reshape(per, 2), d["const4"].reshape(per, 4), d["hinge"].reshape(nH, 3)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("shell_weave_plan_main", [])
    return lambda requests: _run(exe, requests)


def frame(t):
    X = V[TRI[t]]
    t1 = (X[1] - X[0]) / np.linalg.norm(X[1] - X[0])
    r = (X[2] - X[0]) - np.dot(X[2] - X[0], t1) * t1
    return t1, r / np.linalg.norm(r), 0.5 * np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0]))


def check(q, got):
    assert isinstance(got, dict), got
    woven = np.zeros(NT, dtype=np.int64) if q["woven"] is None else q["woven"].astype(np.int64)
    ids = np.flatnonzero(woven == 1)
    assert np.array_equal(got["tri"], ids)
    stvk = np.arange(4 * NT + 1, 6 * NT + 1, dtype=np.float64).reshape(2, NT)
    stvk[:, ids] = 0.0
    assert np.array_equal(got["stvk"], stvk.ravel())  # the two StVK constants of the woven triangles are zero, every other entry as it was
    if not len(ids):
        assert got["const"].size == 0 and got["woven"].size == 0 and got["a"].size == 0 and got["const4"].size == 0  # the empty plan
        assert np.all(got["hinge"][:, 2] == 1.0) and got["same"][0] == 1
        return
    assert np.array_equal(got["woven"], woven)
    nu = np.zeros(NT) if q["nu12"] is None else q["nu12"]
    bw = np.ones(NT) if q["bw"] is None else q["bw"]
    bf = np.ones(NT) if q["bf"] is None else q["bf"]
    a3 = {}
    for i, t in enumerate(ids):
        t1, t2, A = frame(t)
        d = q["dir"][t] / np.linalg.norm(q["dir"][t])
        a = np.array([d @ t1, d @ t2])
        a /= np.linalg.norm(a)
        a3[t] = a[0] * t1 + a[1] * t2
        den = 1.0 - nu[t] * nu[t] * q["E2"][t] / q["E1"][t]
        c4 = np.array([q["E1"][t] / den, nu[t] * q["E2"][t] / den, q["E2"][t] / den, q["G12"][t]])
        assert np.allclose(got["a"][t], a, rtol=0, atol=1e-14) and abs(np.linalg.norm(got["a"][t]) - 1.0) <= 4e-16
        assert np.allclose(got["const4"][t], c4, rtol=1e-14, atol=0)
        assert np.allclose(got["const"][:, i], np.concatenate([a, H[t] * A * c4]), rtol=1e-13, atol=1e-14)
    off = np.setdiff1d(np.arange(NT), ids)
    assert not got["a"][off].any() and not got["const4"][off].any()
    # hinges: the mean over the two triangles of the edge of bendWarp sin^2 phi + bendWeft cos^2 phi, 1 for a triangle that is not woven
    edge_tris = {}
    for t, tri in enumerate(TRI.tolist()):
        for k in range(3):
            edge_tris.setdefault(tuple(sorted((tri[k], tri[(k + 1) % 3]))), []).append(t)
    assert len(got["hinge"]) == sum(len(v) == 2 for v in edge_tris.values()) == 8
    for x0, x1, f in got["hinge"]:
        e = V[int(x1)] - V[int(x0)]
        e /= np.linalg.norm(e)
        want = 0.0
        for t in edge_tris[(int(x0), int(x1))]:
            c2 = (e @ a3[t]) ** 2 if t in a3 else 0.0
            want += (bw[t] * (1.0 - c2) + bf[t] * c2) if t in a3 else 1.0
        assert abs(f - want / 2.0) <= 1e-13 * max(1.0, want), (x0, x1, f, want / 2.0)
    assert got["same"][0] == int(np.all(got["hinge"][:, 2] == 1.0))


def good_requests():
    c30 = np.cos(np.radians(30.0)) * EX - np.sin(np.radians(30.0)) * EY
    some = np.array([0, 1, 0, 1, 1, 0, 0, 1], dtype=np.float64)
    nanwhere = np.where(some == 1, 0.3, np.nan)  # a value of a triangle that is not woven is not read
    return {"every triangle, warp along x": req(bend_warp=10.0, bend_weft=2.0, nu12=0.25),
            "every triangle, warp along y": req(d=EY, bend_warp=10.0, bend_weft=2.0),
            "every triangle, warp at 30 degrees to x": req(d=c30, bend_warp=10.0, bend_weft=2.0),
            "warp out of the plane by 60 degrees, long vector": req(d=1e3 * (0.5 * EX + np.sqrt(0.75) * NORMAL), nu12=-0.4),
            "some triangles": req(woven=some, nu12=nanwhere, bend_warp=np.where(some == 1, 4.0, -1.0), bend_weft=3.0, d=EX + 0.5 * EY),
            "all factors one": req(bend_warp=1.0, bend_weft=1.0, bend_scale=0.37),
            "default factors": req(bend_scale=1.7),
            "equal factors 3": req(bend_warp=3.0, bend_weft=3.0, d=c30),
            "all zeros": req(woven=0, E1=-1.0), "null selector": req(woven=None)}


def test_compact_list_constants_and_hinge_factors(planner):
    G = good_requests()
    res = planner(list(G.values()))
    for (name, q), got in zip(G.items(), res):
        check(q, got)
    by = dict(zip(G, res))
    along = {"x": [], "y": [], "d": []}
    for x0, x1, _ in by["every triangle, warp along x"]["hinge"]:
        e = (V[int(x1)] - V[int(x0)]) @ R  # back in the sheet's own plane
        along["x" if abs(e[1]) < 1e-12 else "y" if abs(e[0]) < 1e-12 else "d"].append((int(x0), int(x1)))
    assert [len(v) for v in along.values()] == [2, 2, 4]
    f = lambda name: {(int(a), int(b)): v for a, b, v in by[name]["hinge"]}
    wx, wy, w30 = f("every triangle, warp along x"), f("every triangle, warp along y"), f("every triangle, warp at 30 degrees to x")
    for e in along["x"]:  # an edge along the warp curves the weft yarns; along the weft, the warp yarns; at 30 degrees a quarter and three quarters
        assert abs(wx[e] - 2.0) <= 1e-13 and abs(wy[e] - 10.0) <= 1e-13 and abs(w30[e] - (0.25 * 10.0 + 0.75 * 2.0)) <= 1e-13
    for e in along["y"]:
        assert abs(wx[e] - 10.0) <= 1e-13 and abs(wy[e] - 2.0) <= 1e-13 and abs(w30[e] - (0.75 * 10.0 + 0.25 * 2.0)) <= 1e-13
    for e in along["d"]:
        assert abs(wx[e] - 6.0) <= 1e-13 and abs(wy[e] - 6.0) <= 1e-13
    some = by["some triangles"]
    assert some["tri"].tolist() == [1, 3, 4, 7]
    mixed = [v for a, b, v in some["hinge"] if v != 1.0]
    assert 0 < len(mixed) and any(abs(v - 1.0) > 0.5 for v in mixed)  # hinges with one woven triangle: (1 + its factor) / 2
    assert by["warp out of the plane by 60 degrees, long vector"]["a"][0] == pytest.approx(by["every triangle, warp along x"]["a"][0], abs=1e-14)
    # all-ones factors leave row 1 of hingeConst bit for bit the shell plan's; so does no factor at all; equal factors are exactly that factor
    for name in ("all factors one", "default factors"):
        assert by[name]["same"][0] == 1 and np.all(by[name]["hinge"][:, 2] == 1.0) and len(by[name]["tri"]) == NT
    assert np.all(by["equal factors 3"]["hinge"][:, 2] == 3.0) and by["equal factors 3"]["same"][0] == 0
    for name in ("all zeros", "null selector"):  # removal returns the empty plan
        assert len(by[name]["tri"]) == 0 and by[name]["same"][0] == 1


def bad_requests():
    one = lambda i, v, base: np.array([v if j == i else base for j in range(NT)], dtype=np.float64)
    dirs = lambda i, v: np.array([v if j == i else EX for j in range(NT)])
    q = lambda **kw: req(**kw)
    bad_dir = lambda i, v: dict(req(), dir=dirs(i, v))
    return {"selector other than 0 or 1": (2, q(woven=one(2, 2, 1))), "selector other than 0 or 1, negative": (0, q(woven=one(0, -1, 0))),
            "not finite, E1": (3, q(E1=one(3, np.nan, 1e5))), "not finite, nu12": (1, q(nu12=one(1, np.inf, 0.2))), "not finite, bend factor": (4, q(bend_warp=one(4, np.inf, 1.0))),
            "not finite, direction": (5, bad_dir(5, [np.nan, 0.0, 1.0])),
            "not positive, E1": (6, q(E1=one(6, 0.0, 1e5))), "not positive, E2": (7, q(E2=one(7, -1.0, 5e4))), "not positive, G12": (0, q(G12=one(0, 0.0, 2e3))),
            "nu12^2 >= E1 / E2": (2, q(nu12=one(2, np.sqrt(2.0) * 1.0000001, 0.2))), "nu12^2 >= E1 / E2, negative": (2, q(nu12=one(2, -1.5, 0.2))),
            "bend factor that is not positive": (3, q(bend_weft=one(3, 0.0, 1.0))), "bend factor that is not positive, warp": (3, q(bend_warp=one(3, -2.0, 1.0))),
            "zero length": (4, bad_dir(4, [0.0, 0.0, 0.0])), "normal to the triangle": (5, bad_dir(5, NORMAL)),
            "normal to the triangle, nearly": (6, bad_dir(6, NORMAL + 5e-7 * EX))}


def test_rejections(planner):
    B = bad_requests()
    for (name, (t, _)), got in zip(B.items(), planner([q for _, q in B.values()])):
        assert isinstance(got, str), (name, got)
        assert name.split(",")[0] in got, (name, got)
        assert f"triangle {t} " in got, (name, got)
    # just inside the two bounds: accepted
    ok = planner([req(nu12=np.sqrt(2.0) * 0.9999999), dict(req(), dir=np.tile(NORMAL + 2e-6 * EX, (NT, 1)))])
    assert all(isinstance(r, dict) and len(r["tri"]) == NT for r in ok)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("shell_weave_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_requests(), bad_requests()
    res = _run(exe, list(G.values()) + [q for _, q in B.values()])
    for q, got in zip(G.values(), res):
        check(q, got)
    assert all(isinstance(r, str) for r in res[len(G):])
