"""Host side of the shells' rubber membrane (`ipcgpu_shell_set_membrane`): `ipc_amd/csrc/shell_rubber_plan.cpp` run as a stand-alone program
(`tests/shell_rubber_plan/main.cpp`) and compared with NumPy constructions; the same program once more under the address and undefined-behaviour
sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "shell_rubber_plan", "main.cpp"), os.path.join(CSRC, "shell_rubber_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "shell_rubber_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "shell_rubber_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, requests):
    """requests: [(K[nTri], model or None, alpha or None)] -> per request the reason of the rejection (str) or a dict"""
    text = []
    for K, model, alpha in requests:
        arrs = [np.asarray(K, dtype=np.float64)] + [np.asarray(a, dtype=np.float64) for a in (model, alpha) if a is not None]
        text.append(f"{len(K)} {int(model is not None)} {int(alpha is not None)} " + " ".join(repr(float(v)) for a in arrs for v in a))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(requests)
    res = []
    for line, (K, *_rest) in zip(out, requests):
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        n, nt = int(a[1]), len(K)
        per = nt if n else 0
        d = {"tri": np.array(a[2:2 + n], dtype=np.int64), "const": np.array(a[2 + n:2 + 3 * n], dtype=np.float64).reshape(2, n),
             "model": np.array(a[2 + 3 * n:2 + 3 * n + per], dtype=np.int64), "alpha": np.array(a[2 + 3 * n + per:2 + 3 * n + 2 * per], dtype=np.float64),
             "stvk": np.array(a[2 + 3 * n + 2 * per:], dtype=np.float64)}
        assert len(d["stvk"]) == 2 * nt
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("shell_rubber_plan_main", [])
    return lambda requests: _run(exe, requests)


K5 = np.array([2.0, 3.0, 0.5, 7.0, 11.0])


def good_requests():
    return {"every triangle, default alpha": (K5, np.ones(5), None), "every triangle, alpha 0.5": (K5, np.ones(5), np.full(5, 0.5)),
            "some triangles": (K5, [0, 1, 0, 1, 1], [9.0, 0.1, float("nan"), 0.0, 0.999]), "all zeros": (K5, np.zeros(5), [-1.0] * 5), "null model": (K5, None, None),
            "null model, alpha given": (K5, None, np.full(5, 0.3)), "no triangle": (np.zeros(0), np.zeros(0), None),
            "StVK triangle without stiffness": (np.array([1.0, 0.0, 1.0, 1.0, 1.0]), [1, 0, 1, 1, 1], None)}


def check(K, model, alpha, got):
    K = np.asarray(K, dtype=np.float64)
    nt = len(K)
    model = np.zeros(nt, dtype=np.int64) if model is None else np.asarray(model, dtype=np.int64)
    al = np.zeros(nt) if alpha is None else np.asarray(alpha, dtype=np.float64)
    ids = np.flatnonzero(model == 1)
    assert isinstance(got, dict), got
    assert np.array_equal(got["tri"], ids)
    assert np.array_equal(got["const"], np.vstack([K[ids] * (1.0 - al[ids]) / 6.0, K[ids] * al[ids] / 6.0]).reshape(2, len(ids)))  # (the same operations: the same rounding)
    want_alpha = np.zeros(nt)
    want_alpha[ids] = al[ids]
    assert np.array_equal(got["model"], model if len(ids) else np.zeros(0)) and np.array_equal(got["alpha"], want_alpha if len(ids) else np.zeros(0))
    stvk = np.arange(4 * nt + 1, 6 * nt + 1, dtype=np.float64).reshape(2, nt)
    stvk[:, ids] = 0.0
    assert np.array_equal(got["stvk"], stvk.ravel())  # the two StVK constants of the rubber triangles are zero, every other entry as it was


def test_compact_list_and_constants(planner):
    G = good_requests()
    res = planner(list(G.values()))
    for (name, req), got in zip(G.items(), res):
        check(*req, got)
    by = dict(zip(G, res))
    assert by["some triangles"]["tri"].tolist() == [1, 3, 4]  # alpha of a StVK triangle is not read (9, nan)
    assert by["some triangles"]["const"][1, 1] == 0.0  # alpha 0: neo-Hookean, no I2 term
    for name in ("all zeros", "null model", "null model, alpha given", "no triangle"):
        assert len(by[name]["tri"]) == 0
    # k1 + k2 = h A mu / 2 = K / 6 whatever alpha
    c = by["every triangle, alpha 0.5"]["const"]
    assert np.allclose(c[0] + c[1], K5 / 6.0, rtol=4e-16, atol=0)


def bad_requests():
    one = lambda i, v, base: [v if j == i else base for j in range(5)]
    return {"model other than 0": (K5, one(2, 2, 1), None), "model other than 0, negative": (K5, one(0, -1, 0), None),
            "alpha outside": (K5, np.ones(5), one(3, 1.0, 0.2)), "alpha outside, negative": (K5, np.ones(5), one(3, -0.1, 0.2)),
            "alpha that is not finite": (K5, np.ones(5), one(1, float("nan"), 0.2)), "alpha that is not finite, inf": (K5, np.ones(5), one(1, float("inf"), 0.2)),
            "no membrane stiffness": (np.array([1.0, 0.0, 1.0, 1.0, 1.0]), np.ones(5), None)}


def test_rejections(planner):
    B = bad_requests()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        assert name.split(",")[0] in got, (name, got)
        assert "triangle" in got


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("shell_rubber_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_requests(), bad_requests()
    res = _run(exe, list(G.values()) + list(B.values()))
    for req, got in zip(G.values(), res):
        check(*req, got)
    assert all(isinstance(r, str) for r in res[len(G):])
