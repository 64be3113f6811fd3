"""Host side of the shells' strain limit (`ipcgpu_shell_set_strain_limit`): `ipc_amd/csrc/shell_limit_plan.cpp` run as a stand-alone program
(`tests/shell_limit_plan/main.cpp`) and compared with NumPy constructions; the same program once more under the address and undefined-behaviour sanitizers.
No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "shell_limit_plan", "main.cpp"), os.path.join(CSRC, "shell_limit_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "shell_limit_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "shell_limit_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, requests):
    """requests: [(K[nTri], limit or None, onset or None, stiff or None)] -> per request the reason of the rejection (str) or a dict"""
    text = []
    for K, limit, onset, stiff in requests:
        arrs = [np.asarray(K, dtype=np.float64)] + [np.asarray(a, dtype=np.float64) for a in (limit, onset, stiff) if a is not None]
        text.append(f"{len(K)} {int(limit is not None)} {int(onset is not None)} {int(stiff is not None)} " + " ".join(repr(float(v)) for a in arrs for v in a))
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
        n = int(a[1])
        d = {"tri": np.array(a[2:2 + n], dtype=np.int64), "const": np.array(a[2 + n:2 + 4 * n], dtype=np.float64).reshape(3, n),
             "triLimit": np.array(a[2 + 4 * n:], dtype=np.float64)}
        assert len(d["triLimit"]) == (len(K) if n else 0)
        res.append(d)
    return res


@pytest.fixture(scope="module")
def planner():
    exe = _build("shell_limit_plan_main", [])
    return lambda requests: _run(exe, requests)


K5 = np.array([2.0, 3.0, 0.5, 7.0, 11.0])


def good_requests():
    return {"every triangle, defaults": (K5, np.full(5, 1.1), None, None),
            "some triangles, onset and stiffness": (K5, [0.0, 1.2, 0.0, 1.5, 1.05], [9.0, 1.0, -3.0, 1.25, 1.0], [0.0, 2.0, float("nan"), 0.5, 1.0]),
            "all zeros": (K5, np.zeros(5), [0.5] * 5, [-1.0] * 5), "null limit": (K5, None, None, None), "no triangle": (np.zeros(0), np.zeros(0), None, None),
            "onset only": (K5, np.full(5, 2.0), np.full(5, 1.5), None), "stiff only": (K5, np.full(5, 2.0), None, np.full(5, 3.0))}


def check(K, limit, onset, stiff, got):
    K = np.asarray(K, dtype=np.float64)
    limit = np.zeros(len(K)) if limit is None else np.asarray(limit, dtype=np.float64)
    on = np.ones(len(K)) if onset is None else np.asarray(onset, dtype=np.float64)
    st = np.ones(len(K)) if stiff is None else np.asarray(stiff, dtype=np.float64)
    ids = np.flatnonzero(limit > 0)
    assert isinstance(got, dict), got
    assert np.array_equal(got["tri"], ids)
    assert np.array_equal(got["const"], np.vstack([on[ids], limit[ids], st[ids] * K[ids]]).reshape(3, len(ids)))  # (one product: the same rounding)
    assert np.array_equal(got["triLimit"], limit if len(ids) else np.zeros(0))


def test_compact_list_and_constants(planner):
    G = good_requests()
    res = planner(list(G.values()))
    for (name, req), got in zip(G.items(), res):
        check(*req, got)
    by = dict(zip(G, res))
    assert by["some triangles, onset and stiffness"]["tri"].tolist() == [1, 3, 4]  # onset and stiffness of an unlimited triangle are not read (9, -3, nan)
    assert len(by["all zeros"]["tri"]) == 0 and len(by["null limit"]["tri"]) == 0 and len(by["no triangle"]["tri"]) == 0


def bad_requests():
    one = lambda i, v, base=1.0: [v if j == i else base for j in range(5)]
    return {"not above its onset": (K5, one(2, 1.0, 1.3), None, None), "not above its onset, below": (K5, one(2, 1.2, 1.5), np.full(5, 1.25), None),
            "onset below 1": (K5, np.full(5, 1.5), one(4, 0.99), None), "stiff > 0": (K5, np.full(5, 1.5), None, one(0, 0.0)),
            "stiff > 0, negative": (K5, np.full(5, 1.5), None, one(0, -2.0)), "negative limit": (K5, one(1, -1.2, 1.5), None, None),
            "not finite": (K5, one(3, float("nan"), 1.5), None, None), "not finite, inf": (K5, one(3, float("inf"), 1.5), None, None),
            "not finite, onset": (K5, np.full(5, 1.5), one(3, float("nan")), None), "not finite, stiff": (K5, np.full(5, 1.5), None, one(3, float("inf"))),
            "no membrane stiffness": (np.array([1.0, 0.0, 1.0, 1.0, 1.0]), np.full(5, 1.5), None, None)}


def test_rejections(planner):
    B = bad_requests()
    for (name, _), got in zip(B.items(), planner(list(B.values()))):
        assert isinstance(got, str), name
        assert name.split(",")[0] in got, (name, got)
        assert "triangle" in got


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("shell_limit_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_requests(), bad_requests()
    res = _run(exe, list(G.values()) + list(B.values()))
    for req, got in zip(G.values(), res):
        check(*req, got)
    assert all(isinstance(r, str) for r in res[len(G):])
