"""Host side of the shells' plastic flow (`ipcgpu_shell_set_plasticity`): `ipc_amd/csrc/shell_plastic_plan.cpp` run as a stand-alone program
(`tests/shell_plastic_plan/main.cpp`, with `shell_plan.cpp` for the shell): the parameter arrays after sequences of range calls, every refusal (each leaves the
plan as it was), which hinges flow and their mean parameters, g on a hand-computed two-triangle case; the same program once more under the address and
undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "shell_plastic_plan", "main.cpp"), os.path.join(CSRC, "shell_plastic_plan.cpp"), os.path.join(CSRC, "shell_plan.cpp")]
INF, NAN = float("inf"), float("nan")


def _build(name, extra):
    exe = os.path.join(HERE, "shell_plastic_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "shell_plastic_plan.h"), os.path.join(CSRC, "shell_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


# a strip of four triangles over the nodes 0 .. 5 (two rows of three), thicknesses 0.01, 0.02, 0.03, 0.04: three hinges
STRIP_V = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]], dtype=float)
STRIP_T = np.array([[0, 2, 1], [1, 2, 3], [2, 4, 3], [3, 4, 5]])
STRIP_H = [0.01, 0.02, 0.03, 0.04]
# the hand-computed case: two right triangles with legs 2 and 1 over the shared edge (0, 0, 0) - (0, 2, 0), thicknesses 0.01 and 0.03
PAIR_V = np.array([[0, 0, 0], [0, 2, 0], [1, 0, 0], [-1, 2, 0]], dtype=float)
PAIR_T = np.array([[0, 2, 1], [1, 3, 0]])
PAIR_H = [0.01, 0.03]


def _run(exe, sets):
    """sets: (V, T, h, rubber, calls) -> per set (results per call, counts4, yield, bendYield, creep, harden, hingeTri, hingeYield, hingeCreep, hingeHarden, hingeG)"""
    text = []
    for V, T, h, rubber, calls in sets:
        text.append(" ".join([f"{len(V)} {len(T)}"] + [repr(float(v)) for v in np.asarray(V).ravel()] + [str(int(v)) for v in np.asarray(T).ravel()] + [repr(float(v)) for v in h]
                             + [str(int(v)) for v in rubber] + [str(len(calls))] + [f"{b} {e} {y!r} {yb!r} {c!r} {K!r}" for b, e, y, yb, c, K in calls]))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(sets)
    res = []
    for line in out:
        parts = line.split("|")
        oks = [True if t == "1" else t[1:].replace("~", " ") for t in parts[0].split()]
        arr = [np.array(p.split(), dtype=np.float64) for p in parts[2:]]
        res.append((oks, [int(v) for v in parts[1].split()]) + tuple(arr))
    return res


def expected(nTri, rubber, calls):
    """the documented rule, restated: valid calls overwrite their range in order, invalid ones change nothing"""
    y, yb, c, K = np.full(nTri, INF), np.full(nTri, INF), np.full(nTri, INF), np.zeros(nTri)
    touched, oks = False, []
    for b, e, yy, yyb, cc, kk in calls:
        ok = nTri > 0 and 0 <= b <= e <= nTri and not any(np.isnan(v) for v in (yy, yyb, cc, kk)) and yy >= 0 and yyb >= 0 and cc > 0 and 0 <= kk < INF
        ok = ok and not ((yy < INF or yyb < INF) and any(rubber[b:e]))
        oks.append(ok)
        if ok:
            touched = True
            y[b:e], yb[b:e], c[b:e], K[b:e] = yy, yyb, cc, kk
    return oks, touched, y, yb, c, K


NO_RUBBER = [0, 0, 0, 0]
_OK = (1, 3, 0.05, 0.002, INF, 0.0)
GOOD = {
    "one range": [_OK],
    "whole shell, finite creep, hardening": [(0, 4, 0.0, 0.0, 3.5, 2.0)],
    "overlapping ranges: the later call overwrites": [(0, 3, 0.05, 0.001, INF, 0.0), (2, 4, 0.1, 0.003, 2.0, 0.5), (1, 2, 0.2, INF, 1.0, 0.25)],
    "+inf switches a range off": [(0, 4, 0.05, 0.002, 4.0, 1.0), (1, 3, INF, INF, INF, 0.0)],
    "membrane only": [(0, 4, 0.05, INF, INF, 0.0)],
    "hinges only": [(0, 4, INF, 0.002, INF, 0.0)],
    "only +inf: allocated, nothing on": [(0, 4, INF, INF, INF, 0.0)],
    "empty ranges": [(0, 0, 0.05, 0.002, INF, 0.0), (4, 4, 0.05, 0.002, INF, 0.0)],
}
BAD = {  # a good call, the bad one (, a good one): name -> (calls, reason)
    "negative begin": ([_OK, (-1, 2, 0.05, 0.002, INF, 0.0), (3, 4, 0.3, 0.1, 1.0, 0.0)], "range out of bounds"),
    "begin behind end": ([_OK, (3, 2, 0.05, 0.002, INF, 0.0)], "range out of bounds"),
    "end behind the shell": ([_OK, (2, 5, 0.05, 0.002, INF, 0.0)], "range out of bounds"),
    "negative yield": ([_OK, (0, 4, -1e-300, 0.002, INF, 0.0)], "yield strain is negative"),
    "negative bendYield": ([_OK, (0, 4, 0.05, -INF, INF, 0.0)], "bending yield strain is negative"),
    "yield NaN": ([_OK, (0, 4, NAN, 0.002, INF, 0.0)], "NaN"),
    "bendYield NaN": ([_OK, (0, 4, 0.05, NAN, INF, 0.0)], "NaN"),
    "creep 0": ([_OK, (0, 4, 0.05, 0.002, 0.0, 0.0)], "creep rate is not positive"),
    "creep negative": ([_OK, (0, 4, 0.05, 0.002, -2.0, 0.0)], "creep rate is not positive"),
    "creep NaN": ([_OK, (0, 4, 0.05, 0.002, NAN, 0.0)], "NaN"),
    "harden negative": ([_OK, (0, 4, 0.05, 0.002, INF, -0.5)], "hardening modulus is negative"),
    "harden inf": ([_OK, (0, 4, 0.05, 0.002, INF, INF)], "hardening modulus is not finite"),
    "harden NaN": ([_OK, (0, 4, 0.05, 0.002, INF, NAN)], "NaN"),
    "bad first call": ([(0, 5, 0.05, 0.002, INF, 0.0)], "range out of bounds"),
}


def strip_set(calls, rubber=NO_RUBBER):
    return (STRIP_V, STRIP_T, STRIP_H, rubber, calls)


def check(calls, got, rubber=NO_RUBBER):
    oks, (nTri, nHinge, nOn, nHingeOn), y, yb, c, K, hingeTri, hy, hc, hK, hg = got
    eo, touched, ey, eyb, ec, eK = expected(4, rubber, calls)
    assert [o is True for o in oks] == eo
    if not touched:
        assert nTri == 0 and nOn == 0 and nHingeOn == 0 and len(y) == 0 and len(hy) == 0
        return
    assert (nTri, nHinge) == (4, 3)
    assert np.array_equal(y, ey) and np.array_equal(yb, eyb) and np.array_equal(c, ec) and np.array_equal(K, eK)
    assert nOn == int(np.sum(ey < INF))
    # the hinges of the strip, ascending by edge: (1, 2) between triangles 0 and 1, (2, 3) between 1 and 2, (3, 4) between 2 and 3
    assert sorted(map(tuple, np.sort(hingeTri.reshape(3, 2).astype(int), axis=1).tolist())) == [(0, 1), (1, 2), (2, 3)]
    for i, (a, b) in enumerate(hingeTri.reshape(3, 2).astype(int)):
        on = eyb[a] < INF and eyb[b] < INF
        assert (hy[i] < INF) == on
        if on:  # the arithmetic means of the two triangles' values
            assert hy[i] == 0.5 * (eyb[a] + eyb[b]) and hc[i] == 0.5 * (ec[a] + ec[b]) and hK[i] == 0.5 * (eK[a] + eK[b])
        else:
            assert hy[i] == INF and hc[i] == INF and hK[i] == 0.0
    assert nHingeOn == int(np.sum(hy < INF))


@pytest.fixture(scope="module")
def planner():
    exe = _build("shell_plastic_plan_main", [])
    return lambda sets: _run(exe, sets)


def test_ranges_hinges_and_means(planner):
    res = dict(zip(GOOD, planner([strip_set(c) for c in GOOD.values()])))
    for name, got in res.items():
        assert all(o is True for o in got[0]), name
        check(GOOD[name], got)
    assert res["overlapping ranges: the later call overwrites"][1] == [4, 3, 4, 1]  # triangle 1 has bendYield +inf: only the hinge (2, 3) flows
    assert res["+inf switches a range off"][1] == [4, 3, 2, 0] and res["membrane only"][1] == [4, 3, 4, 0] and res["hinges only"][1] == [4, 3, 0, 3]
    assert res["only +inf: allocated, nothing on"][1] == [4, 3, 0, 0] and res["empty ranges"][1] == [4, 3, 0, 0]
    hy = res["overlapping ranges: the later call overwrites"][7]
    assert sorted(hy.tolist()) == [0.003, INF, INF]


def test_rejections_leave_the_plan_as_it_was(planner):
    res = dict(zip(BAD, planner([strip_set(calls) for calls, _ in BAD.values()])))
    for name, got in res.items():
        calls, reason = BAD[name]
        bad = [o for o in got[0] if o is not True]
        assert len(bad) == 1 and reason in bad[0] and bad[0].startswith("shell_set_plasticity: "), (name, got[0])
        check(calls, got)  # the plan is what the good calls alone leave


def test_rubber_triangles_and_a_missing_shell_are_refused(planner):
    rubber = [0, 0, 1, 0]
    calls = [(0, 2, 0.05, 0.002, INF, 0.0), (1, 4, 0.05, 0.002, INF, 0.0), (2, 3, INF, 0.002, INF, 0.0), (2, 3, INF, INF, 5.0, 0.5), (3, 4, 0.1, 0.1, INF, 0.0)]
    got = planner([strip_set(calls, rubber)])[0]
    assert [o is True for o in got[0]] == [True, False, False, True, True] and "triangle 2 carries the rubber membrane" in got[0][1]
    check(calls, got, rubber)
    none = planner([(np.zeros((0, 3)), np.zeros((0, 3), dtype=int), [], [], [(0, 0, 0.05, 0.002, INF, 0.0)])])[0]
    assert "no shell is set" in none[0][0] and none[1] == [0, 0, 0, 0]


def test_g_on_a_hand_computed_two_triangle_case(planner):
    got = planner([(PAIR_V, PAIR_T, PAIR_H, [0, 0], [(0, 2, 0.05, 0.002, INF, 0.0)])])[0]
    assert got[1] == [2, 1, 2, 1]
    # |eBar| = 2, A1 = A2 = 1: w_e = 3 |eBar|^2 / (A1 + A2) = 6; h_m = (0.01 + 0.03) / 2 = 0.02; g = h_m w_e / (2 |eBar|) = 0.02 * 6 / 4 = 0.03
    assert got[10].tolist() == pytest.approx([0.03], rel=4 * 2.0 ** -52, abs=0.0)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("shell_plastic_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    lists = list(GOOD.values()) + [calls for calls, _ in BAD.values()]
    for calls, got in zip(lists, _run(exe, [strip_set(c) for c in lists])):
        check(calls, got)
