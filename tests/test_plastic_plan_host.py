"""Host side of the plastic flow (`ipcgpu_set_plasticity`): `ipc_amd/csrc/plastic_plan.cpp` run as a stand-alone program (`tests/plastic_plan/main.cpp`): the
parameter arrays after sequences of range calls, every rejection (each leaves the plan as it was), overlapping ranges, +inf switching a range off; the same
program once more under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "plastic_plan", "main.cpp"), os.path.join(CSRC, "plastic_plan.cpp")]
INF, NAN = float("inf"), float("nan")


def _build(name, extra):
    exe = os.path.join(HERE, "plastic_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "plastic_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, sets):
    """sets: (nT, [(tetBegin, tetEnd, yield, creep, harden), ...]) -> per set (results per call: True or the reason, nT, nOn, yield, creep, harden)"""
    text = [f"{nT} {len(calls)} " + " ".join(f"{b} {e} {y!r} {c!r} {h!r}" for b, e, y, c, h in calls) for nT, calls in sets]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(sets)
    res = []
    for line, (nT, calls) in zip(out, sets):
        head, tail = line.split("|")
        oks = [True if t == "1" else t[1:].replace("~", " ") for t in head.split()]
        assert len(oks) == len(calls)
        a = tail.split()
        n = int(a[0])
        v = np.array(a[2:], dtype=np.float64)
        assert len(v) == 3 * n
        res.append((oks, n, int(a[1]), v[:n], v[n:2 * n], v[2 * n:]))
    return res


def expected(nT, calls):
    """the documented rule, restated: valid calls overwrite their range in order, invalid ones change nothing"""
    y, c, h = np.full(nT, INF), np.full(nT, INF), np.zeros(nT)
    touched, oks = False, []
    for b, e, yy, cc, hh in calls:
        ok = nT > 0 and 0 <= b <= e <= nT and not any(np.isnan(v) for v in (yy, cc, hh)) and yy >= 0 and cc > 0 and 0 <= hh < INF
        oks.append(ok)
        if ok:
            touched = True
            y[b:e], c[b:e], h[b:e] = yy, cc, hh
    return oks, (nT if touched else 0), y, c, h


GOOD = {
    "one range": (10, [(2, 7, 0.05, INF, 0.0)]),
    "whole mesh, finite creep, hardening": (5, [(0, 5, 0.0, 3.5, 2.0)]),
    "overlapping ranges: the later call overwrites": (12, [(0, 8, 0.05, INF, 0.0), (4, 12, 0.1, 2.0, 0.5), (6, 7, 0.2, 1.0, 0.25)]),
    "+inf switches a range off": (12, [(0, 12, 0.05, 4.0, 1.0), (3, 9, INF, INF, 0.0)]),
    "+inf switches everything off again": (6, [(0, 6, 0.05, INF, 0.0), (0, 6, INF, 5.0, 0.0)]),
    "only +inf: allocated, nothing on": (6, [(0, 6, INF, INF, 0.0)]),
    "empty ranges": (6, [(0, 0, 0.05, INF, 0.0), (6, 6, 0.05, INF, 0.0), (3, 3, 0.05, INF, 0.0)]),
    "yield 0": (3, [(1, 2, 0.0, INF, 0.0)]),
    "denormal creep": (3, [(0, 3, 0.1, 5e-324, 0.0)]),
}
_OK = (2, 7, 0.05, INF, 0.0)
BAD = {  # a good call, the bad one, a good one: name -> (nT, calls, reason)
    "negative begin": (10, [_OK, (-1, 4, 0.05, INF, 0.0), (8, 10, 0.3, 1.0, 0.0)], "range out of bounds"),
    "begin behind end": (10, [_OK, (5, 4, 0.05, INF, 0.0)], "range out of bounds"),
    "end behind the mesh": (10, [_OK, (5, 11, 0.05, INF, 0.0)], "range out of bounds"),
    "negative yield": (10, [_OK, (0, 10, -1e-300, INF, 0.0)], "yield strain is negative"),
    "yield -inf": (10, [_OK, (0, 10, -INF, INF, 0.0)], "yield strain is negative"),
    "yield NaN": (10, [_OK, (0, 10, NAN, INF, 0.0)], "NaN"),
    "creep 0": (10, [_OK, (0, 10, 0.05, 0.0, 0.0)], "creep rate is not positive"),
    "creep negative": (10, [_OK, (0, 10, 0.05, -2.0, 0.0)], "creep rate is not positive"),
    "creep NaN": (10, [_OK, (0, 10, 0.05, NAN, 0.0)], "NaN"),
    "harden negative": (10, [_OK, (0, 10, 0.05, INF, -0.5)], "hardening modulus is negative"),
    "harden inf": (10, [_OK, (0, 10, 0.05, INF, INF)], "hardening modulus is not finite"),
    "harden NaN": (10, [_OK, (0, 10, 0.05, INF, NAN)], "NaN"),
    "bad first call": (10, [(0, 11, 0.05, INF, 0.0)], "range out of bounds"),
    "no tetrahedron": (0, [(0, 0, 0.05, INF, 0.0)], "no tetrahedron"),
}


def check(nT, calls, got):
    oks, n, nOn, y, c, h = got
    eo, en, ey, ec, eh = expected(nT, calls)
    assert [o is True for o in oks] == eo
    assert n == en
    if n:
        assert np.array_equal(y, ey) and np.array_equal(c, ec) and np.array_equal(h, eh)
        assert nOn == int(np.sum(ey < INF))
    else:
        assert nOn == 0 and len(y) == 0


@pytest.fixture(scope="module")
def planner():
    exe = _build("plastic_plan_main", [])
    return lambda sets: _run(exe, sets)


def test_ranges(planner):
    res = dict(zip(GOOD, planner(list(GOOD.values()))))
    for name, got in res.items():
        assert all(o is True for o in got[0]), name
        check(*GOOD[name], got)
    assert res["overlapping ranges: the later call overwrites"][3].tolist() == [0.05] * 4 + [0.1] * 2 + [0.2] + [0.1] * 5
    assert res["+inf switches a range off"][2] == 6 and res["+inf switches everything off again"][2] == 0 and res["only +inf: allocated, nothing on"][1] == 6
    assert res["empty ranges"][2] == 0 and res["empty ranges"][1] == 6


def test_rejections(planner):
    res = dict(zip(BAD, planner([(nT, calls) for nT, calls, _ in BAD.values()])))
    for name, got in res.items():
        nT, calls, reason = BAD[name]
        bad = [o for o in got[0] if o is not True]
        assert len(bad) == 1 and reason in bad[0] and bad[0].startswith("set_plasticity: "), (name, got[0])
        check(nT, calls, got)  # the plan is what the good calls alone leave


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("plastic_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    sets = list(GOOD.values()) + [(nT, calls) for nT, calls, _ in BAD.values()]
    for (nT, calls), got in zip(sets, _run(exe, sets)):
        check(nT, calls, got)
