"""Host side of the round colliders (`ipcgpu_opt_add_round_collider`): `ipc_amd/csrc/round_collider_plan.cpp` run as a stand-alone program
(`tests/round_collider_plan/main.cpp`): the record of every accepted shape, every validation rule with its message, and the same program once more
under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "round_collider_plan", "main.cpp"), os.path.join(CSRC, "round_collider_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "round_collider_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "round_collider_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, rows):
    text = "\n".join(" ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for v in r) for r in rows) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    res = []
    for line in out:
        if line.startswith("0 "):
            res.append(line[2:])
        else:
            v = [float.fromhex(t) for t in line.split()[1:]]
            res.append(dict(p0=v[0:3], p1=v[3:6], axis=v[6:9], len=v[9], R=v[10], side=v[11]))
    return res


def row(p0, p1, R, hollow=0, dHat=0.0):
    return list(p0) + list(p1) + [R, hollow, dHat]


GOOD = {"sphere": row((0.25, -0.5, 0.125), (0.25, -0.5, 0.125), 0.75, 0, 0.01),
        "hollow sphere": row((1.0, 2.0, 3.0), (1.0, 2.0, 3.0), 1.5, 1, 0.01),
        "hollow sphere, dHat not known yet": row((1.0, 2.0, 3.0), (1.0, 2.0, 3.0), 0.05, 1, 0.0),
        "capsule along x": row((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.5),
        "skew capsule": row((0.1, -0.2, 0.3), (0.9, 0.5, -0.1), 0.35, 0, 1.0),  # (R^2 <= dHat is a solid collider's business no more than a plane's)
        "tiny capsule": row((0.0, 0.0, 0.0), (0.0, 1e-150, 0.0), 1e-3)}
nan, inf = float("nan"), float("inf")
BAD = {"an end point is not finite": [row((nan, 0, 0), (0, 0, 0), 1.0), row((0, 0, 0), (0, -inf, 0), 1.0), row((0, 0, inf), (0, 0, inf), 1.0)],
       "the radius is not finite": [row((0, 0, 0), (0, 0, 0), nan), row((0, 0, 0), (1, 0, 0), inf)],
       "the radius must be positive": [row((0, 0, 0), (0, 0, 0), 0.0), row((0, 0, 0), (1, 0, 0), -1.0), row((0, 0, 0), (0, 0, 0), -0.0)],
       "hollow is 0 or 1": [row((0, 0, 0), (0, 0, 0), 1.0, 2), row((0, 0, 0), (0, 0, 0), 1.0, -1)],
       "only a sphere (p0 == p1) may be hollow": [row((0, 0, 0), (1, 0, 0), 1.0, 1), row((0, 0, 0), (0, 5e-324, 0), 1.0, 1)],
       "a hollow sphere needs R^2 > dHat": [row((0, 0, 0), (0, 0, 0), 0.1, 1, 0.011), row((0, 0, 0), (0, 0, 0), 0.1, 1, 0.02)],
       "length is zero or not finite": [row((0, 0, 0), (0, 1e-200, 1e-200), 1.0), row((-1e200, 0, 0), (1e200, 1e200, 0), 1.0)]}


def check_good(r, got):
    assert isinstance(got, dict), got
    p0, p1 = np.array(r[0:3]), np.array(r[3:6])
    assert got["p0"] == r[0:3] and got["p1"] == r[3:6] and got["R"] == r[6] and got["side"] == (-1.0 if r[7] else 1.0)
    if np.array_equal(p0, p1):
        assert got["len"] == 0.0 and got["axis"] == [0.0, 0.0, 0.0]
    else:
        d = p1 - p0
        L = math.sqrt(float(d @ d))  # the same three roundings as the C++
        assert got["len"] == L and got["axis"] == list(d / L)
        assert abs(float(np.dot(got["axis"], got["axis"])) - 1.0) <= 4 * 2.0 ** -53


def test_accepted_shapes_carry_the_axis_and_length():
    res = _run(_build("round_plan_main", []), list(GOOD.values()))
    for (name, r), got in zip(GOOD.items(), res):
        check_good(r, got)
    by = dict(zip(GOOD, res))
    assert by["capsule along x"]["axis"] == [1.0, 0.0, 0.0] and by["capsule along x"]["len"] == 1.0
    assert by["tiny capsule"]["axis"] == [0.0, 1.0, 0.0]


def test_every_rule_refuses_with_its_message():
    exe = _build("round_plan_main", [])
    for msg, rows in BAD.items():
        for got in _run(exe, rows):
            assert isinstance(got, str) and got.startswith("round collider: ") and msg in got, (msg, got)
    # the boundary of the hollow rule: R^2 == dHat is refused, the next double above is taken
    edge = _run(exe, [row((0, 0, 0), (0, 0, 0), 0.5, 1, 0.25), row((0, 0, 0), (0, 0, 0), 0.5, 1, math.nextafter(0.25, 0.0))])
    assert isinstance(edge[0], str) and isinstance(edge[1], dict)


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("round_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    rows = list(GOOD.values()) + [r for rs in BAD.values() for r in rs]
    res = _run(exe, rows)
    for r, got in zip(GOOD.values(), res):
        check_good(r, got)
    assert all(isinstance(g, str) for g in res[len(GOOD):])
