"""Host side of the gas law (`ipcgpu_chamber_set_gas`): buildChamberGas and chamberGasPressureOk of `ipc_amd/csrc/chamber_plan.cpp` run as a stand-alone
program (`tests/chamber_gas_plan/main.cpp`): the slice list covers every triangle of every gas chamber once and never crosses a chamber, slices hold at most
256 triangles, their order is by chamber and then by index, constant chambers get no slice, and the validation messages.  The same program once more under
the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "chamber_gas_plan", "main.cpp"), os.path.join(CSRC, "chamber_plan.cpp")]


def _build(name, extra):
    exe = os.path.join(HERE, "chamber_gas_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "chamber_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _set(sizes, gas, p=None, rest=None, fill=None, nxt=None):
    """sizes: triangles per chamber; gas: per chamber None (constant) or (ambient, gamma); fill: per chamber or None (a null pointer); nxt: pressures to ask about"""
    n = len(sizes)
    p = [20.0] * n if p is None else p
    return {"triEnd": np.cumsum(sizes).tolist(), "p": p, "rest": [1e-3 * (i + 1) for i in range(n)] if rest is None else rest, "gas": gas, "fill": fill,
            "next": p if nxt is None else nxt}


def _run(exe, sets):
    text = []
    for s in sets:
        n = len(s["triEnd"])
        a = [str(n), "0" if s["fill"] is None else "1"] + [str(v) for v in s["triEnd"]] + [repr(float(v)) for v in s["p"]] + [repr(float(v)) for v in s["rest"]]
        for c in range(n):
            g = s["gas"][c]
            a += ["0", "0", "1", "0"] if g is None else ["1", repr(float(g[0])), repr(float(g[1])), repr(float(0.0 if s["fill"] is None else s["fill"][c]))]
        text.append(" ".join(a + [repr(float(v)) for v in s["next"]]))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(sets)
    res = []
    for line, s in zip(out, sets):
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        nGas, nSlice, ok = int(a[1]), int(a[2]), int(a[3])
        v = a[4:]
        take = lambda m, t=int: [t(x) for x in (v[:m], v.__delitem__(slice(0, m)))[0]]
        d = {"nGas": nGas, "ok": ok, "gasChamber": take(nGas), "sliceOff": take(nGas + 1), "begin": take(nSlice), "end": take(nSlice), "fill": take(len(s["triEnd"]), float)}
        assert not v
        res.append(d)
    return res


GOOD = {
    "cube, sphere, icosahedron": _set([12, 320, 20], [None, (1e5, 1.4), (2.5e4, 1.0)]),
    "exact multiples and one over": _set([256, 512, 257, 1], [(1e5, 1.0)] * 4),
    "all constant": _set([12, 300], [None, None]),
    "fill volumes given": _set([12, 12, 12], [(1e5, 1.4), None, (1e5, 1.4)], fill=[2e-3, 5.0, -1.0]),
    "eight gas chambers": _set([7] * 9, [(10.0, 1.0)] * 8 + [None]),
    "negative gauge pressure": _set([12], [(100.0, 1.0)], p=[-30.0], nxt=[-100.0]),
}
BAD = {
    "nine gas chambers": (_set([7] * 9, [(10.0, 1.0)] * 9), "9 gas chambers"),
    "ambient < 0": (_set([12, 12], [None, (-1.0, 1.4)]), "chamber 1 has the ambient pressure"),
    "gamma < 1": (_set([12], [(1e5, 0.99)]), "chamber 0 has the exponent gamma"),
    "ambient nan": (_set([12], [(float("nan"), 1.4)]), "chamber 0 has a parameter that is not finite"),
    "gamma inf": (_set([12], [(1e5, float("inf"))]), "chamber 0 has a parameter that is not finite"),
    "fill nan": (_set([12], [(1e5, 1.4)], fill=[float("nan")]), "chamber 0 has a parameter that is not finite"),
    "P0 <= 0": (_set([12, 12], [(30.0, 1.0), (20.0, 1.0)], p=[-10.0, -20.0]), "gas chamber 1: ambient + pressure"),
    "no chambers": (_set([], []), "without chambers"),
}


def check_good(s, d):
    sizes = np.diff([0] + s["triEnd"])
    gasIds = [c for c, g in enumerate(s["gas"]) if g is not None]
    assert d["nGas"] == len(gasIds) and d["gasChamber"] == gasIds
    assert d["sliceOff"][0] == 0 and d["sliceOff"][-1] == len(d["begin"]) == len(d["end"])
    covered = np.zeros(s["triEnd"][-1], dtype=int)
    for g, c in enumerate(gasIds):
        lo, hi = s["triEnd"][c] - sizes[c], s["triEnd"][c]
        sl = range(d["sliceOff"][g], d["sliceOff"][g + 1])
        assert len(sl) == -(-sizes[c] // 256)  # as few slices as 256 allows
        at = lo
        for i in sl:
            assert d["begin"][i] == at and 0 < d["end"][i] - d["begin"][i] <= 256 and d["end"][i] <= hi  # by index, no gap, never across the chamber's end
            covered[d["begin"][i]:d["end"][i]] += 1
            at = d["end"][i]
        assert at == hi
    for c, g in enumerate(s["gas"]):  # every triangle of a gas chamber once, none of a constant chamber
        assert np.all(covered[s["triEnd"][c] - sizes[c]:s["triEnd"][c]] == (0 if g is None else 1))
    assert d["begin"] == sorted(d["begin"])  # chamber after chamber
    for c, g in enumerate(s["gas"]):
        want = s["rest"][c] if g is None or s["fill"] is None or not s["fill"][c] > 0 else s["fill"][c]
        assert d["fill"][c] == want if d["nGas"] else True


def check_all(exe):
    res = _run(exe, list(GOOD.values()) + [b for b, _ in BAD.values()])
    for (name, s), d in zip(GOOD.items(), res):
        assert isinstance(d, dict), (name, d)
        check_good(s, d)
    by = dict(zip(GOOD, res))
    assert by["all constant"]["nGas"] == 0 and by["all constant"]["begin"] == []
    assert by["cube, sphere, icosahedron"]["begin"] == [12, 268, 332] and by["cube, sphere, icosahedron"]["end"] == [268, 332, 352]
    assert by["negative gauge pressure"]["ok"] == 0 and by["cube, sphere, icosahedron"]["ok"] == 1  # chamberGasPressureOk: -100 + 100 <= 0 is refused
    for (name, (_, want)), got in zip(BAD.items(), res[len(GOOD):]):
        assert isinstance(got, str) and want in got, (name, got)


def test_slices_and_validation():
    check_all(_build("chamber_gas_plan_main", []))


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    check_all(_build("chamber_gas_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
