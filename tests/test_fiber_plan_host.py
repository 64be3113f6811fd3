"""Host side of the fibre reinforcement (`ipcgpu_set_fibers`, `ipcgpu_fiber_set_activation`): `ipc_amd/csrc/fiber_plan.cpp` run as a stand-alone program
(`tests/fiber_plan/main.cpp`): every refusal (each leaves the plan as it was), the normalised direction, overwrite and removal, the ascending compact lists,
b = A a against numpy; the same program once more under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import fiber_mp as fm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "fiber_plan", "main.cpp"), os.path.join(CSRC, "fiber_plan.cpp")]
INF, NAN = float("inf"), float("nan")
NT = 12
RNG = np.random.default_rng(5)
A = RNG.normal(size=(9, NT)) * 10.0  # restTriInv, SoA [9][nT]
VOL = 1e-4 * (1.0 + RNG.random(NT))


def _build(name, extra):
    exe = os.path.join(HERE, "fiber_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "fiber_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def F(b, e, d, k, law=0, k2=0.0, tens=0, group=0, per=0):
    d = [] if d is None else list(np.asarray(d, dtype=np.float64).ravel())
    return f"F {b} {e} {per} {k!r} {law} {k2!r} {tens} {group} {len(d) // 3} " + " ".join(repr(float(v)) for v in d)


def ACT(group, act):
    return f"A {group} {act!r}"


def _run(exe, calls, nT=NT, vol=VOL):
    text = f"{nT}\n" + " ".join(repr(float(v)) for v in A[:, :max(nT, 0)].ravel()) + "\n" + " ".join(repr(float(v)) for v in vol[:max(nT, 0)]) + f"\n{len(calls)}\n" + "\n".join(calls) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    oks = [True if t == "1" else t[1:].replace("~", " ") for t in out[0].split()]
    assert len(oks) == len(calls)
    names = ("fibTet", "b", "volK", "k2F", "flagsF", "groupOf", "l0", "dir", "k", "k2", "flags", "group", "act")
    plan = {n: np.array(out[2 + i].split(), dtype=np.float64) for i, n in enumerate(names)}
    plan["nT"], plan["nF"] = (int(v) for v in out[1].split())
    return oks, plan


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    return _build(request.param, [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


D = [0.3, -0.5, 0.8]
REFUSALS = {
    "negative begin": (F(-1, 4, D, 1e4), "range out of bounds"),
    "begin behind end": (F(5, 4, D, 1e4), "range out of bounds"),
    "end behind the mesh": (F(5, NT + 1, D, 1e4), "range out of bounds"),
    "zero direction": (F(0, 4, [0.0, 0.0, 0.0], 1e4), "direction is zero"),
    "NaN direction": (F(0, 4, [0.0, NAN, 1.0], 1e4), "direction is not finite"),
    "infinite direction": (F(0, 4, [INF, 0.0, 1.0], 1e4), "direction is not finite"),
    "one zero direction among per-element ones": (F(0, 2, [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], 1e4, per=1), "direction is zero"),
    "null direction": (F(0, 4, None, 1e4), "null direction"),
    "negative k": (F(0, 4, D, -1.0), "stiffness is negative"),
    "NaN k": (F(0, 4, D, NAN), "stiffness is negative or not finite"),
    "infinite k": (F(0, 4, D, INF), "not finite"),
    "law 1 with k2 = 0": (F(0, 4, D, 1e4, law=1, k2=0.0), "k2 > 0"),
    "law 1 with negative k2": (F(0, 4, D, 1e4, law=1, k2=-2.0), "k2 > 0"),
    "law 1 with NaN k2": (F(0, 4, D, 1e4, law=1, k2=NAN), "k2 > 0"),
    "unknown law": (F(0, 4, D, 1e4, law=2), "unknown law"),
    "negative law": (F(0, 4, D, 1e4, law=-1), "unknown law"),
    "group -1": (F(0, 4, D, 1e4, group=-1), "group is outside [0, 64)"),
    "group 64": (F(0, 4, D, 1e4, group=64), "group is outside [0, 64)"),
    "act = 1": (ACT(0, 1.0), "below 1"),
    "act > 1": (ACT(0, 1.5), "below 1"),
    "NaN act": (ACT(0, NAN), "below 1"),
    "activation group out of range": (ACT(64, 0.1), "group is outside [0, 64)"),
    "activation on a group with exp elements": (ACT(3, 0.2), "not defined for the exp law"),
    "exp on an activated group": (F(0, 2, D, 1e4, law=1, k2=1.0, group=5), "not defined for the exp law"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_the_plan_as_it_was(exe, name):
    bad, reason = REFUSALS[name]
    before = [F(2, 9, D, 2e4, group=1), F(8, 11, [0.0, 1.0, 0.0], 3e4, law=1, k2=4.0, group=3), ACT(5, 0.25), ACT(1, -0.1)]
    oks0, plan0 = _run(exe, before)
    assert oks0 == [True] * 4
    oks, plan = _run(exe, before + [bad])
    assert oks[:4] == [True] * 4 and oks[4] is not True and reason in oks[4], oks[4]
    for k in plan0:
        assert np.array_equal(plan0[k], plan[k]), k


def test_no_tetrahedron_and_activation_before_fibres(exe):
    oks, plan = _run(exe, [F(0, 0, D, 1e4)], nT=0)
    assert "no tetrahedron" in oks[0] and plan["nT"] == 0
    oks, plan = _run(exe, [ACT(0, 0.1)])
    assert "no fibres are set" in oks[0] and plan["nT"] == 0


def test_normalisation_overwrite_removal_and_ascending_lists(exe):
    per = RNG.normal(size=(4, 3)) * np.array([[1e-200], [1.0], [1e200], [3.0]])  # (tiny and huge directions normalise without under- or overflow)
    calls = [F(6, 12, D, 2e4, group=2, tens=1), F(0, 4, per, 5e4, per=1), F(3, 8, [0.0, 0.0, -2.0], 7e4, law=1, k2=3.0, tens=1, group=7), F(9, 11, D, 0.0, law=9, group=99),
             ACT(2, 0.3), ACT(0, -0.2)]
    oks, plan = _run(exe, calls)
    assert oks == [True] * 6  # (k == 0 removes: its other arguments are not looked at)
    k = np.zeros(NT)
    k[6:12], k[0:4], k[3:8], k[9:11] = 2e4, 5e4, 7e4, 0.0
    assert np.array_equal(plan["k"], k)
    dirs = plan["dir"].reshape(3, NT).T
    for t in range(NT):
        want = None if k[t] == 0 else [0.0, 0.0, -1.0] if 3 <= t < 8 else fm.unit(per[t]) if t < 3 else fm.unit(D)
        if want is None:
            assert not dirs[t].any()
        else:
            assert np.allclose(dirs[t], want, rtol=4e-16, atol=0) and abs(np.linalg.norm(dirs[t]) - 1.0) < 4e-16
    assert np.array_equal(plan["flags"], [0, 0, 0, 1, 1, 1, 1, 1, 2, 0, 0, 2])  # exp is flag 1 (its tension-only bit is not set), tensiononly 2
    assert np.array_equal(plan["group"], [0, 0, 0, 7, 7, 7, 7, 7, 2, 0, 0, 2])
    assert np.array_equal(plan["k2"], [0, 0, 0, 3, 3, 3, 3, 3, 0, 0, 0, 0])
    fib = [t for t in range(NT) if k[t] > 0]
    assert plan["nF"] == len(fib) and np.array_equal(plan["fibTet"], fib) and np.all(np.diff(plan["fibTet"]) > 0)
    assert np.array_equal(plan["groupOf"], plan["group"][fib]) and np.array_equal(plan["flagsF"], plan["flags"][fib]) and np.array_equal(plan["k2F"], plan["k2"][fib])
    assert np.array_equal(plan["volK"], VOL[fib] * k[fib])
    b = plan["b"].reshape(3, len(fib)).T
    for i, t in enumerate(fib):
        assert np.array_equal(b[i], fm.b_from(A[:, t], dirs[t]))  # the restatement the mp reference uses: the same bits
        assert np.allclose(b[i], A[:, t].reshape(3, 3, order="F") @ dirs[t], rtol=1e-13, atol=1e-13 * np.abs(A[:, t]).max())
    act = np.zeros(64)
    act[2], act[0] = 0.3, -0.2
    assert np.array_equal(plan["act"], act) and np.array_equal(plan["l0"], 1.0 - act)


def test_removing_everything_and_a_zero_volume(exe):
    oks, plan = _run(exe, [F(0, NT, D, 1e4), F(0, NT, None, 0.0)])
    assert oks == [True, True] and plan["nF"] == 0 and plan["nT"] == NT and not plan["dir"].any()
    vol = VOL.copy()
    vol[4] = 0.0
    oks, plan = _run(exe, [F(2, 7, D, 1e4)], vol=vol)
    assert np.array_equal(plan["fibTet"], [2, 3, 5, 6])  # an element without rest volume carries no fibre energy: left out of the lists
