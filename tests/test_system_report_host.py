"""Host side of the system report (`ipcgpu_opt_system_report`): the slice-list builder of `ipc_amd/csrc/report_plan.cpp`, run as a stand-alone program
(`tests/report_plan/main.cpp`), and the report writer behind `tools/run_scene.py --report`, run on a stub backend.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from ipc_amd import scene_script as ss

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIDTH = 256  # the slice width HipOptimizer::ensureReportPlan asks for


@pytest.fixture(scope="module")
def planner():
    exe = os.path.join(HERE, "report_plan", "_build", "report_plan_main")
    csrc = os.path.join(ROOT, "ipc_amd", "csrc")
    srcs = [os.path.join(HERE, "report_plan", "main.cpp"), os.path.join(csrc, "report_plan.cpp")]
    deps = srcs + [os.path.join(csrc, "report_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{csrc}"] + srcs + ["-o", exe])

    def run(cases):
        """cases: [(width, n, ends)] -> per case None (rejected) or (slices[k, 3], start[nComp + 1])"""
        text = "".join(f"{w} {n} {len(e)} {' '.join(str(int(x)) for x in e)}\n" for w, n, e in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        res = []
        for line, (_w, _n, e) in zip(out, cases):
            a = [int(x) for x in line.split()]
            if a[0] == 0:
                res.append(None)
                continue
            k = a[1]
            assert len(a) == 2 + 3 * k + len(e) + 1
            res.append((np.array(a[2:2 + 3 * k], dtype=np.int64).reshape(k, 3), np.array(a[2 + 3 * k:], dtype=np.int64)))
        return res
    return run


def check_tiling(n, ends, width, slices, start):
    """every index of [0, n) in exactly one slice, in order; no slice wider than `width`, empty, or across a component end; start = a component's slices"""
    ends = np.asarray(ends, dtype=np.int64)
    begins = np.concatenate([[0], ends[:-1]])
    at = 0
    for c, b, e in slices:
        assert b == at and b < e <= b + width, (c, b, e, at)
        assert begins[c] <= b and e <= ends[c], (c, b, e)
        at = e
    assert at == n
    assert len(start) == len(ends) + 1 and start[0] == 0 and start[-1] == len(slices)
    for c in range(len(ends)):
        assert np.all(slices[start[c]:start[c + 1], 0] == c)
        assert start[c + 1] - start[c] == -(-(ends[c] - begins[c]) // width)  # ceil: no component takes more slices than it needs


def test_slices_tile_random_component_tables(planner):
    rng = np.random.default_rng(20240611)
    sizes_pool = [0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 729, 1000]
    cases = [(WIDTH, 0, [0]), (WIDTH, 0, [0, 0, 0]), (WIDTH, 256, [256]), (WIDTH, 257, [0, 257]), (WIDTH, 255, [255, 255]), (1, 5, [2, 2, 5]), (7, 50, [50])]
    for _ in range(200):
        nc = int(rng.integers(1, 12))
        sizes = rng.choice(sizes_pool, nc) if rng.random() < 0.7 else rng.integers(0, 1500, nc)
        ends = np.cumsum(sizes)
        cases.append((WIDTH if rng.random() < 0.8 else int(rng.integers(1, 600)), int(ends[-1]), ends.tolist()))
    res = planner(cases)
    for (w, n, ends), r in zip(cases, res):
        assert r is not None, (n, ends)
        check_tiling(n, ends, w, *r)


def test_invalid_tables_are_rejected(planner):
    bad = [(WIDTH, 10, [5, 4, 10]),  # decreasing
           (WIDTH, 10, [5, 9]),  # last entry below n
           (WIDTH, 10, [5, 11]),  # ... above n
           (WIDTH, 10, [-1, 10]),  # negative
           (WIDTH, 10, [])]  # no component
    assert planner(bad) == [None] * len(bad)


class StubBackend:
    """system_report() of a backend with 3 components: values that need all 17 digits, signed zeros, tiny and huge magnitudes"""

    def __init__(self):
        self.calls = 0
        rng = np.random.default_rng(7)
        self.frames = []
        for k in range(4):
            E = rng.standard_normal(3) * 10.0 ** rng.integers(-300, 300, 3)
            M = rng.standard_normal((3, 3)) / 3.0
            L = rng.standard_normal((3, 3)) * 1e-17
            if k == 0:
                M[:], L[:] = 0.0, -0.0
                E[1] = np.nextafter(1.0, 2.0)
            self.frames.append((E, M, L))

    def system_report(self):
        self.calls += 1
        return self.frames[self.calls - 1]


def test_report_writer_round_trips_through_loadtxt(tmp_path):
    be = StubBackend()
    w = ss.ReportWriter(str(tmp_path / "rep"))
    for _ in be.frames:
        w.write(be)
    for i, name in enumerate(("sysE.txt", "sysM.txt", "sysL.txt")):
        a = np.loadtxt(tmp_path / "rep" / name, ndmin=2)
        want = np.array([np.asarray(f[i]).ravel() for f in be.frames])  # component-major, xyz adjacent
        assert a.shape == want.shape == (4, 3 if i == 0 else 9)
        assert a.tobytes() == want.tobytes() or np.array_equal(a, want)  # the same doubles (loadtxt may turn -0.0 into 0.0: equal, not the same bits)
        assert np.array_equal(a, want)
    # one component: a line holds one value (E) or three (M, L) and still loads
    class One:
        def system_report(self):
            return np.array([0.1]), np.array([[0.1, 0.2, 0.3]]), np.array([[1e-5, -2.5, 1 / 3]])
    w = ss.ReportWriter(str(tmp_path / "one"))
    w.write(One())
    w.write(One())
    assert np.array_equal(np.loadtxt(tmp_path / "one" / "sysE.txt", ndmin=2), [[0.1], [0.1]])
    assert np.array_equal(np.loadtxt(tmp_path / "one" / "sysL.txt", ndmin=2), [[1e-5, -2.5, 1 / 3]] * 2)


def test_apply_hands_components_to_a_backend_that_takes_them():
    """scene_script.apply passes the accumulated component ends right after set_mesh -- and only to a backend that has set_components"""
    src = open(os.path.join(ROOT, "ipc_amd", "scene_script.py")).read()
    body = src[src.index("def apply(sc, be):"):]
    assert body.index("be.set_mesh(") < body.index('hasattr(be, "set_components")') < body.index("be.set_components(sc.node_ranges[1:], sc.tet_ranges[1:])") < body.index("be.opt_init(")
