"""Host side of the contact report (`ipcgpu_contact_report`): the row plan of `ipc_amd/csrc/contact_report_plan.cpp` -- key encoding, row order, compaction
of a histogram, slice list -- run as a stand-alone program (`tests/contact_report_plan/main.cpp`), once more under the address and undefined-behaviour
sanitizers, and the writer behind `tools/run_scene.py --contact-report` on a stub backend.  No GPU."""
import os
import subprocess

import numpy as np

from ipc_amd import lib as ipclib
from ipc_amd import scene_script as ss

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "contact_report_plan", "main.cpp"), os.path.join(CSRC, "contact_report_plan.cpp"), os.path.join(CSRC, "report_plan.cpp")]
WIDTH = 256  # the slice width HipContact::contactReport asks for


def _build(name, extra):
    exe = os.path.join(HERE, "contact_report_plan", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "contact_report_plan.h"), os.path.join(CSRC, "report_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def expected_order(n_comp, n_half):
    """the rows in the order the interface specifies: ascending a; a's component rows b = a.., then its half-space rows, ascending h"""
    return [(a, b) for a in range(n_comp) for b in list(range(a, n_comp)) + [-1 - h for h in range(n_half)]]


def check_keys(out, n_comp, n_half):
    order = expected_order(n_comp, n_half)
    assert out[0] == len(order) == n_comp * (n_comp + 1) // 2 + n_comp * n_half
    body = np.array(out[1:1 + 3 * len(order)]).reshape(-1, 3)
    assert [tuple(r) for r in body[:, :2]] == order  # key k decodes to the k-th pair of the row order ...
    assert np.array_equal(body[:, 2], np.arange(len(order)))  # ... and that pair encodes to k
    assert out[-2:] == [0, 0]  # keys outside the range are refused


def parse_rows(a):
    n = a[0]
    rows = np.array(a[1:1 + 3 * n], dtype=np.int64).reshape(n, 3)
    k = a[1 + 3 * n]
    sl = np.array(a[2 + 3 * n:2 + 3 * n + 3 * k], dtype=np.int64).reshape(k, 3)
    start = np.array(a[2 + 3 * n + 3 * k:], dtype=np.int64)
    return rows, sl, start


def check_rows(a, n_comp, n_half, width, count):
    rows, sl, start = parse_rows(a)
    order = expected_order(n_comp, n_half)
    present = [k for k, c in enumerate(count) if c > 0]
    assert [tuple(r[:2]) for r in rows] == [order[k] for k in present]  # the rows present, in the specified order
    assert np.array_equal(rows[:, 2], np.cumsum([count[k] for k in present]))
    begins = np.concatenate([[0], rows[:-1, 2]]) if len(rows) else np.zeros(0, dtype=np.int64)
    at = 0
    for r, b, e in sl:  # every record in exactly one slice, none wider than `width`, none across a row's end
        assert b == at and b < e <= b + width and begins[r] <= b and e <= rows[r, 2], (r, b, e)
        at = e
    assert at == (rows[-1, 2] if len(rows) else 0)
    assert len(start) == len(rows) + 1 and start[0] == 0 and start[-1] == len(sl)
    for r in range(len(rows)):
        assert np.all(sl[start[r]:start[r + 1], 0] == r)
        assert start[r + 1] - start[r] == -(-(rows[r, 2] - begins[r]) // width)


def _cases():
    rng = np.random.default_rng(20250917)
    keys = [(nc, nh) for nc in range(1, 51) for nh in range(4)]
    hist = []
    pool = [0, 0, 0, 1, 255, 256, 257, 600]
    for nc, nh in [(1, 0), (1, 3), (2, 1), (4, 0), (7, 2), (50, 3)]:
        n = nc * (nc + 1) // 2 + nc * nh
        hist.append((nc, nh, WIDTH, [0] * n))  # nothing present: no rows
        hist.append((nc, nh, WIDTH, [pool[3 + (k % 5)] for k in range(n)]))  # every key present, every size of the list
        for _ in range(6):
            hist.append((nc, nh, WIDTH if rng.random() < 0.7 else int(rng.integers(1, 300)), rng.choice(pool, n).tolist()))
    return keys, hist


def _check_all(exe):
    keys, hist = _cases()
    for (nc, nh), out in zip(keys, _run(exe, [f"K {nc} {nh}" for nc, nh in keys])):
        check_keys(out, nc, nh)
    outs = _run(exe, [f"H {nc} {nh} {w} {len(c)} {' '.join(map(str, c))}" for nc, nh, w, c in hist])
    for (nc, nh, w, c), out in zip(hist, outs):
        check_rows(out, nc, nh, w, c)
    assert parse_rows(outs[0])[0].shape == (0, 3) and outs[0] == [0, 0, 0]  # the all-zero histogram: no row, no slice, one start


def test_keys_rows_and_slices():
    _check_all(_build("contact_report_plan_main", []))


def test_the_same_under_address_and_undefined_behaviour_sanitizers():
    _check_all(_build("contact_report_plan_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))


def test_a_thousand_components_fit_the_key_limit():
    out = _run(_build("contact_report_plan_main", []), ["H 1000 2 256 3 600 0 1"])[0]
    rows, sl, _ = parse_rows(out)
    assert [tuple(r) for r in rows] == [(0, 0, 600), (0, 2, 601)] and len(sl) == 4
    assert 1000 * 1001 // 2 + 1000 * 2 < 1 << 22


class StubBackend:
    """contact_report() of a backend: two calls, rows whose doubles need all 17 digits, an infinite minimum, a half-space row"""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.frames = []
        for n in (3, 0, 2):
            r = np.zeros(n, dtype=ipclib.CONTACT_REPORT_DTYPE)
            for k in ("FA", "FB", "TA", "TB", "RA", "RB"):
                r[k] = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-30, 30, (n, 3))
            r["W"] = -rng.random(n) / 3
            r["minD2"] = rng.random(n) * 1e-6
            r["a"], r["b"] = np.arange(n), np.arange(n) + 1
            r["nPT"], r["argmin"] = 5, 17
            if n == 3:
                r["b"][2], r["minD2"][1], r["argmin"][1] = -1, np.inf, -1
            self.frames.append(r)
        self.calls = 0

    def contact_report(self, x_prev=None, coef=None):
        assert coef == 0.25 and x_prev is not None
        self.calls += 1
        return self.frames[self.calls - 1]


def test_contact_report_writer_round_trips(tmp_path):
    be = StubBackend()
    w = ss.ContactReportWriter(str(tmp_path / "rep"), 0.25)
    for step in range(len(be.frames)):
        w.write(be, step + 1, x_prev=np.zeros((1, 3)))
    a = np.loadtxt(tmp_path / "rep" / "contact.txt", ndmin=2)
    want = []
    for step, fr in enumerate(be.frames):
        for r in fr:
            want.append([step + 1] + [r[k] for k in ("a", "b", "nPP", "nPE", "nPT", "nEE", "nMollified", "argmin", "minD2")]
                        + [v for k in ("FA", "FB", "TA", "TB", "RA", "RB") for v in r[k]] + [r["W"]])
    want = np.array(want, dtype=np.float64)
    assert a.shape == want.shape == (5, 29)
    assert np.array_equal(a, want)  # %.17g: the same doubles, inf included
