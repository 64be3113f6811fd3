"""The air-drag kernels through the C ABI against the mpmath cases of aero_mp.py (tests/golden/aero_mp_cases.npz).  Every case is a node range and an
aerodynamic surface of its own in ONE carrier mesh without tetrahedra (ranges side by side), so each case's energy terms, gradient rows and dense block are
its own.  The rest positions of the carrier are the cases' X (the lagged records are the stored ones, to the bit), the current positions their x.  Wind,
density and dt are the context's, not a surface's: the carrier is evaluated once per environment (w, rho, dt) the cases name -- one context per dt --, and
in every environment EVERY case is compared: its stored results in its own environment, results evaluated on the spot (a few dozen mpmath operations) in
the others.  The tolerance is aero_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_aero_mp.py."""
import numpy as np
import pytest

import aero_mp as am
import codim_common as cc

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)


class Carrier:
    def __init__(self, gpu_lib, cases, dt):
        self.cases, self.dt = cases, dt
        self.off = off = np.concatenate([[0], np.cumsum([len(c["x"]) for c in cases])]).astype(int)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.dbc = np.concatenate([c["dbc"] for c in cases])
        self.tris = [np.asarray(c["tri"], dtype=np.int32) + o for c, o in zip(cases, off)]
        self.owner = np.concatenate([np.full(len(t), i) for i, t in enumerate(self.tris)])
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_aero(self.tris, [cs["cn"] for cs in cases], [cs["ct"] for cs in cases], [bool(cs["one"]) for cs in cases])
        for typ in (1, 2):
            c.set_dbc(np.flatnonzero(self.dbc == typ), typ)
        c.opt_init(dt, False)
        c.set_pattern()
        c.set_positions(self.x)
        c.set_xtilde(self.x)

    def dense_upper(self):
        ia, ja = self.c.get_pattern()
        A = np.zeros((len(ia) - 1, len(ia) - 1))
        A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = self.c.get_a()
        return A


@pytest.fixture(scope="module")
def stored():
    return am.load()


@pytest.fixture(scope="module")
def carriers(gpu_lib, stored):
    return {dt: Carrier(gpu_lib, stored, dt) for dt in sorted({e[2] for e in am.environments(stored)})}


def test_lagged_records_and_lists_are_the_stored_ones(carriers, stored):
    for car in carriers.values():
        lag = car.c.aero_state(with_force=False)[1]
        assert np.array_equal(lag, np.vstack([c["lag"] for c in stored]))  # the plan's documented order, to the bit
        info = car.c.aero_get()
        assert info["n"] == len(stored) and info["nTri"] == len(car.owner) and np.array_equal(info["tri"], np.vstack(car.tris))
        assert np.array_equal(info["cn"], [c["cn"] for c in stored]) and np.array_equal(info["ct"], [c["ct"] for c in stored])
        assert np.array_equal(info["oneSided"], [bool(c["one"]) for c in stored]) and np.all(info["wind"] == 0) and info["density"] == 1.225


def test_energy_gradient_hessian_and_state_against_mpmath(carriers, stored):
    worst, bad = {}, []
    for env in am.environments(stored):
        w, rho, dt = env
        car = carriers[dt]
        c, off = car.c, car.off
        c.aero_set_wind(w, rho)
        assert np.array_equal(c.aero_get()["wind"], w) and c.aero_get()["density"] == rho
        cases = [am.in_environment(cs, env) for cs in stored]
        where0 = f"wind {w} rho {rho:g} dt {dt:g}"
        per = c.aero_energy_per_elem()
        F, lag, tot = c.aero_state()
        assert np.all(np.isfinite(per)) and np.all(np.isfinite(F)) and np.all(np.isfinite(tot))
        for i, cs in enumerate(cases):  # the per-triangle terms one by one: each within its case's energy tolerance
            assert np.all(np.abs(per[car.owner == i] - cs["perE"]) <= am.expected(cs, "E")[1]), (cs["name"], where0)
        cc.compare(am, cases, "F", lambda i: F[car.owner == i], 1.0, True, worst, bad, where0)
        # the totals: the per-case tolerances add up; the fixed-order sums add (nTri + 16) u of the magnitudes at the most
        nT = len(per)
        sumF = sum(cs["F"].sum(axis=0) for cs in cases)
        tolF = sum(am.expected(cs, "F")[1].sum(axis=0) for cs in cases) + am.U * (nT + 16) * np.abs(F).sum(axis=0)
        power, tolP = sum(cs["power"] for cs in cases), sum(am.expected(cs, "power")[1] for cs in cases)
        on = np.concatenate([am.reference(am.NP, cs, env=env)["on"] for cs in stored])  # (the float64 flags: at u = 0 mpmath sees a rounding, the kernel an exact zero)
        area = lag[on, 3].sum()
        print(f"{where0}: total force {tot[:3]} (reference {sumF}, tolerance {tolF}), power {tot[3]!r} ({power!r}, {tolP:.3g}), loaded area {tot[4]!r} ({area!r})")
        assert np.all(np.abs(tot[:3] - sumF) <= tolF) and abs(tot[3] - power) <= tolP + am.U * (nT + 16) * abs(power) and tot[3] >= 0.0
        assert abs(tot[4] - area) <= am.U * (nT + 16 + 4) * area
        assert np.array_equal(F, c.aero_state()[0]) and np.array_equal(tot, c.aero_state()[2])  # two calls, the same bits
        for coef in COEFS:
            Eall = c.aero_energy(coef)
            assert Eall == c.aero_energy(coef)  # the same bits
            Esum, Etol = sum(am.expected(cs, "E", coef)[0] for cs in cases), sum(am.expected(cs, "E", coef)[1] for cs in cases)
            print(f"{where0} coef {coef:g}: total energy {Eall!r}, reference {Esum!r}, tolerance {Etol:.3g}")
            assert abs(Eall - Esum) <= Etol
            cc.compare(am, cases, "E", lambda i: coef * per[car.owner == i].sum(), coef, True, worst, bad, f"{where0} coef {coef:g}")
            for proj in (True, False):
                g = c.aero_gradient_add(coef, proj)
                c.set_zero()
                c.aero_hessian_add(coef, proj)
                A = car.dense_upper()
                where = f"{where0} coef {coef:g} projectDBC {int(proj)}"
                cc.compare(am, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
                cc.compare(am, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
                dropped = np.repeat((car.dbc == 1) | ((car.dbc == 2) & proj), 3)
                assert dropped.any() and np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)  # dropped rows: exactly zero
                for i, cs in enumerate(cases):
                    s = slice(3 * off[i], 3 * off[i + 1])
                    own = (tuple(float(v) for v in cs["w"]), float(cs["rho"]), float(cs["dt"])) == env
                    if own and cs["name"] in ("u = 0", "one-sided, leeward"):  # these write nothing at all, and what they return is finite: exact zeros
                        assert np.all(g[s] == 0.0) and np.all(A[s, s] == 0.0) and np.all(per[car.owner == i] == 0.0) and np.all(F[car.owner == i] == 0.0), cs["name"]
                    if own and cs["name"] == "one-sided, exactly at u_n = 0":  # the normal part is exactly zero: n = e_z, so no z entry is written
                        assert np.all(g[s].reshape(-1, 3)[:, 2] == 0.0) and np.all(A[s, s][2::3, :] == 0.0) and np.all(A[s, s][:, 2::3] == 0.0) and np.any(A[s, s] != 0.0)
                    A[s, s] = 0.0  # ... and nothing between the cases
                assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {am.M:g})")
    assert not bad, "\n".join(bad)


def test_pattern_holds_every_block(carriers):
    car = next(iter(carriers.values()))
    ia, ja = car.c.get_pattern()
    P = np.zeros((len(ia) - 1, len(ia) - 1), dtype=bool)
    P[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = True
    for t in np.vstack(car.tris):  # the three diagonal and three upper off-diagonal blocks of every triangle
        for a in t:
            for b in t:
                if a <= b:
                    assert np.all(P[3 * a:3 * a + 3, 3 * b:3 * b + 3][np.triu(np.ones((3, 3), dtype=bool)) if a == b else np.ones((3, 3), dtype=bool)])


def test_more_than_one_block_of_lanes(gpu_lib):
    """a strip of 2 x 150 quads, 600 triangles: three workgroups of 256 lanes, the last one partly filled; energy, state and gradient sums against the
    float64 restatement per triangle (each of its terms is within the per-triangle tolerance checked above; here the REDUCTIONS are under test)"""
    nx = 150
    P = np.array([[i * 0.01, j * 0.01, 0.002 * np.sin(0.3 * i + j)] for i in range(nx + 1) for j in range(3)])
    idx = lambda i, j: i * 3 + j
    tri = np.array([t for i in range(nx) for j in range(2) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))], dtype=np.int32)
    assert len(tri) == 600
    dt, w = 0.01, np.array([0.5, -1.0, 2.0])
    x = P + dt * 0.3 * np.random.default_rng(2).standard_normal(P.shape)
    c = gpu_lib.Context(0)
    c.set_mesh(P, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_aero([tri], 1.28, 0.1, False)
    c.opt_init(dt, False)
    c.set_pattern()
    c.set_positions(x)
    c.aero_set_wind(w, 1.225)
    case = {"x": x, "tri": tri, "lag": am.rest_records(P, tri), "cn": 1.28, "ct": 0.1, "one": 0, "w": w, "rho": 1.225, "dt": dt}
    assert np.array_equal(c.aero_state(with_force=False)[1], case["lag"])
    r = am.reference(am.NP, case)
    per, (F, _, tot) = c.aero_energy_per_elem(), c.aero_state()
    # (the restatement forms u exactly as the kernel does -- sums, one division, one subtraction: nothing to contract --, so only what follows u differs, by
    # contraction and the order of a few sums: 64 u of the terms' magnitudes covers a few dozen operations)
    m = am.reference(am.NP, case, magnitudes=True)
    refPer, refF = np.array(r["per"]), np.array(r["F"])
    assert np.all(np.abs(per - refPer) <= 64 * am.U * np.array(m["per"])) and np.all(np.abs(F - refF) <= 64 * am.U * np.array(m["F"]).max(axis=1)[:, None])
    E = c.aero_energy(1.0)
    assert abs(E - per.sum()) <= am.U * (len(per) + 16) * np.abs(per).sum() and E == c.aero_energy(1.0)
    assert np.all(np.abs(tot[:3] - F.sum(axis=0)) <= am.U * (len(per) + 16) * np.abs(F).sum(axis=0)) and abs(tot[4] - case["lag"][:, 3].sum()) <= am.U * 620 * tot[4]
    g = c.aero_gradient_add(1.0, True).reshape(-1, 3)
    # the nodal forces sum to the total force (atomic sums: any order, |sum| within n u of the magnitudes)
    assert np.all(np.abs(-g.sum(axis=0) - tot[:3]) <= am.U * 4 * len(per) * np.abs(F).sum(axis=0))
    c.aero_hessian_add(1.0, True)  # every block is in the pattern (IPCGPU_ERR_STATE otherwise)
