"""The plastic-flow kernel through `ipcgpu_plastic_update`, element by element against the mpmath reference of plastic_mp.py: every case as a one-tet mesh, and
the cases tiled over carrier meshes of isolated tets at nT = 63, 64, 65 and 257 (wave and workgroup edges) with a range in the middle switched off.
Tolerance: plastic_mp.reference -- M (sens + u |A|_max), pinned on the CPU by test_plastic_mp.py.  The reference is evaluated from the doubles the GPU holds
(its own restTriInv), once per distinct case, and shared."""
import numpy as np
import pytest

import plastic_mp as pm

pytestmark = pytest.mark.gpu

CASES = pm.cases()
_REFS = {}


def ref_of(i, A):
    """the reference of case i at the GPU's A (the same rest shape gives the same A: computed once)"""
    key = (i, A.tobytes())
    if key not in _REFS:
        _REFS[key] = pm.reference(CASES[i], A=A, seed=i)
    return _REFS[key]


class Carrier:
    """a context on a mesh of isolated tets, case idx[t] on tet t, under SNH (finite for the inverted cases); off: a range whose plasticity is switched off"""

    def __init__(self, gpu_lib, idx, off=(0, 0)):
        self.idx, self.n, self.off = list(idx), len(idx), off
        lay = [CASES[i] for i in self.idx]
        V = np.concatenate([c["Xr"] for c in lay])
        self.X = np.concatenate([c["X"] for c in lay])
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(V, np.arange(4 * self.n, dtype=np.int32).reshape(-1, 4), YM=pm.YM, PR=pm.PR, density=pm.DENSITY)
        c.set_energy_type("SNH")
        c.opt_init(0.01, False)
        c.set_positions(self.X)
        t = 0
        while t < self.n:  # runs of equal parameters in one call
            e = t
            key = lambda k: (lay[k]["yield"], lay[k]["creep"], lay[k]["harden"])
            while e < self.n and key(e) == key(t):
                e += 1
            c.set_plasticity((t, e), *key(t))
            t = e
        if off[1] > off[0]:
            c.set_plasticity(off, pm.INF)
        self.alpha0 = np.array([cs["alpha"] for cs in lay])
        c.plastic_set_state(alpha=self.alpha0)
        f = c.features()
        self.A9, self.vol = f["restTriInv"].copy(), f["triArea"].copy()
        self.dts = sorted({cs["dt"] for cs in lay})

    def is_off(self, t):
        return self.off[0] <= t < self.off[1] or not CASES[self.idx[t]]["yield"] < pm.INF

    def flow(self):
        """one flow per distinct dt, each over the elements of that dt alone (the others switched off for the call); the counters summed"""
        c, ny, ns = self.c, 0, 0
        for dt in self.dts:
            for t in range(self.n):
                cs = CASES[self.idx[t]]
                if len(self.dts) > 1 and not self.is_off(t):
                    c.set_plasticity((t, t + 1), cs["yield"] if cs["dt"] == dt else pm.INF, cs["creep"], cs["harden"])
            a, b = c.plastic_update(dt)
            ny, ns = ny + a, ns + b
        for t in range(self.n):  # the parameters as they were
            cs = CASES[self.idx[t]]
            if len(self.dts) > 1 and not self.is_off(t):
                c.set_plasticity((t, t + 1), cs["yield"], cs["creep"], cs["harden"])
        return ny, ns

    def check(self, energy=False):
        c = self.c
        assert np.array_equal(c.plastic_get()["restTriInv0"], self.A9) and np.array_equal(c.plastic_get()["alpha"], self.alpha0)
        pe0, _ = c.plastic_state()
        ny, ns = self.flow()
        A1, al1 = c.features()["restTriInv"], c.plastic_get()["alpha"]
        assert np.all(np.isfinite(A1)) and np.all(np.isfinite(al1))  # (dilation: n = 0 divides nothing)
        lo = hi = skipped = 0
        worst, bad = 0.0, []
        E = c.elastic_energy_per_elem() if energy else None
        for t, i in enumerate(self.idx):
            cs, name = CASES[i], CASES[i]["name"]
            A = pm.to3(self.A9[t])
            if self.is_off(t):
                assert np.array_equal(A1[t], self.A9[t]) and al1[t] == self.alpha0[t], name  # switched off: the bits stay
                assert pe0[t, 1] == pm.INF
                continue
            r = ref_of(i, A)
            skipped += r["skipped"]
            lo += r["yielded"] and r["decided"]
            hi += r["yielded"] or not r["decided"]
            assert pe0[t, 1] == cs["yield"] + cs["harden"] * cs["alpha"] and pe0[t, 2] == cs["alpha"], name
            assert np.isnan(pe0[t, 0]) if r["skipped"] else abs(pe0[t, 0] - r["n"]) <= pm.DECIDE, (name, pe0[t, 0], r["n"])
            if r["decided"] and not r["yielded"]:
                assert np.array_equal(A1[t], self.A9[t]) and al1[t] == self.alpha0[t], name  # below yield or skipped: not a bit is written
            errA, errAl = np.abs(pm.to3(A1[t]) - r["A1"]), abs(al1[t] - r["alpha1"])
            worst = max(worst, float((errA / r["tolA"]).max()) * pm.M)
            if not (np.all(errA <= r["tolA"]) and errAl <= r["tolAlpha"]):
                bad.append(f"tet {t} {name}: |A' - ref| / tol = {float((errA / r['tolA']).max()):.3g}, |alpha' - ref| = {errAl:.3g} (tol {r['tolAlpha']:.3g})")
            if energy:
                Er, Et = pm.energy_reference(cs["X"], r, self.vol[t], seed=i)
                if not abs(E[t] - Er) <= Et:
                    bad.append(f"tet {t} {name}: E {E[t]!r} vs {Er!r}, tol {Et:.3g}")
        print(f"nT {self.n}: worst |A' - ref| / (sens + u scale) = {worst:.3g} (M = {pm.M:g}); yielded {ny} in [{lo}, {hi}], skipped {ns}")
        assert not bad, "\n".join(bad)
        assert lo <= ny <= hi and ns == skipped  # exact where the reference decides
        pe1, tot = c.plastic_state()
        assert np.array_equal(pe1[:, 2], al1) and tot[2] == al1.max() and abs(tot[3] - float(np.sum(self.vol * al1))) <= 1e-13 * float(np.sum(np.abs(self.vol) * al1)) + 1e-300
        if len(self.dts) == 1:
            assert (tot[0], tot[1]) == (ny, ns)
        # the same state once more gives the same bits; reset restores A0 to the bit
        c.plastic_reset()
        assert np.array_equal(c.features()["restTriInv"], self.A9) and np.all(c.plastic_get()["alpha"] == 0.0)
        c.plastic_set_state(alpha=self.alpha0)
        assert self.flow() == (ny, ns)
        assert np.array_equal(c.features()["restTriInv"], A1) and np.array_equal(c.plastic_get()["alpha"], al1)
        assert np.array_equal(c.plastic_state()[1], tot)
        c.plastic_reset()
        assert np.array_equal(c.features()["restTriInv"], self.A9)
        c.close()


def test_every_case_as_a_one_tet_mesh(gpu_lib):
    for i in range(len(CASES)):
        Carrier(gpu_lib, [i]).check(energy=True)


@pytest.mark.parametrize("nT", [63, 64, 65, 257])
def test_cases_tiled_with_a_range_switched_off(gpu_lib, nT):
    idx = [(5 * t + 1) % len(CASES) for t in range(nT)]  # (5 and the case count are coprime: every case appears)
    assert len(set(idx)) == len(CASES)
    Carrier(gpu_lib, idx, off=(nT // 3, nT // 3 + 7)).check(energy=(nT == 63))
