"""ipcgpu_elastic_stress under the stable neo-Hookean energy against the mpmath Cauchy stress of snh_mp.py (sigma = mu c F F^T / J + k I), per element and nodal, at
snh_mp's tolerance M (sens + u scale) per entry; inverted elements are finite and uncounted; two calls give the same bits."""
import math

import numpy as np
import pytest

import snh_mp as smp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    return [c for c in smp.load(prefix="e_") if smp.stress_checked(c)]


def _context(gpu_lib, lay):
    V, F, X = smp.carrier(lay)
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=0.0, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    smp.configure(c, lay, set_dbc=False)
    c.set_positions(X)
    return c


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_stress_per_element_and_nodal(gpu_lib, pool, n):
    inverted = [c for c in pool if c["ref_S"][7] < 0]
    assert len(inverted) >= 4
    lay = [pool[t % len(pool)] for t in range(n)]
    lay[n - 1] = inverted[n % len(inverted)]  # the last lane of the layout is an inverted element
    c = _context(gpu_lib, lay)
    elem, node, bad = c.elastic_stress()
    elem2, node2, bad2 = c.elastic_stress()
    assert bad == 0 and bad2 == 0
    assert np.array_equal(elem, elem2) and np.array_equal(node, node2)
    worst = 0.0
    for t, cs in enumerate(lay):
        assert np.all(np.isfinite(elem[t])), cs["name"]
        r = smp.ratio(cs, "S", elem[t])
        worst = max(worst, r)
        assert r <= smp.M, (cs["name"], r)
        if cs["YM"] == 0.0:
            assert np.all(elem[t, :7] == 0.0)
        # isolated tets: the mean over one element is that element's tensor (vol s / vol: at most two roundings), the von Mises stress that of the mean
        vol = float(smp.deformation(cs["Xr"], cs["X"])[2])
        for k in range(4):
            assert np.all(np.abs(node[4 * t + k, :6] - elem[t, :6]) <= 4 * smp.U * np.abs(elem[t, :6]))
            assert abs(node[4 * t + k, 6] - elem[t, 6]) <= 64 * smp.U * max(np.abs(elem[t, :6]).max(), abs(elem[t, 6]))
            assert abs(node[4 * t + k, 7] - vol) <= 1e-9 * vol
    print(f"n = {n}: worst err / (sens + u scale) = {worst:.3g} (M = {smp.M:g})")
    c.close()


def test_nodal_mean_on_the_block(gpu_lib):
    """the 48-tet block: nodal values against math.fsum of the device's own element records weighted by the rest volumes (4 n u sum |t_i|, as for NH / FCR), the
    element records against mp"""
    import elastic_mp as emp
    Z = np.load(emp.GOLDEN)
    V, F, X = Z["m_V"], Z["m_F"], Z["m_X"]
    cases = smp.load(prefix="b_")
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    c.set_positions(X)
    elem, node, bad = c.elastic_stress()
    assert bad == 0
    for t, cs in enumerate(cases):
        assert smp.ratio(cs, "S", elem[t]) <= smp.M, cs["name"]
    vol = c.features()["triArea"]  # (the rest volumes the device weights with)
    for v in range(len(V)):
        ts = [t for t in range(len(F)) if v in F[t]]
        w = math.fsum(vol[t] for t in ts)
        for k in range(6):
            terms = [vol[t] * elem[t, k] for t in ts]
            assert abs(node[v, k] - math.fsum(terms) / w) <= 4 * len(ts) * smp.U * math.fsum(abs(x) for x in terms) / w
        assert abs(node[v, 7] - w) <= 4 * len(ts) * smp.U * w
    c.close()
