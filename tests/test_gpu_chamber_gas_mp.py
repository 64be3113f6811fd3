"""The gas law's device quantities -- V, gauge, beta, W, the gradient and u_c = gradV_c -- through the C ABI against the mpmath states of chamber_gas_mp.py
(tests/golden/chamber_gas_mp_cases.npz).  ONE context holds three chambers: a 12-triangle cube (constant), a 320-triangle icosphere (gas, gamma 1.4: two
slices with a ragged tail) and a 20-triangle icosahedron (gas, gamma 1), so the gas chambers' ranges start off every wave and slice boundary.  States:
rest, a random perturbation, a uniform compression to V = 0.3 V0, a translation by 1e3.

Tolerance: chamber_gas_mp.tolerance = M (sens + u scale), M = 1 the next power of two above the float64 NumPy restatement's worst ratio, 0.688
(test_chamber_gas_mp.py pins it).  The device's worst ratios, measured on an MI355X and printed by test_state_energy_gradient_against_mpmath:
V 0.037, gauge 0.068, beta 0.076, W 0.023, u 0.386, g 0.248.

V, gauge, beta, W, the energies and the per-triangle energies are bit-identical between two calls and between two contexts, and a context whose
chambers are all constant gives the same bits with and without chamber_set_gas(zeros).  The gradient and u_c are sums of fp64 atomics in the one triangle
kernel there is (k_chamber_assemble<false>: a second copy of it is ruled out), so they repeat to rounding, 64 u of the largest entry, not to the bit."""
import numpy as np
import pytest

import chamber_gas_mp as gm
import codim_common as cc

pytestmark = pytest.mark.gpu


def make_context(gpu_lib, X, ch, gas=True, call_set_gas=True):
    c = gpu_lib.Context(0)
    c.set_mesh(X, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_chambers([q["tri"] for q in ch], [q["p"] for q in ch])
    if call_set_gas:
        c.chamber_set_gas([q["gas"] and gas for q in ch], [q["ambient"] for q in ch], [q["gamma"] for q in ch])
    c.opt_init(0.01, False)
    c.set_pattern()
    return c


def outputs(c, x, n):
    c.set_positions(x)
    vol, gauge, beta = c.chamber_gas_state()
    return [vol, gauge, beta, np.array([c.chamber_energy(1.0), c.chamber_energy(0.025 ** 2)]), c.chamber_energy_per_elem(), c.chamber_gradient_add(1.0, False)] \
        + [c.chamber_volume_gradient(i, False) for i in range(n)]


@pytest.fixture(scope="module")
def setup(gpu_lib):
    X, ch, off = gm.scene()
    return X, ch, off, make_context(gpu_lib, X, ch), gm.load()


def test_state_energy_gradient_against_mpmath(setup):
    X, ch, off, c, stored = setup
    got = c.chamber_gas_get()
    assert got["isGas"].tolist() == [0, 1, 1] and np.array_equal(got["fillVolume"], [q["V0"] for q in ch])  # the rest volume, to the bit (chamber_plan.h)
    worst, bad = {}, []
    for name, x, refs in stored:
        c.set_positions(x)
        vol, gauge, beta = c.chamber_gas_state()
        assert gauge[0] == ch[0]["p"] and beta[0] == 0.0  # the constant chamber
        per = c.chamber_energy_per_elem()
        end = np.cumsum([len(q["tri"]) for q in ch])
        g = c.chamber_gradient_add(1.0, False)
        for i, ref in refs.items():
            s = slice(3 * off[i], 3 * off[i + 1])
            u = c.chamber_volume_gradient(i, False)
            assert np.all(u[:s.start] == 0.0) and np.all(u[s.stop:] == 0.0)
            # W_c as the sum of the per-triangle shares W_c V_t / V_c.  Each share carries the rounding of its own V_t, quotient and product on top of W_c's
            # error: 4 u |W| Vmag / V in all (Vmag = scale_V bounds sum |V_t|), which is taken off before the ratio
            W = per[end[i] - len(ch[i]["tri"]):end[i]].sum()
            shareErr = 4 * gm.U * abs(ref["W"]) * ref["scale_V"] / ref["V"]
            dev = dict(V=vol[i], gauge=gauge[i], beta=beta[i], W=W, u=u[s], g=g[s])
            for k in gm.QUANT:
                own = ref if k not in ("u", "g") else {k: ref[k][s], "sens_" + k: ref["sens_" + k][s], "scale_" + k: ref["scale_" + k]}  # (stored over all nodes)
                assert k not in ("u", "g") or (np.all(np.delete(ref[k], np.arange(s.start, s.stop)) == 0.0) and np.abs(own[k]).max() > 0)
                err = np.abs(np.asarray(dev[k]) - np.asarray(own[k]))
                r = gm.ratio(np.maximum(err - shareErr, 0.0) if k == "W" else err, own, k)
                worst[k] = max(worst.get(k, 0.0), r)
                print(f"{name} chamber {i} {k}: err / (sens + u scale) {r:.3g}")
                if not r <= gm.M:
                    bad.append(f"{name} chamber {i} {k}: ratio {r:.3g} over M = {gm.M:g}")
        # the energy entry point: the constant chamber's -p V plus the gas chambers' W, each within its tolerance (the cube's: 16 (sens + u scale) of
        # chamber_mp, here bounded by 16 u |p| Vmag with Vmag <= the cube's bounding volume about r_c)
        E = c.chamber_energy(1.0)
        Egas = sum(ref["W"] for ref in refs.values())
        tol = sum(float(gm.tolerance(ref, "W")) for ref in refs.values())
        Ecube = per[:end[0]].sum()
        assert abs((E - Ecube) - Egas) <= tol + 4 * gm.U * (abs(Ecube) + abs(E)), (name, E, Ecube, Egas, tol)
    print("worst err / (sens + u scale) on the device: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (M = {gm.M:g})")
    assert not bad, "\n".join(bad)


def test_projected_dirichlet_entries_are_dropped(gpu_lib):
    X, ch, off = gm.scene()
    c = gpu_lib.Context(0)
    c.set_mesh(X, cc.NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_chambers([q["tri"] for q in ch], [q["p"] for q in ch])
    c.chamber_set_gas([q["gas"] for q in ch], [q["ambient"] for q in ch], [q["gamma"] for q in ch])
    held = np.array([off[1] + 3, off[2] + 1])
    c.set_dbc(held, 2)  # (type 2: projected with projectDBC only, so the unprojected call shows what is dropped)
    c.opt_init(0.01, False)
    c.set_pattern()
    for i in (1, 2):
        u, full = c.chamber_volume_gradient(i, True), c.chamber_volume_gradient(i, False)
        drop = np.zeros(len(u), dtype=bool)
        drop[np.repeat(3 * held, 3) + np.tile(np.arange(3), len(held))] = True
        # (the kept entries are atomic sums: equal to rounding, not to the bit)
        assert np.all(u[drop] == 0.0) and np.allclose(u[~drop], full[~drop], rtol=0, atol=64 * gm.U * np.abs(full).max()) and np.abs(full[drop]).max() > 0


def test_bits_repeat_between_calls_and_between_contexts(setup, gpu_lib):
    X, ch, off, c, stored = setup
    other = make_context(gpu_lib, X, ch)
    for name, x, _ in stored[1:3]:
        a, b, d = outputs(c, x, 3), outputs(c, x, 3), outputs(other, x, 3)
        # (the gradient sums by atomics, entry by entry; here every entry's addends come from one chamber's triangles in a race -- it is compared to
        # rounding, everything else to the bit)
        for i, (p, q, r) in enumerate(zip(a, b, d)):
            if i == 5 or i >= 6:
                assert np.allclose(p, q, rtol=0, atol=64 * gm.U * np.abs(p).max()) and np.allclose(p, r, rtol=0, atol=64 * gm.U * np.abs(p).max()), (name, i)
            else:
                assert np.array_equal(p, q) and np.array_equal(p, r), (name, i)


def test_all_constant_chambers_ignore_set_gas_with_zeros(gpu_lib):
    X, ch, off = gm.scene()
    x = gm.states(X, ch, off)["perturbed"]
    a = outputs(make_context(gpu_lib, X, ch, gas=False, call_set_gas=True), x, 3)
    b = outputs(make_context(gpu_lib, X, ch, gas=False, call_set_gas=False), x, 3)
    for i, (p, q) in enumerate(zip(a[:5], b[:5])):  # state, energies, per-triangle energies: no atomics, to the bit
        assert np.array_equal(p, q), i
    for p, q in zip(a[5:], b[5:]):
        assert np.allclose(p, q, rtol=0, atol=64 * gm.U * np.abs(p).max())
