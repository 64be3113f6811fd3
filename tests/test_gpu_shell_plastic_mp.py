"""The shells' plastic-flow kernels through ipcgpu_shell_plastic_update / _state against the mpmath reference of shell_plastic_mp.py.  Every case is one
connected component of ONE carrier mesh without tetrahedra (node ranges side by side; there is no contact here): single triangles for the membrane flow,
pairs of triangles over one hinge for the hinge flow.  The reference takes the doubles the library holds (B, the two StVK constants, thetaBar, g) as its
inputs; the tolerances are shell_plastic_mp's: sens + M U scale."""
import numpy as np
import pytest

import shell_plastic_mp as spm

pytestmark = pytest.mark.gpu

INF = float("inf")
NO_T = np.zeros((0, 4), dtype=np.int32)
DT = 0.01


class Carrier:
    """tri cases (one triangle each) first, then hinge cases (two triangles each); per-case parameters through one range call per case"""

    def __init__(self, gpu_lib, tcases, hcases):
        self.tcases, self.hcases = tcases, hcases
        X, x, tri, h, nu = [], [], [], [], []
        off = 0
        for c in tcases:
            X.append(c["Xr"]); x.append(c["X"]); tri.append(np.array([[0, 1, 2]]) + off); h.append(c["thickness"]); nu.append(c["nu"])
            off += 3
        for c in hcases:
            X.append(c["Xr"]); x.append(c["X"]); tri.append(spm.HINGE_TRI + off); h += [c["thickness"]] * 2; nu += [0.3] * 2
            off += 4
        self.X, self.x, self.tri = np.vstack(X), np.vstack(x), np.vstack(tri).astype(np.int32)
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, np.array(h), 1e5, np.array(nu), 1000.0, bend_scale=1.0)
        c.opt_init(DT, False)
        c.set_positions(self.x)
        nt = len(tcases)
        for i, cs in enumerate(tcases):
            assert cs["dt"] in (DT, 0.1, 0.025)
            c.shell_set_plasticity((i, i + 1), cs["yield"], INF, cs["creep"], cs["harden"])
        for j, cs in enumerate(hcases):
            c.shell_set_plasticity((nt + 2 * j, nt + 2 * j + 2), INF, cs["yield"], cs["creep"], cs["harden"])
        self.sh = c.shell_get()
        assert self.sh["nHinge"] == len(hcases) and np.array_equal(self.sh["hinges"][:, 0], 3 * nt + 4 * np.arange(len(hcases)))

    def start(self, dt):
        """history of the cases (alpha, alphaB), records at rest; -> the state before the flow"""
        c = self.c
        c.shell_plastic_reset()
        c.shell_plastic_set_state(alpha=[cs["alpha"] for cs in self.tcases] + [0.0] * (2 * len(self.hcases)), alphaB=[cs["alpha"] for cs in self.hcases])
        return c.shell_plastic_get()


def _by_dt(cases):
    out = {}
    for i, c in enumerate(cases):
        out.setdefault(c["dt"], []).append(i)
    return out


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, spm.tri_cases(), spm.hinge_cases())


def _ratio(err, tol):
    err, tol = np.atleast_1d(np.abs(err)).astype(float).ravel(), np.atleast_1d(tol).astype(float).ravel()
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, np.finfo(float).tiny))))


def test_flows_and_state_against_mpmath(carrier):
    """every dt of the cases is its own update from the same start; the cases of another dt are checked in their own pass"""
    c, tcases, hcases = carrier.c, carrier.tcases, carrier.hcases
    nt = len(tcases)
    worst = {"B": 0.0, "alpha": 0.0, "n": 0.0, "ratio": 0.0, "thetaBar": 0.0, "alphaB": 0.0, "eps": 0.0}
    for dt in sorted(set(cs["dt"] for cs in tcases + hcases)):
        g0 = carrier.start(dt)
        assert np.array_equal(g0["B"], g0["B0"]) and np.array_equal(g0["thetaBar"], g0["thetaBar0"])
        pt0, ph0, _ = c.shell_plastic_state()
        counts = c.shell_plastic_update(dt)
        g1 = c.shell_plastic_get()
        pt1, ph1, tot = c.shell_plastic_state()
        assert np.array_equal(g1["triConst"][:, 4:], g0["triConst"][:, 4:])  # h A mu, h A lambda_ps: never written
        assert np.array_equal(tot[:4], counts)
        exp_counts, undecided = np.zeros(4, dtype=int), np.zeros(4, dtype=int)
        for i, cs in enumerate(tcases):
            k = (g0["triConst"][i, 4], g0["triConst"][i, 5])
            ref = spm.tri_reference(dict(cs, dt=dt), B=spm.to2(g0["B"][i]), k=k, seed=i)
            name = f"{cs['name']} (dt {dt:g})"
            B1 = spm.to2(g1["B"][i])
            worst["B"] = max(worst["B"], _ratio(B1 - ref["B1"], ref["tolB"]))
            worst["alpha"] = max(worst["alpha"], _ratio(g1["alpha"][i] - ref["alpha1"], ref["tolAlpha"]))
            assert _ratio(B1 - ref["B1"], ref["tolB"]) <= 1.0 and _ratio(g1["alpha"][i] - ref["alpha1"], ref["tolAlpha"]) <= 1.0, name
            # the state before the flow: n (also where the flow is off), y, alpha, the area ratio 1
            if np.isnan(ref["nState"]):
                assert np.isnan(pt0[i, 0]), name
            else:
                worst["n"] = max(worst["n"], _ratio(pt0[i, 0] - ref["nState"], ref["tolN"]))
                assert _ratio(pt0[i, 0] - ref["nState"], ref["tolN"]) <= 1.0, name
            assert pt0[i, 1] == ref["y"] and pt0[i, 2] == cs["alpha"] and pt0[i, 3] == 1.0, name
            # ... and after it: the area ratio det B0 / det B'
            worst["ratio"] = max(worst["ratio"], _ratio(pt1[i, 3] - ref["ratio"], ref["tolRatio"]))
            assert _ratio(pt1[i, 3] - ref["ratio"], ref["tolRatio"]) <= 1.0 and pt1[i, 2] == g1["alpha"][i], name
            wrote = not (np.array_equal(g1["B"][i], g0["B"][i]) and g1["alpha"][i] == g0["alpha"][i])
            exact_rest = "n = 0 = y exactly" in cs["name"]
            if ref["decided"] or exact_rest:
                assert wrote == ref["yielded"], name  # not a bit is written unless the triangle yields
                exp_counts[0] += ref["yielded"]
            else:
                undecided[0] += 1
            exp_counts[1] += ref["skipped"]
        for j, cs in enumerate(hcases):
            ref = spm.hinge_reference(dict(cs, dt=dt), thetaBar=g0["thetaBar"][j], g=g0["g"][j], seed=j)
            name = f"{cs['name']} (dt {dt:g})"
            assert g0["hingeYield"][j] == cs["yield"] and g0["hingeCreep"][j] == cs["creep"] and g0["hingeHarden"][j] == cs["harden"]
            for key, got, want, tol in (("thetaBar", g1["thetaBar"][j], ref["thetaBar1"], ref["tolTheta"]), ("alphaB", g1["alphaB"][j], ref["alphaB1"], ref["tolAlpha"])):
                worst[key] = max(worst[key], _ratio(got - want, tol))
                assert _ratio(got - want, tol) <= 1.0, (name, key, got, want, tol)
            if np.isnan(ref["eps"]) and cs["yield"] < INF:
                assert np.isnan(ph0[j, 0]), name
            elif cs["yield"] < INF:
                worst["eps"] = max(worst["eps"], _ratio(ph0[j, 0] - ref["eps"], ref["tolEps"]))
                assert _ratio(ph0[j, 0] - ref["eps"], ref["tolEps"]) <= 1.0, name
            assert ph0[j, 1] == ref["y"] and ph0[j, 2] == cs["alpha"] and ph0[j, 3] == 0.0, name
            assert ph1[j, 3] == g1["thetaBar"][j] - g0["thetaBar0"][j] and ph1[j, 2] == g1["alphaB"][j], name
            wrote = not (g1["thetaBar"][j] == g0["thetaBar"][j] and g1["alphaB"][j] == g0["alphaB"][j])
            if ref["decided"] or "eps = 0 = y" in cs["name"]:
                assert wrote == ref["yielded"], name
                exp_counts[2] += ref["yielded"]
            else:
                undecided[2] += 1
            exp_counts[3] += ref["skipped"]
        # the triangles of the hinge cases have no membrane flow; their records keep their bits
        assert np.array_equal(g1["B"][nt:], g0["B"][nt:]) and np.all(g1["alpha"][nt:] == 0.0)
        assert np.all(exp_counts <= counts) and np.all(np.asarray(counts) <= exp_counts + undecided), (counts, exp_counts, undecided)
        assert tot[4] == g1["alpha"].max() and tot[5] == g1["alphaB"].max()
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


def _strip(n_quads=150, seed=5):
    """a strip of 2 n_quads triangles in the plane z = 0, then stretched along x by a factor that varies along the strip and bent about y"""
    rng = np.random.default_rng(seed)
    nx = n_quads + 1
    X = np.array([[i * 0.1, j * 0.1, 0.0] for i in range(nx) for j in range(2)]) + np.pad(rng.uniform(-0.01, 0.01, (2 * nx, 2)), ((0, 0), (0, 1)))
    tri = np.array([t for i in range(n_quads) for t in ((2 * i, 2 * i + 2, 2 * i + 1), (2 * i + 1, 2 * i + 2, 2 * i + 3))], dtype=np.int32)
    s = 1.0 + 0.08 * rng.uniform(0.0, 1.0, nx).cumsum() / nx * 2.0  # stretch grows along the strip: the first part stays below yield
    xs = np.concatenate([[0.0], np.cumsum(0.1 * (0.96 + 0.1 * rng.uniform(0.0, 1.0, nx - 1)))])
    phi = 0.02 * np.arange(nx) ** 1.5 / nx ** 0.5  # curvature grows along the strip too
    x = X.copy()
    for i in range(nx):
        for j in range(2):
            v = 2 * i + j
            p = phi[i] + 0.05 * j * np.sin(1.3 * i)  # a twist between the two rows: the quads are not planar, their diagonal hinges bend too
            x[v] = [np.sin(p) * 2.0 + xs[i] * np.cos(p), X[v, 1] * (1.0 + 0.02 * (i % 3)), np.cos(p) * 2.0 - xs[i] * np.sin(p)]
    return X, x, tri


def test_random_strip_counters_untouched_records_and_determinism(gpu_lib):
    X, x, tri = _strip()
    nTri = len(tri)
    assert nTri == 300 and nTri > 256 and nTri % 64 != 0
    c = gpu_lib.Context(0)
    c.set_mesh(X, NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_shell(tri, 0.02, 1e5, 0.3, 1000.0, bend_scale=1.0)
    c.opt_init(DT, False)
    c.set_positions(x)
    sh = c.shell_get()
    nH = sh["nHinge"]
    c.shell_set_plasticity((0, nTri), 1.0, 1.0, 5.0, 0.5)  # far from yielding: only to read the records the reference starts from
    g = c.shell_plastic_get()
    n_ref = sorted(float(spm.tri_strain(x[tri[t]], spm.to2(g["B"][t]), g["triConst"][t, 4], g["triConst"][t, 5])[3]) for t in range(nTri))
    e_ref = sorted(float(g["g"][i] * abs(spm.hinge_theta(x[sh["hinges"][i]]) - g["thetaBar"][i])) for i in range(nH))
    # thresholds halfway between the two middle strains of the reference: about half of the strip yields, and every decision is far from rounding
    yld, yb = 0.5 * (n_ref[nTri // 2 - 1] + n_ref[nTri // 2]), 0.5 * (e_ref[nH // 2 - 1] + e_ref[nH // 2])
    c.shell_set_plasticity((0, nTri), yld, yb, 5.0, 0.5)
    c.shell_set_plasticity((nTri - 7, nTri), INF, INF, INF, 0.0)  # a range switched off again: its records keep their bits, its hinges do not flow
    runs = []
    for _ in range(2):
        c.shell_plastic_reset()
        g0 = c.shell_plastic_get()
        counts = c.shell_plastic_update(DT)
        runs.append((counts, c.shell_plastic_get()))
    (counts, g1), (counts2, g2) = runs
    assert counts == counts2
    for key in ("B", "alpha", "thetaBar", "alphaB"):
        assert np.array_equal(g1[key], g2[key]), key  # two runs agree to the bit
    refs = [spm.tri_reference(dict(X=x[tri[t]], B=None, k=None, **{"yield": g0["yield"][t]}, creep=g0["creep"][t], harden=g0["harden"][t], alpha=0.0, dt=DT),
                              B=spm.to2(g0["B"][t]), k=(g0["triConst"][t, 4], g0["triConst"][t, 5]), seed=t) for t in range(nTri)]
    href = [spm.hinge_reference(dict(X=x[sh["hinges"][i]], **{"yield": g0["hingeYield"][i]}, creep=g0["hingeCreep"][i], harden=g0["hingeHarden"][i], alpha=0.0, dt=DT),
                                thetaBar=g0["thetaBar"][i], g=g0["g"][i], seed=i) for i in range(nH)]
    assert all(r["decided"] for r in refs) and all(r["decided"] for r in href)  # (a median lies between two strains, 2^-40 from neither)
    want = (sum(r["yielded"] for r in refs), sum(r["skipped"] for r in refs), sum(r["yielded"] for r in href), sum(r["skipped"] for r in href))
    assert counts == want
    assert 0.35 * nTri < want[0] < 0.65 * nTri and 0.3 * nH < want[2] < 0.7 * nH and want[1] == 0 and want[3] == 0
    for t, r in enumerate(refs):
        if r["yielded"]:
            assert np.all(np.abs(spm.to2(g1["B"][t]) - r["B1"]) <= r["tolB"]) and abs(g1["alpha"][t] - r["alpha1"]) <= r["tolAlpha"], t
        else:
            assert np.array_equal(g1["B"][t], g0["B"][t]) and g1["alpha"][t] == 0.0, t  # untouched records keep their bits
    for i, r in enumerate(href):
        if r["yielded"]:
            assert abs(g1["thetaBar"][i] - r["thetaBar1"]) <= r["tolTheta"] and abs(g1["alphaB"][i] - r["alphaB1"]) <= r["tolAlpha"], i
        else:
            assert g1["thetaBar"][i] == g0["thetaBar"][i] and g1["alphaB"][i] == 0.0, i
    assert np.array_equal(g1["triConst"][:, 4:], g0["triConst"][:, 4:])
    # the mean rule on the device's side: a hinge next to the switched-off range does not flow
    off_tris = set(range(nTri - 7, nTri))
    tri_sets = [set(t) for t in tri.tolist()]
    for i in range(nH):
        pair = [t for t in range(nTri) if set(sh["hinges"][i][:2]) <= tri_sets[t]]
        assert (g0["hingeYield"][i] == INF) == bool(off_tris & set(pair)), i
