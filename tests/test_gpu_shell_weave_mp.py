"""The woven-cloth kernels of the shells through the C ABI against the mpmath cases of shell_weave_mp.py (tests/golden/shell_weave_mp_cases.npz).  Every case is
one connected component of ONE carrier mesh without tetrahedra (node ranges side by side), so each case's energy terms, gradient rows and dense block are its
own; the tolerance is shell_weave_mp.tolerance = M (sens + u scale), derived there and pinned on the CPU by test_shell_weave_mp.py."""
import numpy as np
import pytest

import codim_common as cc
import shell_mp as smp
import shell_weave_mp as wmp

pytestmark = pytest.mark.gpu

COEFS = (1.0, 0.025 ** 2)
NO_T = np.zeros((0, 4), dtype=np.int32)


def dense_upper(c):
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A


class Carrier:
    def __init__(self, gpu_lib, cases, bend_scale=1.0, weave=True, fabric=None):
        self.cases = cases
        self.off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cases])]).astype(int)
        # (the cases stay where they are, overlapping in space -- there is no contact here, only elasticity)
        self.X = np.vstack([c["X"] for c in cases])
        self.x = np.vstack([c["x"] for c in cases])
        self.tri = np.vstack([c["tri"] + o for c, o in zip(cases, self.off)]).astype(np.int32)
        self.triOwner = np.concatenate([np.full(len(c["tri"]), i) for i, c in enumerate(cases)])
        cat = self.cat = lambda k: np.concatenate([c[k] for c in cases])
        self.dbc, self.woven = cat("dbc"), cat("woven")
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(self.X, NO_T, YM=1e5, PR=0.3, density=1000.0)
        c.set_shell(self.tri, cat("h"), cat("YM"), cat("PR"), cat("rho"), bend_scale=bend_scale)
        if weave:
            f = {k: cat(k) for k in ("E1", "E2", "G12", "nu12")} if fabric is None else fabric
            c.set_shell_weave(self.woven, cat("dir"), f["E1"], f["E2"], f["G12"], f["nu12"])
        for typ in (1, 2):
            if np.any(self.dbc == typ):
                c.set_dbc(np.flatnonzero(self.dbc == typ), typ)
        c.opt_init(0.01, False)
        c.set_pattern()
        c.set_positions(self.x)
        c.set_xtilde(self.x)


@pytest.fixture(scope="module")
def carrier(gpu_lib):
    return Carrier(gpu_lib, wmp.load())


def test_energy_gradient_hessian_and_state_against_mpmath(carrier):
    c, cases, off = carrier.c, carrier.cases, carrier.off
    worst, bad = {}, []
    got = c.shell_weave_get()
    assert np.array_equal(got["woven"], carrier.woven) and not got["a"][carrier.woven == 0].any() and not got["const4"][carrier.woven == 0].any()
    for t in np.flatnonzero(carrier.woven == 1):
        cs = cases[carrier.triOwner[t]]
        k = t - np.flatnonzero(carrier.triOwner == carrier.triOwner[t])[0]
        a = wmp.warp_in_plane(wmp.NP, cs["X"][cs["tri"][k]].tolist(), cs["dir"][k].tolist())
        assert np.allclose(got["a"][t], a, rtol=0, atol=1e-14)
        assert np.allclose(got["const4"][t], [float(v) for v in wmp.moduli(*[float(cs[q][k]) for q in ("E1", "E2", "G12", "nu12")])], rtol=1e-14, atol=0)
    perTri = c.shell_weave_energy_per_elem()
    assert np.all(perTri[carrier.woven == 0] == 0.0) and np.all(np.isfinite(perTri))
    state = c.shell_weave_state()
    assert state.shape == (len(carrier.tri), 6) and np.all(state[carrier.woven == 0] == 0.0)
    cc.compare(wmp, cases, "S", lambda i: state[carrier.triOwner == i], 1.0, True, worst, bad, "state")
    on = carrier.woven == 1
    assert np.all(np.abs(np.linalg.norm(state[on, 3:], axis=1) - 1.0) <= 8 * wmp.U)  # the warp direction is a unit vector
    for coef in COEFS:
        cc.compare(wmp, cases, "E", lambda i: coef * perTri[carrier.triOwner == i].sum(), coef, True, worst, bad, f"coef {coef:g}")
        E = c.shell_weave_energy(coef)
        want, tol = sum(wmp.expected(cs, "E", coef)[0] for cs in cases), sum(wmp.expected(cs, "E", coef)[1] for cs in cases)
        print(f"coef {coef:g}: total {E:.17g}, mpmath {want:.17g}, err / tol {abs(E - want) / tol:.3g}")
        assert abs(E - want) <= tol
        for proj in (True, False):
            g = c.shell_weave_gradient_add(coef, proj)
            c.set_zero()
            c.shell_weave_hessian_add(coef, proj)
            A = dense_upper(c)
            where = f"coef {coef:g} projectDBC {int(proj)}"
            cc.compare(wmp, cases, "g", lambda i: g[3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            cc.compare(wmp, cases, "H", lambda i: A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]], coef, proj, worst, bad, where)
            dropped = np.repeat((carrier.dbc == 1) | ((carrier.dbc == 2) & proj), 3)
            assert np.all(g[dropped] == 0.0) and np.all(A[dropped, :] == 0.0) and np.all(A[:, dropped] == 0.0)
            for i in range(len(cases)):  # nothing between the components
                A[3 * off[i]:3 * off[i + 1], 3 * off[i]:3 * off[i + 1]] = 0.0
            assert np.all(A == 0.0)
    print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) + f" (M = {wmp.M:g})")
    assert not bad, "\n".join(bad)
    st = {cs["name"]: i for i, cs in enumerate(cases)}
    p, m = state[carrier.triOwner == st["direction d"]][0], state[carrier.triOwner == st["direction -d"]][0]
    assert np.array_equal(p[:3], m[:3]) and np.array_equal(p[3:], -m[3:])  # d and -d: the same law, bit for bit; the reported direction turns round
    assert perTri[carrier.triOwner == st["direction d"]][0] == perTri[carrier.triOwner == st["direction -d"]][0]


def test_state_is_nan_where_a_yarn_has_no_length(carrier):
    c = carrier.c
    x = carrier.x.copy()
    i = [cs["name"] for cs in carrier.cases].index("stretch along warp")
    x[carrier.off[i]:carrier.off[i + 1]] = [0.25, 0.5, 0.75]  # collapsed to a point
    c.set_positions(x)
    try:
        s = c.shell_weave_state()[carrier.triOwner == i][0]
        others = c.shell_weave_state()[carrier.triOwner != i]
        E = c.shell_weave_energy_per_elem()[carrier.triOwner == i][0]
    finally:
        c.set_positions(carrier.x)
    assert s[0] == -0.5 and s[1] == -0.5 and np.all(np.isnan(s[2:])) and np.all(np.isfinite(others))
    assert np.isfinite(E) and E > 0.0  # the law is a polynomial: finite on a collapsed triangle


def test_term_alone_is_the_shell_with_it_minus_the_shell_without(gpu_lib):
    """two triangles sharing an edge, one StVK and one woven, with bending on: ipcgpu_shell_* of this context minus ipcgpu_shell_* of a context whose woven triangle
    carries a weave of vanishing moduli (its StVK constants are zeroed all the same, the hinge factor is 1 in both) is what ipcgpu_shell_weave_* return"""
    case = {cs["name"]: cs for cs in wmp.load()}["StVK and woven triangle sharing an edge"]
    lift = dict(case, x=case["x"] + np.outer([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.2]))  # out of the plane: the hinge carries energy
    tiny = {"E1": 1e-300, "E2": 1e-300, "G12": 1e-300, "nu12": 0.0}
    full, rest = Carrier(gpu_lib, [lift]).c, Carrier(gpu_lib, [lift], fabric=tiny).c
    assert np.all(full.shell_weave_get()["hingeFactor"] == 1.0) and np.array_equal(full.shell_energy_per_elem()[0], rest.shell_energy_per_elem()[0])
    assert full.shell_energy_per_elem()[0][1] == 0.0 and full.shell_energy_per_elem()[1][0] > 0.0  # no StVK energy on the woven triangle; the hinge is bent
    u64 = 64 * wmp.U
    for coef in COEFS:
        Ef, Er, Ew = full.shell_energy(coef), rest.shell_energy(coef), full.shell_weave_energy(coef)
        assert Ew > 0.0 and abs((Ef - Er) - Ew) <= u64 * Ef and rest.shell_weave_energy(coef) <= 1e-290
        assert Ew == coef * full.shell_weave_energy_per_elem()[1] or abs(Ew - coef * full.shell_weave_energy_per_elem()[1]) <= 2 * wmp.U * Ew
        for proj in (True, False):
            gf, gr, gw = full.shell_gradient_add(coef, proj), rest.shell_gradient_add(coef, proj), full.shell_weave_gradient_add(coef, proj)
            assert np.abs(gw).max() > 0 and np.abs((gf - gr) - gw).max() <= u64 * np.abs(gf).max()
            mats = []
            for ctx, fn in ((full, "shell_hessian_add"), (rest, "shell_hessian_add"), (full, "shell_weave_hessian_add")):
                ctx.set_zero()
                getattr(ctx, fn)(coef, proj)
                mats.append(ctx.get_a())
            assert np.abs(mats[2]).max() > 0 and np.abs((mats[0] - mats[1]) - mats[2]).max() <= u64 * np.abs(mats[0]).max()
    # the stepper's assembly carries the term: its gradient is the shell's (xTilde = x: the inertia term adds nothing to it)
    coef = COEFS[1]
    g = full.assemble_newton(coef, True, with_gradient=True)
    gs = full.shell_gradient_add(coef, True)
    assert np.abs(g - gs).max() <= u64 * np.abs(gs).max()


def test_strip_with_65_woven_triangles_of_130(gpu_lib):
    """2 x 66 nodes, 130 triangles, every "up" triangle woven: 65 lanes, one more than a wave of the 64-wide assemble kernel.  Every coordinate is dyadic, so each up
    triangle has bit for bit the edge vectors of the stored single triangle: the reference is that case assembled 65 times"""
    up = {cs["name"]: cs for cs in wmp.load()}["strip, up triangle"]
    V, tri = smp.grid(66, 2, spacing=wmp.STRIP_H)
    assert len(tri) == 130 and np.array_equal(V[tri[0]], up["X"])
    x = V @ wmp.STRIP_MAP.T
    woven = (np.arange(130) % 2 == 0).astype(np.int32)
    assert woven.sum() == 65
    c = gpu_lib.Context(0)
    c.set_mesh(V, NO_T, YM=1e5, PR=0.3, density=1000.0)
    c.set_shell(tri, up["h"][0], up["YM"][0], 0.3, 1000.0, bend_scale=1.0)
    c.set_shell_weave(woven, wmp.STRIP_DIR, up["E1"][0], up["E2"][0], up["G12"][0], up["nu12"][0])
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_positions(x)
    n3 = 3 * len(V)
    coef = COEFS[1]
    Ew = Et = 0.0
    gw, gt, Hw, Ht = np.zeros(n3), np.zeros(n3), np.zeros((n3, n3)), np.zeros((n3, n3))
    for t in np.flatnonzero(woven):
        idx = np.array([3 * v + i for v in tri[t] for i in range(3)])
        Ew, Et = Ew + wmp.expected(up, "E", coef)[0], Et + wmp.expected(up, "E", coef)[1]
        gw[idx] += wmp.expected(up, "g", coef)[0]
        gt[idx] += wmp.expected(up, "g", coef)[1]
        Hw[np.ix_(idx, idx)] += wmp.expected(up, "H", coef)[0]
        Ht[np.ix_(idx, idx)] += wmp.expected(up, "H", coef)[1]
    perTri = c.shell_weave_energy_per_elem()
    assert np.all(perTri[1::2] == 0.0) and len(set(perTri[0::2])) == 1 and perTri[128] > 0.0
    state = c.shell_weave_state()
    Sw, St = wmp.expected(up, "S")
    assert np.all(state[1::2] == 0.0) and np.all(np.abs(state[0::2] - Sw[0]) <= St[0]) and len({tuple(r) for r in state[0::2]}) == 1
    E = c.shell_weave_energy(coef)
    g = c.shell_weave_gradient_add(coef, True)
    c.set_zero()
    c.shell_weave_hessian_add(coef, True)
    A = dense_upper(c)
    print(f"strip: energy err / tol {abs(E - Ew) / Et:.3g}, gradient {np.max(wmp.ratio(g - gw, gt)):.3g}, "
          f"matrix {np.max(wmp.ratio(A - np.triu(Hw), np.triu(Ht))):.3g} of the tolerance")
    assert abs(E - Ew) <= Et
    assert np.all(np.abs(g - gw) <= gt)
    assert np.all(np.abs(A - np.triu(Hw)) <= np.triu(Ht))
    assert np.any(g[-3:] != 0.0)  # the last node belongs to the last woven triangle (128), the 65th lane


@pytest.mark.parametrize("d", [(1.0, 0.0, 0.0), (0.3, -1.0, 0.4)])
def test_isotropic_weave_is_the_plain_stvk_shell(gpu_lib, d):
    """E1 = E2 = E, nu12 = nu, G12 = E / (2 (1 + nu)) on every triangle against a context that never made the call: energy, gradient and matrix agree within the sum
    of the two restatements' tolerances (shell_weave_mp's for the woven one, shell_mp's for the StVK one), whatever the direction"""
    geo = {cs["name"]: cs for cs in wmp.load()}["tilted rest triangle, rotated and stretched"]
    E, nu = 1e5, 0.3
    iso = wmp._case("isotropic", geo["X"], geo["x"], d=d, E1=E, E2=E, G12=E / (2 * (1 + nu)), nu12=nu)
    iso.update(wmp.evaluate(iso))
    stvk = smp._case("StVK", geo["X"], geo["x"], [[0, 1, 2]], h=0.01, YM=E, PR=nu)
    stvk.update(smp.evaluate(stvk))
    a, b = Carrier(gpu_lib, [iso]).c, Carrier(gpu_lib, [iso], weave=False).c
    assert a.shell_energy_per_elem()[0][0] == 0.0 and b.shell_weave_energy(1.0) == 0.0
    for coef in COEFS:
        tol = lambda k: np.asarray(wmp.tolerance(iso, k, coef)) + np.asarray(smp.tolerance(stvk, k, coef))
        Ea, Eb = a.shell_energy(coef), b.shell_energy(coef)
        ga, gb = a.shell_gradient_add(coef, False), b.shell_gradient_add(coef, False)
        mats = []
        for ctx in (a, b):
            ctx.set_zero()
            ctx.shell_hessian_add(coef, False)
            mats.append(dense_upper(ctx))
        print(f"direction {d}, coef {coef:g}: energy {abs(Ea - Eb) / tol('E'):.3g}, gradient {np.max(np.abs(ga - gb) / tol('g')):.3g}, "
              f"matrix {np.max(np.abs(mats[0] - mats[1]) / tol('H')):.3g} of the summed tolerance")
        assert Eb > 0 and abs(Ea - Eb) <= tol("E")
        assert np.all(np.abs(ga - gb) <= tol("g"))
        assert np.all(np.abs(mats[0] - mats[1]) <= tol("H"))
