"""Hand-placed elastic elements and step-bound cases through the C ABI, each compared AT ITS OWN SCALE with the mpmath reference of elastic_mp.py (stored in
tests/golden/elastic_mp_cases.npz).  Every element is one tet of a mesh of isolated tets, so every gradient entry and every entry of a tet's 12 x 12 block
belongs to exactly one element.  Tolerance per quantity: M (sens + u scale), elastic_mp.tol -- derived there, pinned on the CPU by test_elastic_mp.py."""
import numpy as np
import pytest

import elastic_mp as emp
from stencil_mp import tet_blocks  # noqa: F401  (blocks() below is Placed's, which reads through it)
from test_gpu_stencils_mp import Placed

pytestmark = pytest.mark.gpu

ENERGIES = (emp.NH, emp.FCR)


@pytest.fixture(scope="module")
def elems():
    return emp.load(prefix="e_")


@pytest.fixture(scope="module")
def steps():
    return emp.load(prefix="s_")


class Carrier:
    """a context on the carrier mesh with element case lay[t] on tet t"""

    def __init__(self, gpu_lib, lay, energy, shared_apex=False):
        self.lay, self.n = lay, len(lay)
        V, F, X = emp.carrier(lay)
        if shared_apex:  # a fan: local node 0 of every tet is ONE node (the cases' node 0 sits at the origin at rest and now)
            assert all(np.all(c["Xr"][0] == 0.0) and np.all(c["X"][0] == 0.0) for c in lay)
            keep = np.array([0] + [4 * t + k for t in range(self.n) for k in (1, 2, 3)])
            V, X = V[keep], X[keep]
            F = np.array([[0, 1 + 3 * t, 2 + 3 * t, 3 + 3 * t] for t in range(self.n)], dtype=np.int32)
        self.V, self.F, self.X = V, F, X
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(V, F, YM=0.0, PR=0.4, density=emp.DENSITY)
        c.set_energy_type(emp.ENERGY_NAMES[energy])
        if shared_apex:
            for t, cs in enumerate(lay):
                c.set_component_material((1 + 3 * t, 4 + 3 * t), (t, t + 1), emp.DENSITY, float(cs["YM"]), float(cs["PR"]))
        else:
            emp.configure(c, lay)
        c.opt_init(0.01, False)
        c.set_pattern()
        c.set_positions(X)

    blocks = Placed.blocks  # per-tet 12 x 12 out of the upper CSR (isolated tets only)

    def upper(self):
        """dense upper triangle of the matrix"""
        ia, ja = self.c.get_pattern()
        A = np.zeros((len(ia) - 1, len(ia) - 1))
        A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = self.c.get_a()
        return A


class Misses:
    def __init__(self):
        self.bad, self.worst = [], {}

    def check(self, case, k, got, coef=1.0, proj=True, where="", newton=False):
        assert np.all(np.isfinite(got)), (case["name"], k, where)
        r = emp.hessian_ratio(case, got, coef, proj) if k == "H" else emp.ratio(case, k, got, coef, proj, newton)
        key = k + (" (clamp)" if emp.margin(case, k) != emp.M else "")
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        if not r <= emp.margin(case, k):
            self.bad.append(f"{case['name']} [{case['index']}] {k} {where}: err / (sens + u scale) = {r:.3g}")

    def done(self):
        print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())) + f" (M = {emp.M:g}, clamp {emp.M_CLAMP_H:g})")
        assert not self.bad, "\n".join(self.bad)


def check_dropped(case, proj, g, H):
    gn, hn = emp.dropped_nodes(case, proj)
    for k in gn:
        assert np.all(g[3 * k:3 * k + 3] == 0.0), case["name"]
    for k in hn:
        assert np.all(H[3 * k:3 * k + 3, :] == 0.0) and np.all(H[:, 3 * k:3 * k + 3] == 0.0), case["name"]


def inertia_diag(lay, proj, mass):
    """what assemble_newton adds to every tet's diagonal: the lumped mass (features()["mass"]), 1 on projected Dirichlet nodes"""
    D = np.zeros((len(lay), 12))
    for t, c in enumerate(lay):
        hn = emp.dropped_nodes(c, proj)[1]
        for k in range(4):
            D[t, 3 * k:3 * k + 3] = 1.0 if k in hn else mass[4 * t + k]
    return D, mass


def both_kernels(p, m, coef=1.0):
    """every tet of layout p: gradient and block from the tet-parallel atomic kernel and from the patch kernel, against the reference and against each other"""
    lay, c = p.lay, p.c
    c.set_xtilde(p.X)  # no inertia force: the patch kernel's gradient is the elastic one
    for proj in (True, False):
        g1 = c.elastic_gradient(coef, proj)
        c.set_zero()
        c.elastic_hessian_add(coef, proj)
        B1 = p.blocks()
        g2 = c.assemble_newton(coef, proj, with_gradient=True)
        B2 = p.blocks()
        D, mass = inertia_diag(lay, proj, c.features()["mass"])
        assert np.all(np.abs(mass - emp.mass_mp(p.V, len(lay))) <= 1e-9 * mass)  # (the rest volume of a sliver is a cancelling determinant)
        for t, cs in enumerate(lay):
            H2 = B2[t] - np.diag(D[t])
            hn = emp.dropped_nodes(cs, proj)[1]
            for k in hn:  # identity rows: exactly 1 on the diagonal, nothing else
                assert np.all(B2[t][3 * k:3 * k + 3, 3 * k:3 * k + 3] == np.eye(3))
            for g, H, nm in ((g1, B1[t], "tet-parallel"), (g2, H2, "patch")):
                gt = g[12 * t:12 * t + 12]
                m.check(cs, "g", gt, coef, proj, f"{nm} tet {t} projectDBC {proj}", newton=nm == "patch")  # (the Newton gradient is also cleared where rows are dropped)
                m.check(cs, "H", H, coef, proj, f"{nm} tet {t} projectDBC {proj}")
                check_dropped(cs, proj, gt, H)
                if cs["YM"] == 0.0:
                    assert np.all(gt == 0.0) and np.all(H == 0.0)
            live = np.repeat([k not in hn for k in range(4)], 3)
            assert np.all(np.abs(g1[12 * t:12 * t + 12] - g2[12 * t:12 * t + 12])[live] <= 2 * emp.tol(cs, "g", coef, proj)[live]) and np.all(g2[12 * t:12 * t + 12][~live] == 0.0), cs["name"]
            if not cs["ref_ambiguous"]:  # (where the entries depend on the SVD basis both kernels run the same code in the same order: they agree all the same)
                assert np.all(np.abs(B1[t] - H2) <= 2 * emp.tol(cs, "H", coef, proj) + 4 * emp.U * np.diag(D[t])), cs["name"]  # (+ the rounding of H + mass)
            else:
                assert np.all(np.abs(B1[t] - H2) <= 8 * emp.U * coef * cs["ref_Hscale"] + 4 * emp.U * np.diag(D[t])), cs["name"]


@pytest.mark.parametrize("energy", ENERGIES)
def test_energy(gpu_lib, elems, energy):
    lay = [c for c in elems if c["energy"] == energy]
    p = Carrier(gpu_lib, lay, energy)
    m = Misses()
    pe = p.c.elastic_energy_per_elem()
    for t, cs in enumerate(lay):
        m.check(cs, "E", pe[t])
    Eref = np.array([cs["ref_E"] for cs in lay])
    rng = np.random.default_rng(5)
    xt = p.X + 1e-3 * rng.normal(size=p.X.shape)
    mass = p.c.features()["mass"]
    from mpmath import mpf
    inertia = float(sum(mpf(float(mass[v])) * sum((mpf(float(p.X[v, i])) - mpf(float(xt[v, i]))) ** 2 for i in range(3)) for v in range(len(mass))) / 2)
    for coef in (1.0, 0.025 ** 2):
        bound = sum(emp.tol(cs, "E", coef) for cs in lay)
        E = p.c.elastic_energy(coef)
        print(f"coef {coef:g}: |E - sum E_mp| = {abs(E - coef * Eref.sum()):.3g}, bound {bound:.3g}")
        assert abs(E - coef * Eref.sum()) <= bound
        p.c.set_xtilde(p.X)
        assert abs(p.c.incremental_potential(coef) - coef * Eref.sum()) <= bound  # without inertia
        p.c.set_xtilde(xt)
        assert abs(p.c.incremental_potential(coef) - (coef * Eref.sum() + inertia)) <= bound + emp.M * emp.U * len(mass) * inertia
    p.c.close()
    m.done()


@pytest.mark.parametrize("energy", ENERGIES)
def test_gradient_and_hessian_of_every_case(gpu_lib, elems, energy):
    p = Carrier(gpu_lib, [c for c in elems if c["energy"] == energy], energy)
    m = Misses()
    both_kernels(p, m)
    p.c.close()
    m.done()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(gpu_lib, elems, n):
    """the cases drawn cyclically; the last tet of the layout (and lane 63 of every full wave) enters the Jacobi path of make_pd3 -- an indefinite A3 -- while its
    neighbours take the fast exit: a divergent wave.  Every tet is checked."""
    pool = [c for c in elems if c["energy"] == emp.NH and c["ref_negA3"] == 0 and c["YM"] > 0]
    jac = [c for c in elems if c["energy"] == emp.NH and c["ref_negA3"] > 0]
    lay = [pool[t % len(pool)] for t in range(n)]
    for t in list(range(63, n, 64)) + [n - 1]:
        lay[t] = jac[(t // 64) % len(jac)]
    p = Carrier(gpu_lib, lay, emp.NH)
    m = Misses()
    both_kernels(p, m, coef=0.5)
    p.c.close()
    m.done()


@pytest.mark.parametrize("n", [2, 17, 64])
def test_fan_of_tets_on_one_node(gpu_lib, elems, n):
    """n tets share their node 0: the reference of the shared node is the sum of the elements' mp contributions, its tolerance the sum of theirs; both kernels.
    Two patch assemblies of one state give the same bits (its order is fixed); nothing of the kind is claimed for the atomic kernel."""
    pool = [c for c in elems if c["energy"] == emp.NH and np.all(c["Xr"] == emp.UNIT) and c["YM"] > 0 and not c["dtype"].any() and not c["ref_ambiguous"]]
    assert len(pool) >= 17 and all(emp.tol(c, "H").max() <= 1e-9 * c["ref_Hscale"] for c in pool)  # the sum of the tolerances stays a tight bound
    lay = [pool[t % len(pool)] for t in range(n)]
    p = Carrier(gpu_lib, lay, emp.NH, shared_apex=True)
    c = p.c
    c.set_xtilde(p.X)
    G = np.array([cs["ref_g"] for cs in lay])
    H = np.array([cs["ref_H"] for cs in lay])
    gtol = sum(emp.tol(cs, "g")[:3] for cs in lay)
    Htol = sum(emp.tol(cs, "H")[:3, :3] for cs in lay)
    mass0 = float(c.features()["mass"][0])
    m = Misses()
    g1 = c.elastic_gradient(1.0, True)
    c.set_zero()
    c.elastic_hessian_add(1.0, True)
    A1 = p.upper()
    g2 = c.assemble_newton(1.0, True, with_gradient=True)
    A2, a2 = p.upper(), c.get_a()
    g3 = c.assemble_newton(1.0, True, with_gradient=True)
    assert np.array_equal(g2, g3) and np.array_equal(a2, c.get_a())
    A2[:3, :3] -= mass0 * np.eye(3)
    for g, A, nm in ((g1, A1, "tet-parallel"), (g2, A2, "patch")):
        err = np.abs(g[:3] - G[:, :3].sum(axis=0))
        print(f"n = {n} {nm}: apex gradient error / bound {err / gtol}")
        assert np.all(err <= gtol)
        assert np.all(np.triu(np.abs(A[:3, :3] - H[:, :3, :3].sum(axis=0)) <= Htol + 4 * emp.U * mass0 * np.eye(3)) == np.triu(np.ones((3, 3), dtype=bool)))
        for t, cs in enumerate(lay):  # the nine entries of the tet's own nodes and the blocks that couple them to the apex belong to this element alone
            own = np.arange(3 + 9 * t, 12 + 9 * t)
            got_g = np.concatenate([cs["ref_g"][:3], g[own]])
            got_H = cs["ref_H"].copy()
            got_H[:3, 3:] = A[:3, own]
            got_H[3:, :3] = A[:3, own].T
            blk = np.triu(A[np.ix_(own, own)])
            if nm == "patch":
                blk = blk - np.diag(np.repeat(c.features()["mass"][1 + 3 * t:4 + 3 * t], 3))
            got_H[3:, 3:] = blk + np.triu(blk, 1).T
            m.check(cs, "g", got_g, where=f"{nm} tet {t}")
            m.check(cs, "H", got_H, where=f"{nm} tet {t}")
    c.close()
    m.done()


def upper(c):
    """dense upper triangle of the matrix"""
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A


def test_block_of_tets(gpu_lib):
    """a 2 x 2 x 2 block of cells, 48 tets on 27 nodes: interior nodes and edges shared by many tets.  The reference is the sum of the per-element mp contributions,
    the tolerance the sum of theirs, for both kernels; two patch assemblies of one state give the same bits (nothing of the kind is claimed for the atomic kernel)."""
    Z = np.load(emp.GOLDEN)
    V, F, X = Z["m_V"], Z["m_F"], Z["m_X"]
    cases = emp.load(prefix="b_")
    assert len(cases) == len(F) == 48 and all(np.array_equal(cs["X"], X[f]) for cs, f in zip(cases, F))
    n = 3 * len(V)
    G, Gt, H, Ht = np.zeros(n), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    for cs, f in zip(cases, F):
        idx = np.array([3 * v + i for v in f for i in range(3)])
        G[idx] += cs["ref_g"]
        Gt[idx] += emp.tol(cs, "g")
        H[np.ix_(idx, idx)] += cs["ref_H"]
        Ht[np.ix_(idx, idx)] += emp.tol(cs, "H")
    assert Ht.max() <= 1e-8 * np.abs(H).max()
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=emp.DENSITY)
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_positions(X)
    c.set_xtilde(X)
    g1 = c.elastic_gradient(1.0, True)
    c.set_zero()
    c.elastic_hessian_add(1.0, True)
    A1 = upper(c)
    g2 = c.assemble_newton(1.0, True, with_gradient=True)
    A2, a2 = upper(c), c.get_a()
    g3 = c.assemble_newton(1.0, True, with_gradient=True)
    assert np.array_equal(g2, g3) and np.array_equal(a2, c.get_a())
    mass = np.repeat(c.features()["mass"], 3)
    A2 = A2 - np.diag(mass)
    up = np.triu(np.ones((n, n), dtype=bool))
    for g, A, nm in ((g1, A1, "tet-parallel"), (g2, A2, "patch")):
        eg, eh = np.abs(g - G) / Gt, (np.abs(A - H) / np.where(Ht > 0, Ht, 1.0))[up & (Ht > 0)]
        print(f"{nm}: worst error / summed tolerance: gradient {eg.max():.3g}, matrix {eh.max():.3g}")
        assert np.all(eg <= 1.0) and np.all(np.abs(A - H)[up] <= (Ht + (4 * emp.U * np.diag(mass) if nm == "patch" else 0.0))[up])
        assert np.all(A[up & (Ht == 0)] == 0.0)  # pairs of nodes that share no tet
    c.close()


def step_carrier(gpu_lib, n, placed):
    """n unit tets at rest; `placed` {tet: step case} puts a case's positions (as rest shape too) and search direction on that tet, every other p is 0"""
    V = np.tile(emp.UNIT, (n, 1))
    P = np.zeros((4 * n, 3))
    for t, cs in placed.items():
        V[4 * t:4 * t + 4] = cs["X"]
        P[4 * t:4 * t + 4] = cs["P"]
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.arange(4 * n, dtype=np.int32).reshape(n, 4), YM=1e5, PR=0.4, density=emp.DENSITY)
    c.opt_init(0.01, False)
    c.set_positions(V)
    return c, P


def test_step_bound_per_case(gpu_lib, steps):
    """each case alone on a carrier whose other tets do not move, at tet 0, at the last lane of a wave, at the first of the next and at the last tet of 257"""
    m = Misses()
    for tet, n in ((0, 1), (63, 65), (64, 65), (256, 257)):
        c, _ = step_carrier(gpu_lib, n, {})
        for cs in steps:
            X, P = np.tile(emp.UNIT, (n, 1)), np.zeros((4 * n, 3))
            X[4 * tet:4 * tet + 4], P[4 * tet:4 * tet + 4] = cs["X"], cs["P"]
            c.set_positions(X)
            got = c.filter_step_size(P.reshape(-1), float(cs["tmax"]))
            m.check(cs, "bound", got, where=f"tet {tet} of {n}")
            if cs["ref_root"] < 0 or cs["ref_root"] > cs["tmax"]:
                assert got == cs["tmax"], cs["name"]  # no root below tMax: the step comes back untouched
        c.close()
    m.done()


@pytest.mark.parametrize("tmax", [1.0, 0.3])
def test_step_bound_is_the_minimum_over_the_elements(gpu_lib, steps, tmax):
    cs_ = [cs for cs in steps if cs["tmax"] == tmax]
    c, P = step_carrier(gpu_lib, 70, {3 * k + 1: cs for k, cs in enumerate(cs_)})
    got = c.filter_step_size(P.reshape(-1), tmax)
    low = min(cs_, key=lambda cs: cs["ref_bound"])
    print(f"tMax {tmax}: {got!r}, the smallest reference {low['ref_bound']!r} ({low['name']})")
    assert emp.ratio(low, "bound", got) <= emp.M
    c.set_energy_type("FCR")  # no element-inversion safeguard under FCR: the step comes back untouched
    assert c.filter_step_size(P.reshape(-1), tmax) == tmax
    c.close()


def test_check_inversion(gpu_lib, elems):
    by = {c["name"]: c for c in elems}
    good = by["NH general"]
    flat = dict(good, X=good["X"].copy())
    flat["X"][3] = flat["X"][0] + 0.3 * (flat["X"][1] - flat["X"][0]) + 0.4 * (flat["X"][2] - flat["X"][0]) + 1e-12 * np.cross(flat["X"][1] - flat["X"][0], flat["X"][2] - flat["X"][0])
    inv = by["FCR inverted, s_2 -0.5"]
    for lay, want in (([good] * 64 + [flat], True), ([good] * 64 + [inv], False), ([inv] + [good] * 3, False), ([good] * 257, True)):
        p = Carrier(gpu_lib, lay, emp.NH)
        assert p.c.check_inversion() == want
        p.c.close()
