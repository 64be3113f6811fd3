"""The stable neo-Hookean energy (energy type 2, `SNH`) through the C ABI, element by element against the mpmath reference of snh_mp.py (stored in
tests/golden/snh_mp_cases.npz), built like test_gpu_elastic_mp.py: every case is one tet of a carrier mesh of isolated tets, so every gradient entry and every entry
of a tet's 12 x 12 block belongs to exactly one element.  Tolerance per quantity: M (sens + u scale), snh_mp.tol -- derived there, pinned on the CPU by
test_snh_mp.py.  Every case is compared entry by entry: the projection of this energy does not depend on the SVD's basis."""
import numpy as np
import pytest
from mpmath import mpf

import elastic_mp as emp
import snh_mp as smp
from test_gpu_stencils_mp import Placed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elems():
    return smp.load(prefix="e_")


class Carrier:
    """a context on the carrier mesh with element case lay[t] on tet t"""

    def __init__(self, gpu_lib, lay, energy="SNH", shared_apex=False):
        self.lay, self.n = lay, len(lay)
        V, F, X = smp.carrier(lay)
        if shared_apex:  # a fan: local node 0 of every tet is ONE node (the cases' node 0 sits at the origin at rest and now)
            assert all(np.all(c["Xr"][0] == 0.0) and np.all(c["X"][0] == 0.0) for c in lay)
            keep = np.array([0] + [4 * t + k for t in range(self.n) for k in (1, 2, 3)])
            V, X = V[keep], X[keep]
            F = np.array([[0, 1 + 3 * t, 2 + 3 * t, 3 + 3 * t] for t in range(self.n)], dtype=np.int32)
        self.V, self.F, self.X = V, F, X
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(V, F, YM=0.0, PR=0.4, density=smp.DENSITY)
        c.set_energy_type(energy)
        if shared_apex:
            for t, cs in enumerate(lay):
                c.set_component_material((1 + 3 * t, 4 + 3 * t), (t, t + 1), smp.DENSITY, float(cs["YM"]), float(cs["PR"]))
        else:
            smp.configure(c, lay)
        c.opt_init(0.01, False)
        c.set_pattern()
        c.set_positions(X)

    blocks = Placed.blocks  # per-tet 12 x 12 out of the upper CSR (isolated tets only)


def upper(c):
    """dense upper triangle of the matrix"""
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A


class Misses:
    def __init__(self):
        self.bad, self.worst = [], {}

    def check(self, case, k, got, coef=1.0, proj=True, where="", newton=False):
        assert np.all(np.isfinite(got)), (case["name"], k, where)
        r = smp.ratio(case, k, got, coef, proj, newton)
        self.worst[k] = max(self.worst.get(k, 0.0), r)
        if not r <= smp.M:
            self.bad.append(f"{case['name']} [{case['index']}] {k} {where}: err / (sens + u scale) = {r:.3g}")

    def done(self):
        print("worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())) + f" (M = {smp.M:g})")
        assert not self.bad, "\n".join(self.bad)


def check_dropped(case, proj, g, H):
    gn, hn = smp.dropped_nodes(case, proj)
    for k in gn:
        assert np.all(g[3 * k:3 * k + 3] == 0.0), case["name"]
    for k in hn:
        assert np.all(H[3 * k:3 * k + 3, :] == 0.0) and np.all(H[:, 3 * k:3 * k + 3] == 0.0), case["name"]


def both_kernels(p, m, coefs=(1.0,)):
    """every tet of layout p: gradient and block from the tet-parallel atomic kernel and from the patch kernel, projectDBC on and off, against the reference and
    against each other; two patch assemblies of one state give the same bits"""
    lay, c = p.lay, p.c
    c.set_xtilde(p.X)  # no inertia force: the patch kernel's gradient is the elastic one
    mass = c.features()["mass"]
    assert np.all(np.abs(mass - smp.mass_mp(p.V, len(lay))) <= 1e-9 * mass)
    for coef in coefs:
        for proj in (True, False):
            g1 = c.elastic_gradient(coef, proj)
            c.set_zero()
            c.elastic_hessian_add(coef, proj)
            B1 = p.blocks()
            g2 = c.assemble_newton(coef, proj, with_gradient=True)
            B2, a2 = p.blocks(), c.get_a()
            g3 = c.assemble_newton(coef, proj, with_gradient=True)
            assert np.array_equal(g2, g3) and np.array_equal(a2, c.get_a())
            for t, cs in enumerate(lay):
                hn = smp.dropped_nodes(cs, proj)[1]
                D = np.concatenate([np.full(3, 1.0 if k in hn else mass[4 * t + k]) for k in range(4)])
                H2 = B2[t] - np.diag(D)
                # the patch kernel stores fl(H_ii + m): one rounding of a sum of size m + |H_ii|, which no tolerance of H knows about (at coef 0.025^2 the mass of
                # the 1e2-edge tet is 1e4 x its H).  That rounding, u (m + |H_ii|) <= 2 u max(m, |H_ii|), is taken off the diagonal's error before it is measured.
                ref = smp.expected(cs, "H", coef, proj)[0]
                err = H2 - ref
                slack = np.diag(2 * smp.U * np.maximum(D, np.abs(np.diag(ref))))
                H2m = ref + np.sign(err) * np.maximum(np.abs(err) - slack, 0.0)
                for k in hn:  # identity rows: exactly 1 on the diagonal, nothing else
                    assert np.all(B2[t][3 * k:3 * k + 3, 3 * k:3 * k + 3] == np.eye(3))
                for g, H, nm in ((g1, B1[t], "tet-parallel"), (g2, H2m, "patch")):
                    gt = g[12 * t:12 * t + 12]
                    where = f"{nm} tet {t} projectDBC {proj} coef {coef:g}"
                    m.check(cs, "g", gt, coef, proj, where, newton=nm == "patch")  # (the Newton gradient is also cleared where rows are dropped)
                    m.check(cs, "H", H, coef, proj, where)
                    check_dropped(cs, proj, gt, H)
                    if cs["YM"] == 0.0:
                        assert np.all(gt == 0.0) and np.all(H == 0.0)
                assert np.all(np.abs(B1[t] - H2) <= 2 * smp.tol(cs, "H", coef, proj) + 4 * smp.U * np.diag(D)), cs["name"]  # (+ the rounding of H + mass)


def test_energy(gpu_lib, elems):
    p = Carrier(gpu_lib, elems)
    m = Misses()
    pe = p.c.elastic_energy_per_elem()
    for t, cs in enumerate(elems):
        m.check(cs, "E", pe[t])
    Eref = np.array([cs["ref_E"] for cs in elems])
    xt = p.X + 1e-3 * np.random.default_rng(5).normal(size=p.X.shape)
    mass = p.c.features()["mass"]
    inertia = float(sum(mpf(float(mass[v])) * sum((mpf(float(p.X[v, i])) - mpf(float(xt[v, i]))) ** 2 for i in range(3)) for v in range(len(mass))) / 2)
    for coef in (1.0, 0.025 ** 2):
        bound = sum(smp.tol(cs, "E", coef) for cs in elems)
        E = p.c.elastic_energy(coef)
        print(f"coef {coef:g}: |E - sum E_mp| = {abs(E - coef * Eref.sum()):.3g}, bound {bound:.3g}")
        assert abs(E - coef * Eref.sum()) <= bound
        p.c.set_xtilde(p.X)
        assert abs(p.c.incremental_potential(coef) - coef * Eref.sum()) <= bound  # without inertia
        p.c.set_xtilde(xt)
        assert abs(p.c.incremental_potential(coef) - (coef * Eref.sum() + inertia)) <= bound + smp.M * smp.U * len(mass) * inertia
    p.c.close()
    m.done()


def test_gradient_and_hessian_of_every_case(gpu_lib, elems):
    p = Carrier(gpu_lib, elems)
    m = Misses()
    both_kernels(p, m, coefs=(1.0, 0.025 ** 2))
    p.c.close()
    m.done()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(gpu_lib, elems, n):
    """the cases drawn cyclically; the last tet of the layout (and lane 63 of every full wave) enters the Jacobi path of make_pd3 -- an indefinite A -- while its
    neighbours take the fast exit: a divergent wave.  Every tet is checked."""
    pool = [c for c in elems if c["ref_negA"] == 0 and c["YM"] > 0]
    jac = [c for c in elems if c["ref_negA"] > 0]
    assert len(jac) >= 2
    lay = [pool[t % len(pool)] for t in range(n)]
    for t in list(range(63, n, 64)) + [n - 1]:
        lay[t] = jac[(t // 64) % len(jac)]
    p = Carrier(gpu_lib, lay)
    m = Misses()
    both_kernels(p, m, coefs=(0.5,))
    p.c.close()
    m.done()


@pytest.mark.parametrize("n", [2, 17, 64])
def test_fan_of_tets_on_one_node(gpu_lib, elems, n):
    """n tets share their node 0: the reference of the shared node is the sum of the elements' mp contributions, its tolerance the sum of theirs; both kernels"""
    pool = [c for c in elems if np.all(c["Xr"] == smp.UNIT) and c["YM"] > 0 and not c["dtype"].any() and smp.tol(c, "H").max() <= 1e-9 * c["ref_Hscale"]]
    assert len(pool) >= 17  # the sum of the tolerances stays a tight bound
    lay = [pool[t % len(pool)] for t in range(n)]
    p = Carrier(gpu_lib, lay, shared_apex=True)
    c = p.c
    c.set_xtilde(p.X)
    G = np.array([cs["ref_g"] for cs in lay])
    H = np.array([cs["ref_H"] for cs in lay])
    gtol = sum(smp.tol(cs, "g")[:3] for cs in lay)
    Htol = sum(smp.tol(cs, "H")[:3, :3] for cs in lay)
    mass = c.features()["mass"]
    m = Misses()
    g1 = c.elastic_gradient(1.0, True)
    c.set_zero()
    c.elastic_hessian_add(1.0, True)
    A1 = upper(c)
    g2 = c.assemble_newton(1.0, True, with_gradient=True)
    A2, a2 = upper(c), c.get_a()
    g3 = c.assemble_newton(1.0, True, with_gradient=True)
    assert np.array_equal(g2, g3) and np.array_equal(a2, c.get_a())
    A2[:3, :3] -= mass[0] * np.eye(3)
    for g, A, nm in ((g1, A1, "tet-parallel"), (g2, A2, "patch")):
        assert np.all(np.abs(g[:3] - G[:, :3].sum(axis=0)) <= gtol)
        assert np.all(np.triu(np.abs(A[:3, :3] - H[:, :3, :3].sum(axis=0)) <= Htol + 4 * smp.U * mass[0] * np.eye(3)) == np.triu(np.ones((3, 3), dtype=bool)))
        for t, cs in enumerate(lay):  # the nine entries of the tet's own nodes and the blocks that couple them to the apex belong to this element alone
            own = np.arange(3 + 9 * t, 12 + 9 * t)
            got_g = np.concatenate([cs["ref_g"][:3], g[own]])
            got_H = cs["ref_H"].copy()
            got_H[:3, 3:] = A[:3, own]
            got_H[3:, :3] = A[:3, own].T
            blk = np.triu(A[np.ix_(own, own)])
            if nm == "patch":
                blk = blk - np.diag(np.repeat(mass[1 + 3 * t:4 + 3 * t], 3))
            got_H[3:, 3:] = blk + np.triu(blk, 1).T
            m.check(cs, "g", got_g, where=f"{nm} tet {t}")
            m.check(cs, "H", got_H, where=f"{nm} tet {t}")
    c.close()
    m.done()


def test_block_of_tets(gpu_lib):
    """the 2 x 2 x 2 block of cells of elastic_mp_cases.npz, 48 tets on 27 nodes, under SNH: the reference is the sum of the per-element mp contributions, the
    tolerance the sum of theirs, for both kernels and for the energies; two patch assemblies of one state give the same bits"""
    Z = np.load(emp.GOLDEN)
    V, F, X = Z["m_V"], Z["m_F"], Z["m_X"]
    cases = smp.load(prefix="b_")
    assert len(cases) == len(F) == 48 and all(np.array_equal(cs["X"], X[f]) for cs, f in zip(cases, F))
    n = 3 * len(V)
    G, Gt, H, Ht = np.zeros(n), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    for cs, f in zip(cases, F):
        idx = np.array([3 * v + i for v in f for i in range(3)])
        G[idx] += cs["ref_g"]
        Gt[idx] += smp.tol(cs, "g")
        H[np.ix_(idx, idx)] += cs["ref_H"]
        Ht[np.ix_(idx, idx)] += smp.tol(cs, "H")
    assert Ht.max() <= 1e-8 * np.abs(H).max()
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_positions(X)
    c.set_xtilde(X)
    Eref, Et = sum(cs["ref_E"] for cs in cases), sum(smp.tol(cs, "E") for cs in cases)
    assert abs(c.elastic_energy(1.0) - Eref) <= Et and abs(c.incremental_potential(1.0) - Eref) <= Et
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
        assert np.all(eg <= 1.0) and np.all(np.abs(A - H)[up] <= (Ht + (4 * smp.U * np.diag(mass) if nm == "patch" else 0.0))[up])
        assert np.all(A[up & (Ht == 0)] == 0.0)  # pairs of nodes that share no tet
    c.close()


def test_no_inversion_safeguard(gpu_lib, elems):
    """filter_step_size returns tmax unchanged for a direction that inverts an element, and the same context switched to NH shortens it; check_inversion is a
    query of the mesh and still reports an inverted tet; energy type 3 is an argument error"""
    n = 65
    V = np.tile(smp.UNIT, (n, 1))
    c = gpu_lib.Context(0)
    c.set_mesh(V, np.arange(4 * n, dtype=np.int32).reshape(n, 4), YM=1e5, PR=0.4, density=smp.DENSITY)
    c.set_energy_type("SNH")
    c.opt_init(0.01, False)
    c.set_positions(V)
    P = np.zeros((4 * n, 3))
    P[4 * 64 + 3] = (0.0, 0.0, -2.0)  # node 3 of the last tet through the plane of the other three at t = 1/2 (the filter's root: 0.8 of the way, t = 0.4)
    assert c.filter_step_size(P.reshape(-1), 1.0) == 1.0
    c.set_energy_type("NH")
    t = c.filter_step_size(P.reshape(-1), 1.0)
    assert abs(t - 0.4) <= 1e-12
    c.set_energy_type("SNH")
    assert c.check_inversion()
    X = V.copy()
    X[4 * 64 + 3] = (0.0, 0.0, -1.0)
    c.set_positions(X)
    assert not c.check_inversion()
    assert c._L.ipcgpu_set_energy_type(c.h, 3) == -1  # IPCGPU_ERR_ARG
    assert c._L.ipcgpu_set_energy_type(c.h, 2) == 0
    c.close()
    by = {cs["name"]: cs for cs in elems}
    p = Carrier(gpu_lib, [by["SNH general 0"]] * 64 + [by["SNH reflection of rest, rotated"]])
    assert not p.c.check_inversion()
    p.c.close()
