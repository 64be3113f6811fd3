"""Hand-placed contact and friction stencils through the C ABI, each compared AT ITS OWN SCALE with the mpmath reference of stencil_mp.py (stored in
tests/golden/stencil_mp_cases.npz): a stencil whose contribution is a millionth of its neighbour's is checked as tightly as the neighbour.  Every stencil
lives on one tet of a mesh of isolated tets, so every gradient entry and every entry of a tet's 12 x 12 block belongs to exactly one stencil.
Tolerance per quantity: M (sens + u scale), stencil_mp.tol -- derived there, pinned on the CPU by test_stencil_mp.py."""
import ctypes as C

import numpy as np
import pytest

import stencil_mp as smp

pytestmark = pytest.mark.gpu

BINS = (0, 1, 2, 3, 4, 5, 7)


@pytest.fixture(scope="module")
def contact():
    return smp.load(prefix="c_")


@pytest.fixture(scope="module")
def friction():
    return smp.load(prefix="f_")


@pytest.fixture(scope="module")
def shared():
    return smp.load(prefix="h_")


class Placed:
    """a context on the carrier mesh with `lay[t]` (a case or None) on tet t, the constraint sets in tet order"""

    def __init__(self, gpu_lib, lay, with_sets=True):
        self.lay, self.n = lay, len(lay)
        V, F, SF = smp.carrier_mesh(self.n)
        self.X = V.copy()
        for t, cs in enumerate(lay):
            if cs is not None:
                self.X[4 * t:4 * t + 4] = cs["X"]
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
        self.dbc = np.array(sorted(4 * t + int(k) for t, cs in enumerate(lay) if cs is not None for k in cs["dbc"] if k >= 0), dtype=np.int32)
        if len(self.dbc):
            c.set_dbc(self.dbc, 1)
        c.opt_init(0.01, False)
        c.set_surface(SF)
        c.set_pattern()
        c.set_positions(self.X)
        edges = smp.edge_lookup(c.get_surface()[1])
        self.act, self.act_tet, para, eiej = [], [], [], []
        for t, cs in enumerate(lay):
            if cs is None:
                continue
            tup, ee = smp.tuples_of(cs, t, edges)
            if cs["para"]:
                para.append(tup)
                eiej.append(ee)
            else:
                self.act.append(tup)
                self.act_tet.append(t)
        self.act = np.array(self.act, dtype=np.int32).reshape(-1, 4)
        if with_sets:
            c.contact_set(self.act, np.array(para, dtype=np.int32).reshape(-1, 4), np.array(eiej, dtype=np.int32).reshape(-1, 2))

    def blocks(self):
        ia, ja = self.c.get_pattern()
        assert np.all(np.repeat(np.arange(len(ia) - 1), np.diff(ia)) // 12 == ja // 12)  # isolated tets: no entry couples two of them
        B = smp.tet_blocks(ia, ja, self.c.get_a(), self.n)
        return B + np.triu(B, 1).transpose(0, 2, 1)  # the stored upper triangle mirrored: compared with the symmetric reference entry by entry


class Misses:
    def __init__(self):
        self.bad, self.worst = [], 0.0

    def check(self, case, k, got, where=""):
        assert np.all(np.isfinite(got)), (case["name"], k, where)
        r = smp.ratio(case, k, got)
        self.worst = max(self.worst, r)
        if not r <= smp.M:
            self.bad.append(f"{case['name']} [{case['index']}] {k} {where}: err / (sens + u scale) = {r:.3g}")

    def done(self):
        print(f"worst err / (sens + u scale) = {self.worst:.3g} (M = {smp.M:g})")
        assert not self.bad, "\n".join(self.bad)


def check_dropped(case, g, H):
    for k in case["dbc"]:
        if k >= 0:
            assert np.all(g[3 * k:3 * k + 3] == 0.0) and np.all(H[3 * k:3 * k + 3, :] == 0.0) and np.all(H[:, 3 * k:3 * k + 3] == 0.0), case["name"]


def test_distances_and_constraint_jacobian(gpu_lib, contact):
    """k_evaluate_tuples and k_jt_tuples on every active case"""
    act = [cs for cs in contact if not cs["para"]]
    p = Placed(gpu_lib, act, with_sets=False)
    L, c = p.c._L, p.c
    L.ipcgpu_contact_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ipcgpu_contact_jt_multiply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    val, inp, out = np.zeros(len(act)), np.random.default_rng(3).uniform(0.5, 2.0, len(act)) * np.where(np.arange(len(act)) % 2, -1.0, 1.0), np.zeros(12 * p.n)
    c._chk(L.ipcgpu_contact_evaluate(c.h, len(act), p.act.ctypes.data, val.ctypes.data))
    c._chk(L.ipcgpu_contact_jt_multiply(c.h, len(act), p.act.ctypes.data, inp.ctypes.data, 0.75, out.ctypes.data))
    m = Misses()
    for t, cs in enumerate(act):
        m.check(cs, "d", val[t])
        m.check(cs, "gd", out[12 * t:12 * t + 12] / (0.75 * cs["mult"] * inp[t]), "J^T")  # (the scaling adds two roundings: inside M)
    c.close()
    m.done()


@pytest.mark.parametrize("kappa", smp.KAPPAS)
def test_energy_and_gradient(gpu_lib, contact, kappa):
    lay = [cs for cs in contact if cs["kappa"] == kappa] + [None, None]
    p = Placed(gpu_lib, lay)
    cs_ = lay[:-2]
    E = p.c.contact_energy(smp.DHAT, kappa)
    Eref = np.array([cs["ref_E"] for cs in cs_])
    bound = smp.M * (sum(cs["sens_E"] for cs in cs_) + smp.U * np.abs(Eref).sum())
    print(f"energy: |E - sum E_mp| = {abs(E - Eref.sum()):.3g}, bound {bound:.3g}")
    assert abs(E - Eref.sum()) <= bound
    m = Misses()
    for proj in (True, False):
        g = p.c.contact_gradient_add(smp.DHAT, kappa, proj)
        assert len(p.dbc) and np.all(g.reshape(-1, 3)[p.dbc] == 0.0)
        assert np.all(g[12 * len(cs_):] == 0.0)
        for t, cs in enumerate(cs_):
            m.check(cs, "g", g[12 * t:12 * t + 12], f"projectDBC {proj}")
    p.c.close()
    m.done()


def hessian_layout(gpu_lib, lay, kappa):
    p = Placed(gpu_lib, lay)
    m = Misses()
    for proj in (True, False):
        p.c.set_zero()
        p.c.contact_hessian_add(smp.DHAT, kappa, proj)
        B = p.blocks()
        for t, cs in enumerate(lay):
            if cs is None:
                assert np.all(B[t] == 0.0)
                continue
            m.check(cs, "H", B[t], f"tet {t} projectDBC {proj}")
            check_dropped(cs, np.zeros(12), B[t])
    p.c.close()
    m.done()


@pytest.mark.parametrize("kappa", smp.KAPPAS)
def test_hessian_every_case_once(gpu_lib, contact, kappa):
    """layout A: every bin is one partial wave"""
    lay = [cs for cs in contact if cs["kappa"] == kappa]
    assert all(any(smp.bin_of(cs) == b for cs in lay) for b in BINS) and not any(smp.bin_of(cs) == 6 for cs in contact)
    hessian_layout(gpu_lib, lay[:7] + [None] + lay[7:] + [None], kappa)


COUNTS = (1, 63, 64, 65, 130)


def tiled(contact, kappa, counts, seed):
    lay = []
    for b, k in counts.items():
        pool = [cs for cs in contact if smp.bin_of(cs) == b and cs["kappa"] == kappa]
        lay += [pool[j % len(pool)] for j in range(k)]  # copies of a case have bit-identical coordinates
    lay += [None] * 3
    return [lay[i] for i in np.random.default_rng(seed).permutation(len(lay))]


@pytest.mark.parametrize("shift", range(5))
def test_hessian_full_and_partial_waves(gpu_lib, contact, shift):
    """layout B: the bins hold 1, 63, 64, 65 and 130 entries (which bin holds which count rotates with `shift`), in shuffled order, so that well- and
    ill-conditioned stencils sit side by side in every wave; every copy of a case meets the same reference under the same tolerance"""
    kappa = smp.KAPPAS[shift % 2]
    hessian_layout(gpu_lib, tiled(contact, kappa, {b: COUNTS[(i + shift) % 5] for i, b in enumerate(BINS)}, 40 + shift), kappa)


@pytest.mark.parametrize("which", ["only_mollified", "only_active"])
def test_hessian_with_one_list_empty(gpu_lib, contact, which):
    bins = BINS[4:] if which == "only_mollified" else BINS[:4]
    hessian_layout(gpu_lib, tiled(contact, smp.KAPPAS[1], {b: COUNTS[(i + 2) % 5] for i, b in enumerate(bins)}, 50), smp.KAPPAS[1])


@pytest.mark.parametrize("n", [300, 257, 64])
def test_many_stencils_on_one_node(gpu_lib, shared, n):
    """node 0 against the faces of n other tets: more contributions to one node than a workgroup has threads (300, 257), exactly one wave (64)"""
    cs_ = shared[:n]
    kappa = float(cs_[0]["kappa"])
    V, F, SF = smp.carrier_mesh(n + 1)
    X = V.copy()
    X[0] = cs_[0]["X"][0]
    act = []
    for t, cs in enumerate(cs_):
        assert np.all(cs["X"][0] == X[0])
        X[4 * (t + 1) + 1:4 * (t + 1) + 4] = cs["X"][1:]
        act.append((-1, 4 * (t + 1) + 1, 4 * (t + 1) + 2, 4 * (t + 1) + 3))
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(0.01, False)
    c.set_surface(SF)
    c.set_positions(X)
    c.contact_set(np.array(act, dtype=np.int32))
    pairs = c.contact_connectivity()
    want = {(0, a[k]) for a in act for k in (1, 2, 3)}  # the pairs inside a triangle's tet are the mesh's own
    assert len(pairs) == len(want) == 3 * n and {(int(a), int(b)) for a, b in pairs} == want
    c.set_pattern(pairs)
    E = c.contact_energy(smp.DHAT, kappa)
    Eref = np.array([cs["ref_E"] for cs in cs_])
    assert abs(E - Eref.sum()) <= smp.M * (sum(cs["sens_E"] for cs in cs_) + smp.U * np.abs(Eref).sum())
    g = c.contact_gradient_add(smp.DHAT, kappa, True)
    G = np.array([cs["ref_g"] for cs in cs_])
    bound = smp.M * (sum(cs["sens_g"][:3] for cs in cs_) + smp.U * np.abs(G[:, :3]).sum(axis=0))
    print(f"n = {n}: node 0 gradient error / bound {np.abs(g[:3] - G[:, :3].sum(axis=0)) / bound}")
    assert np.all(np.abs(g[:3] - G[:, :3].sum(axis=0)) <= bound)
    m = Misses()
    for t, cs in enumerate(cs_):
        got = np.concatenate([cs["ref_g"][:3], g[12 * (t + 1) + 3:12 * (t + 1) + 12]])  # the triangle's nine entries belong to this stencil alone
        m.check(cs, "g", got, "triangle nodes")
    c.set_zero()
    c.contact_hessian_add(smp.DHAT, kappa, True)
    ia, ja = c.get_pattern()
    a = c.get_a()
    rows = np.zeros((3, 3 * V.shape[0]))
    for r in range(3):
        rows[r, ja[ia[r]:ia[r + 1]]] = a[ia[r]:ia[r + 1]]
    H = np.array([cs["ref_H"] for cs in cs_])
    bound = smp.M * (sum(cs["sens_H"][:3, :3] for cs in cs_) + smp.U * np.abs(H[:, :3, :3]).sum(axis=0))
    err = np.abs(rows[:, :3] - H[:, :3, :3].sum(axis=0))
    assert np.all(np.triu(err <= bound) == np.triu(np.ones((3, 3), dtype=bool))), (err, bound)
    for t, cs in enumerate(cs_):
        got = cs["ref_H"].copy()
        got[:3, 3:] = rows[:, 12 * (t + 1) + 3:12 * (t + 1) + 12]  # the blocks (0, v) of this stencil's three triangle nodes
        got[3:, :3] = got[:3, 3:].T
        m.check(cs, "H", got, "blocks (0, v)")
    c.close()
    m.done()


def test_lagged_friction(gpu_lib, friction):
    m = Misses()
    for kappa, eps2 in sorted({(float(cs["kappa"]), float(cs["eps2"])) for cs in friction}):
        lay = [cs for cs in friction if cs["kappa"] == kappa and cs["eps2"] == eps2] + [None]
        p = Placed(gpu_lib, lay)
        cs_, c = lay[:-1], p.c
        lag = c.friction_update(smp.DHAT, kappa)
        assert len(lag["lam"]) == len(cs_)
        for t, cs in enumerate(cs_):
            m.check(cs, "lam", lag["lam"][t])
            m.check(cs, "coord", lag["coord"][t])
            m.check(cs, "basis", lag["basis"][t])  # signed: the construction fixes the direction of both tangents
        Xn = p.X.copy()
        for t, cs in enumerate(cs_):
            Xn[4 * t:4 * t + 4] = cs["Xn"]
        c.set_positions(Xn)
        coef = float(cs_[0]["coef"])
        E = c.friction_energy(p.X, eps2, coef)
        Eref = np.array([cs["ref_E"] for cs in cs_])
        assert abs(E - Eref.sum()) <= smp.M * (sum(cs["sens_E"] for cs in cs_) + smp.U * np.abs(Eref).sum()), (kappa, eps2, E, Eref.sum())
        g = c.friction_gradient_add(p.X, eps2, coef)
        c.set_zero()
        c.friction_hessian_add(p.X, eps2, coef, True)
        B = p.blocks()
        assert np.all(g[12 * len(cs_):] == 0.0) and np.all(B[len(cs_)] == 0.0)
        for t, cs in enumerate(cs_):
            m.check(cs, "g", g[12 * t:12 * t + 12])
            m.check(cs, "H", B[t])
            if np.all(cs["Xn"] == cs["X"]):  # |u| = 0: no force, the block coef lam (2 / eps) T^T T is finite
                assert np.all(g[12 * t:12 * t + 12] == 0.0) and np.abs(B[t]).max() > 0
        c.close()
    m.done()
