"""Contact groups (`ipcgpu_set_contact_groups`) through the C ABI: masked pairs of bodies are absent from the constraint sets, the CCD sweeps and the
intersection check, friction multipliers carry the factor of their pair of groups, and a body masked against a static one falls through it in free
fall.  The oracle cannot filter: expected values are its unfiltered results, filtered on the host here.

The scene: three `make_box(3, 1, 3)` slabs A, B, C stacked with the gap of `two_blocks(0.004)` (tests/test_gpu_friction.py), vertically aligned so that
vertices face vertices and edges face parallel edges -- that is what puts PP, PE and mollified tuples beside the PT and EE ones into both A-B and B-C --,
jittered, dHat = 1e-6 * bboxDiag2 * 160: A-B and B-C are active, A-C (0.3 apart) is not."""
import numpy as np
import pytest

from ipc_amd import scene

pytestmark = pytest.mark.gpu

GAP, THICK, SEED = 0.004, 0.3, 0  # seed: picked on the CPU so that every kind of tuple occurs in A-B and in B-C (asserted in `stack`)
KEYS = ("active", "para", "para_eiej", "cs_ptee")
ALL_ON = ([0, 1, 2], np.ones((3, 3), dtype=np.uint8))


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def collide_without(*pairs, n=3):
    c = np.ones((n, n), dtype=np.uint8)
    for g, h in pairs:
        c[g, h] = c[h, g] = 0
    return c


def slabs(origins, size=(1.0, THICK, 1.0)):
    Vs, Fs, off = [], [], 0
    for o in origins:
        V, F = scene.make_box(3, 1, 3, size=size, origin=o)
        Vs.append(V)
        Fs.append(F + off)
        off += V.shape[0]
    return np.vstack(Vs), np.vstack(Fs).astype(np.int32), Vs[0].shape[0], Fs[0].shape[0]


def kind_of(a):
    return "EE" if a[0] >= 0 else "PP" if a[2] < 0 else "PE" if a[3] < 0 else "PT"


class Stack:
    pass


@pytest.fixture(scope="module")
def stack(orc):
    S = Stack()
    V, S.F, S.nB, S.tB = slabs([(0, k * (THICK + GAP), 0) for k in range(3)])
    S.V = scene.jitter(V, S.F, rel=3e-3, seed=SEED)
    S.SF = scene.surface_tris(S.F)
    S.m = orc.Mesh(S.V, S.F, YM=1e5, PR=0.4, density=1000.0)
    S.m.set_surface(S.SF)
    S.dHat = 1e-3 ** 2 * S.m.features()["bboxDiag2"] * 160
    S.cs = orc.Contacts()
    S.sets = S.cs.build(S.m, S.dHat)
    S.svi, S.sfe = orc.mesh_surface(S.m)
    S.sfe = np.asarray(S.sfe).reshape(-1, 2)
    # the condition of the test: every kind of tuple in both pairs of neighbours, nothing between A and C, nothing inside a body
    pairs = S_pairs(S, S.sets)
    kinds = np.array([kind_of(a) for a in S.sets["active"]])
    for ab in ((0, 1), (1, 2)):
        sel = np.all(pairs["active"] == ab, axis=1)
        for k in ("PP", "PE", "PT", "EE"):
            assert np.count_nonzero(kinds[sel] == k) >= 1, (ab, k)
        assert np.count_nonzero(np.all(pairs["para"] == ab, axis=1)) >= 1, ab
        assert np.count_nonzero(np.all(pairs["cs_ptee"] == ab, axis=1)) >= 1, ab
    for k in KEYS:
        assert set(map(tuple, pairs[k])) == {(0, 1), (1, 2)}, k
    return S


def S_pairs(S, sets):
    """per list the (lower, higher) components of every entry: a primitive's component is that of its first node"""
    comp = lambda v: np.asarray(v) // S.nB
    a = sets["active"]
    first = np.where(a[:, 0] < 0, -a[:, 0] - 1, a[:, 0])
    other = np.where(a[:, 0] < 0, a[:, 1], a[:, 2])
    q = sets["para_eiej"]
    cs = sets["cs_ptee"]
    pt = cs[:, 0] < 0
    c0 = np.where(pt, S.svi[np.where(pt, -cs[:, 0] - 1, 0)], S.sfe[np.where(pt, 0, cs[:, 0]), 0])
    c1 = np.where(pt, S.SF[np.where(pt, cs[:, 1], 0), 0], S.sfe[np.where(pt, 0, cs[:, 1]), 0])
    # a mollified tuple of PP / PE form carries its two edges in paraEEeIeJ; one of EE form carries (-1, -1) there and its four nodes itself
    pa = sets["para"]
    byEdge = q[:, 0] >= 0
    q0 = np.where(byEdge, S.sfe[np.where(byEdge, q[:, 0], 0), 0], pa[:, 0])
    q1 = np.where(byEdge, S.sfe[np.where(byEdge, q[:, 1], 0), 0], pa[:, 2])
    assert np.all(q0 >= 0) and np.all(q1 >= 0)
    out = {}
    for k, (x, y) in (("active", (first, other)), ("para_eiej", (q0, q1)), ("cs_ptee", (c0, c1))):
        cx, cy = comp(x), comp(y)
        out[k] = np.stack([np.minimum(cx, cy), np.maximum(cx, cy)], axis=1).reshape(-1, 2)
    out["para"] = out["para_eiej"]
    return out


def filtered(S, sets, masked):
    """the sets with the entries of the masked pairs of components deleted, order kept"""
    pairs = S_pairs(S, sets)
    keep = {k: np.array([tuple(p) not in masked for p in pairs[k]], dtype=bool).reshape(-1) for k in KEYS}
    return {k: sets[k][keep[k]] for k in KEYS}


def context(gpu_lib, S, groups=None, fric_scale=None):
    c = gpu_lib.Context(0)
    c.set_mesh(S.V, S.F, YM=1e5, PR=0.4, density=1000.0)
    c.set_components([S.nB, 2 * S.nB, 3 * S.nB], [S.tB, 2 * S.tB, 3 * S.tB])
    if groups is not None:
        c.set_contact_groups(groups[0], groups[1], fric_scale)
    c.opt_init(0.025, False)
    c.set_surface(S.SF)
    return c


MASKS = {
    "all on": (ALL_ON, set()),
    "A-B off": (([0, 1, 2], collide_without((0, 1))), {(0, 1)}),
    "B-C off": (([0, 1, 2], collide_without((1, 2))), {(1, 2)}),
    "one group that does not collide with itself": (([0, 0, 0], np.zeros((1, 1), dtype=np.uint8)), {(0, 1), (1, 2), (0, 2), (0, 0), (1, 1), (2, 2)}),
}


@pytest.mark.parametrize("mask", list(MASKS))
def test_sets_are_the_oracles_with_the_masked_pairs_deleted(gpu_lib, stack, mask):
    S = stack
    groups, masked = MASKS[mask]
    c = context(gpu_lib, S, groups)
    got = c.contact_build(S.dHat)
    want = filtered(S, S.sets, masked)
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (mask, k)  # the same tuples in the same order
    if mask == "all on":
        plain = context(gpu_lib, S)
        ref = plain.contact_build(S.dHat)
        assert all(np.array_equal(got[k], ref[k]) and np.array_equal(ref[k], S.sets[k]) for k in KEYS)
        assert plain.get_contact_groups()[0] == 1 and np.all(plain.get_contact_groups()[1] == 0xFFFF0000)
        plain.close()
    elif masked == {(0, 1)} or masked == {(1, 2)}:
        assert all(0 < len(got[k]) < len(S.sets[k]) for k in KEYS)
        n, w = c.get_contact_groups()
        assert n == 3 and np.array_equal((w >> 4) & 15, np.repeat([0, 1, 2], S.nB))
    else:
        assert all(len(got[k]) == 0 for k in KEYS)
    # what consumes the sets takes the filtered ones: the connectivity of the pattern look-ahead, the contact report's rows
    held = c.contact_held()
    assert np.array_equal(held["active"], want["active"])
    conn = c.contact_connectivity()
    comp = conn // S.nB
    assert all((min(p), max(p)) not in masked for p in comp.tolist())
    rep = c.contact_report(S.dHat, 1e3)
    assert {(int(r["a"]), int(r["b"])) for r in rep} == {(0, 1), (1, 2)} - masked
    c.close()


def test_ccd_does_not_sweep_masked_pairs(orc, gpu_lib, stack):
    S = stack
    c = context(gpu_lib, S, MASKS["A-B off"][0])
    c.contact_build(S.dHat)
    cand = S.sets["cs_ptee"]
    A, C_ = slice(0, S.nB), slice(2 * S.nB, 3 * S.nB)
    # only A moves, into B by more than the gap
    p = np.zeros_like(S.V)
    p[A, 1] = 0.02
    fo, _, _ = orc.ccd_full(S.m, p.reshape(-1), 0.8, 1.0)
    assert fo < 1.0
    assert c.ccd_partial(p.reshape(-1), 0.8, 1.0) == (1.0, (0, 0))
    assert c.ccd_full(p.reshape(-1), 0.8, 1.0)[:2] == (1.0, (0, 0))
    s, cap, arg, _ = c.ccd_full_reference(p.reshape(-1), 0.8, 1.0)
    assert s == cap and arg == (-1, -1, -1)
    # C moves into B as well: the bound of B-C alone, which is the oracle's for the direction with A's part reversed (A-B separates there, and the
    # mean |p| behind the reference sweep's cap is the same)
    rng = np.random.default_rng(21)
    p = 0.002 * rng.normal(size=S.V.shape)
    p[A, 1] += 0.02
    p[C_, 1] -= 0.02
    prev = p.copy()
    prev[A] = -p[A]
    so, arg_o = orc.ccd_partial(S.cs, S.m, prev.reshape(-1), 0.8, 1.0)
    fo, pfo, _ = orc.ccd_full(S.m, prev.reshape(-1), 0.8, 1.0)
    unmasked, _, _ = orc.ccd_full(S.m, p.reshape(-1), 0.8, 1.0)
    assert fo < 1.0 and so < 1.0 and unmasked <= fo
    sg, pg = c.ccd_partial(p.reshape(-1), 0.8, 1.0)
    fg, pfg, _ = c.ccd_full(p.reshape(-1), 0.8, 1.0)
    print("ccd partial", sg, so, "full", fg, fo)
    assert abs(sg - so) <= 1e-9 * so and pg == tuple(int(x) for x in cand[arg_o])
    assert abs(fg - fo) <= 1e-9 * fo and pfg == pfo
    masked_ref = c.ccd_full_reference(p.reshape(-1), 0.8, 1.0)
    c.set_contact_groups(None, None)
    plain_ref = c.ccd_full_reference(prev.reshape(-1), 0.8, 1.0)
    print("ccd reference", masked_ref, plain_ref)
    assert masked_ref[:3] == plain_ref[:3] and masked_ref[0] < masked_ref[1] and masked_ref[3] < plain_ref[3]
    c.close()


def test_intersection_check_skips_masked_pairs(gpu_lib, stack):
    S = stack
    c = context(gpu_lib, S)
    B, C_ = slice(S.nB, 2 * S.nB), slice(2 * S.nB, 3 * S.nB)
    X = S.V.copy()
    X[B, 1] -= GAP + 0.5 * THICK  # B half a thickness into A
    c.set_positions(X)
    assert c.is_intersected()
    c.set_contact_groups(*MASKS["A-B off"][0])
    assert not c.is_intersected()
    c.set_contact_groups(*MASKS["B-C off"][0])
    assert c.is_intersected()
    c.set_contact_groups(*MASKS["A-B off"][0])
    X[C_, 1] -= 2 * GAP + THICK  # C half a thickness into B
    c.set_positions(X)
    assert c.is_intersected()
    c.set_contact_groups(*MASKS["one group that does not collide with itself"][0])
    assert not c.is_intersected()
    c.close()


def test_a_point_inside_a_tetrahedron_of_a_masked_group_is_not_an_intersection(gpu_lib, stack):
    """k_points_in_tets: two isolated nodes (`.pt` points), each a component of its own, the first in A's group, the second in C's; both sit at the
    centroid of an element of B."""
    S = stack
    centroid = S.V[S.F[S.tB + 4]].mean(axis=0)
    away = np.array([3.0, 3.0, 3.0])
    V = np.vstack([S.V, away, away + 1.0])
    c = gpu_lib.Context(0)
    c.set_mesh(V, S.F, YM=1e5, PR=0.4, density=1000.0)
    nV = V.shape[0]
    c.set_components([S.nB, 2 * S.nB, 3 * S.nB, nV - 1, nV], [S.tB, 2 * S.tB, 3 * S.tB, 3 * S.tB, 3 * S.tB])
    c.set_surface(S.SF)
    groups = [0, 1, 2, 0, 2]
    assert not c.is_intersected()
    X = V.copy()
    X[nV - 2] = centroid
    c.set_positions(X)
    assert c.is_intersected()
    c.set_contact_groups(groups, collide_without((0, 1)))
    assert not c.is_intersected()  # the point of A's group inside B
    c.set_contact_groups(groups, collide_without((1, 2)))
    assert c.is_intersected()
    c.set_contact_groups(groups, collide_without((0, 1)))
    X[nV - 1] = centroid + 1e-3
    c.set_positions(X)
    assert c.is_intersected()  # the point of C's group inside B
    c.set_contact_groups(groups, collide_without((0, 1), (1, 2)))
    assert not c.is_intersected()
    c.close()


def test_friction_multipliers_carry_the_scale_of_their_pair_of_groups(orc, gpu_lib, stack):
    S = stack
    V, m = S.V, S.m
    scale = np.array([[1.0, 0.25, 0.0], [0.25, 1.0, 1.0], [0.0, 1.0, 1.0]])
    c = context(gpu_lib, S, ALL_ON, scale)
    act = S.sets["active"]
    pairs = S_pairs(S, S.sets)["active"]
    ab, bc = np.all(pairs == (0, 1), axis=1), np.all(pairs == (1, 2), axis=1)
    assert np.all(ab | bc) and {kind_of(a) for a in act[ab]} == {kind_of(a) for a in act[bc]} == {"PP", "PE", "PT", "EE"}
    factor = np.where(ab, 0.25, 1.0)
    try:
        c.contact_set(act)
        fr = orc.Friction()
        lo = fr.update(m, act, 1.0, 2.0e3)
        lg = c.friction_update(1.0, 2.0e3)
        assert len(lg["lam"]) == len(act)  # n_lagged does not depend on the scales
        print("lambda", relerr(lg["lam"], lo["lam"] * factor))
        assert relerr(lg["lam"], lo["lam"] * factor) < 1e-12
        assert np.abs(lg["coord"] - lo["coord"]).max() < 1e-12 and np.abs(lg["basis"] - lo["basis"]).max() < 1e-12
        frAB, frBC = orc.Friction(), orc.Friction()
        frAB.update(m, act[ab], 1.0, 2.0e3)
        frBC.update(m, act[bc], 1.0, 2.0e3)
        rng = np.random.default_rng(5)
        U = 2e-4 * rng.normal(size=V.shape)
        U[::3] *= 30.0  # sliding on both sides of eps
        eps2, mu = (1.5e-3) ** 2, 0.37
        Vn = V + U
        m.set_V(Vn)
        c.set_positions(Vn)
        Eo = frAB.energy(m, V, eps2, 0.25 * mu) + frBC.energy(m, V, eps2, mu)
        Eg = c.friction_energy(V, eps2, mu)
        go = frAB.gradient(m, V, eps2, 0.25 * mu) + frBC.gradient(m, V, eps2, mu)
        gg = c.friction_gradient_add(V, eps2, mu)
        print("energy", abs(Eg - Eo) / abs(Eo), "gradient", relerr(gg, go))
        assert abs(Eg - Eo) <= 1e-11 * abs(Eo)
        assert relerr(gg, go) < 1e-10
        extra = np.array(S.cs.connectivity(m).tolist(), dtype=np.int32)
        c.set_pattern(extra)
        ia, ja = m.pattern(extra_edges=extra)
        for proj in (False, True):
            if proj:
                dbc = np.unique(np.abs(act[:6, 1]))
                m.set_dbc(dbc, 1)
                c.set_dbc(dbc, 1)
            c.set_zero()
            c.friction_hessian_add(V, eps2, mu, proj)
            a_o = frAB.hessian(m, V, len(ja), eps2, 0.25 * mu, proj) + frBC.hessian(m, V, len(ja), eps2, mu, proj)
            print("hessian", proj, relerr(c.get_a(), a_o))
            assert relerr(c.get_a(), a_o) < 1e-9 and np.count_nonzero(a_o) > 0
        # a scale of 0: the stencils stay in the lagged set with a zero multiplier
        c.set_positions(V)
        m.set_V(V)
        c.set_contact_groups(ALL_ON[0], ALL_ON[1], np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]]))
        lz = c.friction_update(1.0, 2.0e3)
        assert len(lz["lam"]) == len(act) and np.all(lz["lam"][ab] == 0.0) and relerr(lz["lam"][bc], lo["lam"][bc]) < 1e-12
    finally:
        m.clear_dbc()
        m.set_V(V)
        c.close()


def test_set_components_and_set_mesh_go_back_to_the_default(gpu_lib, stack):
    S = stack
    c = context(gpu_lib, S, MASKS["A-B off"][0])
    assert len(c.contact_build(S.dHat)["active"]) < len(S.sets["active"])
    c.set_components([S.nB, 2 * S.nB, 3 * S.nB], [S.tB, 2 * S.tB, 3 * S.tB])
    assert c.get_contact_groups()[0] == 1 and np.all(c.get_contact_groups()[1] == 0xFFFF0000)
    got = c.contact_build(S.dHat)
    assert all(np.array_equal(got[k], S.sets[k]) for k in KEYS)
    c.set_contact_groups(*MASKS["B-C off"][0])
    assert len(c.contact_build(S.dHat)["active"]) < len(S.sets["active"])
    c.set_mesh(S.V, S.F, YM=1e5, PR=0.4, density=1000.0)
    c.opt_init(0.025, False)
    c.set_surface(S.SF)
    got = c.contact_build(S.dHat)
    assert all(np.array_equal(got[k], S.sets[k]) for k in KEYS)
    c.set_contact_groups(None, None)  # the explicit way back
    assert c.get_contact_groups()[0] == 1
    c.close()


def test_errors(gpu_lib, stack):
    S = stack
    c = gpu_lib.Context(0)
    with pytest.raises(gpu_lib.IpcGpuError, match="error -3"):  # IPCGPU_ERR_STATE: no mesh
        c.set_contact_groups([0], [[1]])
    c.set_mesh(S.V, S.F)
    with pytest.raises(gpu_lib.IpcGpuError, match="one group per component"):  # the default table has one component
        c.set_contact_groups(*ALL_ON)
    c.set_contact_groups([0], [[0]])
    c.set_components([S.nB, 2 * S.nB, 3 * S.nB], [S.tB, 2 * S.tB, 3 * S.tB])
    for bad in (([0, 1], ALL_ON[1]), ([0, 1, 3], ALL_ON[1]), ([0, 1, 2], [[1, 1, 0], [1, 1, 1], [1, 1, 1]])):
        with pytest.raises(gpu_lib.IpcGpuError, match="error -1"):
            c.set_contact_groups(*bad)
    with pytest.raises(gpu_lib.IpcGpuError, match="error -1"):
        c.set_contact_groups(ALL_ON[0], ALL_ON[1], -np.ones((3, 3)))
    assert c.get_contact_groups()[0] == 1  # nothing of the rejected tables was kept
    c.set_shard(0, 2)
    with pytest.raises(gpu_lib.IpcGpuError, match="sharded"):
        c.set_contact_groups(*ALL_ON)
    c.close()


G, DT = 9.80665, 0.04


def drop_scene(gpu_lib, with_d):
    """A static slab A (wide enough for two), B at rest just above it and masked against it, optionally D beside B, unmasked"""
    VA, FA = scene.make_box(3, 1, 3, size=(2.4, THICK, 1.0), origin=(0, 0, 0))
    parts = [(VA, FA)] + [scene.make_box(3, 1, 3, size=(1.0, THICK, 1.0), origin=(x0, THICK + GAP, 0)) for x0 in ((0.05, 1.35) if with_d else (0.05,))]
    V = np.vstack([p[0] for p in parts])
    offs = np.cumsum([0] + [p[0].shape[0] for p in parts])
    F = np.vstack([p[1] + o for p, o in zip(parts, offs)]).astype(np.int32)
    V = scene.jitter(V, F, rel=3e-3)
    node_end, tet_end = offs[1:], np.cumsum([p[1].shape[0] for p in parts])
    c = gpu_lib.Context(0)
    c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
    c.set_components(node_end, tet_end)
    c.set_contact_groups(list(range(len(parts))), collide_without((0, 1), n=len(parts)))
    c.opt_init(DT, True)
    c.set_surface(scene.surface_tris(F))
    c.set_dbc(np.arange(offs[1], dtype=np.int32), 1)
    c.enable_self_collision(1e-3)
    c.precompute()
    return c, V, offs


def step_and_check_no_ab(c, offs):
    assert c.solve_timestep(200) < 200
    comp = lambda v: np.searchsorted(offs[1:], v, side="right")
    a = c.contact_held()["active"]
    first = np.where(a[:, 0] < 0, -a[:, 0] - 1, a[:, 0])
    other = np.where(a[:, 0] < 0, a[:, 1], a[:, 2])
    assert not np.any((np.minimum(comp(first), comp(other)) == 0) & (np.maximum(comp(first), comp(other)) == 1))
    rep = c.contact_report()
    rows = {(int(r["a"]), int(r["b"])): r for r in rep}
    assert (0, 1) not in rows
    return rows


def test_a_body_masked_against_a_static_one_falls_through_it_in_free_fall(gpu_lib):
    """A uniform translation lies in the null space of the elastic Hessian and nothing else acts on B: backward Euler from rest gives
    y_k = y_0 - g dt^2 k (k + 1) / 2 for every node, through A and out on the other side."""
    c, V, offs = drop_scene(gpu_lib, with_d=False)
    B = slice(offs[1], offs[2])
    worst = 0.0
    for k in range(1, 10):
        step_and_check_no_ab(c, offs)
        X = c.state()["V"]
        want = V[B].copy()
        want[:, 1] -= G * DT * DT * k * (k + 1) / 2
        worst = max(worst, np.abs(X[B] - want).max())
        assert np.array_equal(X[:offs[1]], V[:offs[1]])
    print("largest deviation from free fall", worst)
    assert X[B, 1].max() < V[:offs[1], 1].min()  # all of B below all of A
    assert worst <= 1e-9 * 1.0  # of the block size
    c.close()


def test_an_unmasked_body_beside_the_masked_one_lands(gpu_lib):
    c, V, offs = drop_scene(gpu_lib, with_d=True)
    A, B, D = slice(0, offs[1]), slice(offs[1], offs[2]), slice(offs[2], offs[3])
    seen = False
    for k in range(1, 10):
        rows = step_and_check_no_ab(c, offs)
        X = c.state()["V"]
        assert X[D, 1].min() > X[A, 1].max() - 0.01 and not c.is_intersected()  # D stays on top (A's top face is flat up to the jitter)
        if (0, 2) in rows:
            seen = True
            assert rows[(0, 2)]["minD2"] > 0.0
        assert (1, 2) not in rows
    assert seen and X[B, 1].max() < X[A, 1].min()
    c.close()
