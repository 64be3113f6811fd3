"""The fibre kernels (ipc_amd/csrc/fiber_kernels.hip) against the mpmath reference tests/fiber_mp.py: energy per element, gradient and CSR blocks of every
case as a one-tet mesh, the cases tiled over isolated tets at sizes that hit wave and workgroup edges, a shared-node block with Dirichlet nodes against the
per-element sums, and the lanes that must write nothing.  Tolerances are fiber_mp's M (sens + u scale); b and vol k of the reference come from the context's
own restTriInv and volume (the kernels' inputs)."""
import numpy as np
import pytest

import fiber_mp as fm

pytestmark = pytest.mark.gpu

CASES = fm.cases()
ENERGY = {0: "NH", 1: "FCR", 2: "SNH"}
GROUP_OF_ACT = {-0.2: 0, 0.0: 1, 0.3: 2}
ACTS = {0: -0.2, 2: 0.3}


def _ctx(gpu_lib, X, T, x, energy=0, dbc=None):
    c = gpu_lib.Context(0)
    c.set_mesh(X, T, YM=1e5, PR=0.4, density=1000.0)
    c.set_energy_type(ENERGY[energy])
    for typ in (1, 2):
        if dbc is not None and np.any(dbc == typ):
            c.set_dbc(np.flatnonzero(dbc == typ), typ)
    c.opt_init(0.01, False)
    c.set_pattern()
    c.set_positions(x)
    c.set_xtilde(x)
    return c


def _set(c, t0, t1, case):
    c.set_fibers((t0, t1), case["a"], case["k"], law=case["law"], k2=case["k2"], tension_only=case["tension_only"], group=GROUP_OF_ACT[case["act"]])


def _dense_upper(c):
    ia, ja = c.get_pattern()
    A = np.zeros((len(ia) - 1, len(ia) - 1))
    A[np.repeat(np.arange(len(ia) - 1), np.diff(ia)), ja] = c.get_a()
    return A


def _worst(got, ref, case, k, coef=1.0, proj=True):
    val, tol = fm.expected(case, ref, k, coef, proj)
    return float(np.max(fm.ratio(np.asarray(got) - val, tol / fm.M))) / fm.M  # in units of the tolerance


_EVAL = {}


def _reference(i, A9, vol):
    """the evaluated case i with the context's rest inputs; one evaluation per (case, inputs)"""
    key = (i, A9.tobytes(), float(vol))
    if key not in _EVAL:
        c = fm.with_elems(CASES[i], A9, vol)
        _EVAL[key] = (c, fm.evaluate(c))
    return _EVAL[key]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_one_tet(gpu_lib, i):
    cs = CASES[i]
    c = _ctx(gpu_lib, cs["X"], cs["T"], cs["x"], cs["energy"])
    _set(c, 0, 1, cs)
    for g, a in ACTS.items():
        c.fiber_set_activation(g, a)
    f = c.features()
    case, ref = _reference(i, f["restTriInv"][0], f["triArea"][0])
    assert c.fiber_get()["n"] == 1
    worst = {}
    for coef in (1.0, 0.37):
        E, per = c.fiber_energy(coef), c.fiber_energy_per_elem()
        g = c.fiber_gradient_add(coef, True)
        c.set_zero()
        c.fiber_hessian_add(coef, True)  # (raises where codimErr is set)
        H = _dense_upper(c)
        assert not np.isnan(E) and not np.isnan(per).any() and not np.isnan(g).any() and not np.isnan(H).any()
        assert c.fiber_energy(coef) == E  # the same state, the same bits
        if cs["overflow"]:
            assert E == np.inf and per[0] == np.inf and not g.any() and not H.any()
            continue
        worst["E"] = max(worst.get("E", 0.0), _worst(E, ref, case, "E", coef))
        worst["perW"] = max(worst.get("perW", 0.0), _worst(per, ref, case, "perW"))
        worst["g"] = max(worst.get("g", 0.0), _worst(g, ref, case, "g", coef))
        worst["H"] = max(worst.get("H", 0.0), float(np.max(fm.ratio(H - np.triu(fm.expected(case, ref, "H", coef)[0]), fm.tolerance(ref, "H", coef) / fm.M))) / fm.M)
    pe, tot = c.fiber_state()
    if not cs["overflow"]:
        assert abs(pe[0, 0] - ref["len"][0]) <= fm.M * (4 * fm.U * max(ref["len"][0], 1.0) + ref["sens_len"][0]) and tot[0] == pe[0, 0] == tot[1]
    print(f"{cs['name']}: worst error / tolerance {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst
    c.close()


@pytest.mark.parametrize("nT", [63, 64, 65, 257])
def test_tiled_over_isolated_tets(gpu_lib, nT):
    use = [i for i, cs in enumerate(CASES) if cs["X"] is not None and np.array_equal(cs["X"], fm.REG) and cs["energy"] == 0]
    pick = [use[t % len(use)] for t in range(nT)]
    free = range(nT // 3, nT // 2)  # a range in the middle carries no fibres
    X = np.vstack([fm.REG] * nT)
    x = np.vstack([CASES[i]["x"] for i in pick])
    T = (np.arange(4 * nT, dtype=np.int32)).reshape(nT, 4)
    c = _ctx(gpu_lib, X, T, x)
    for t, i in enumerate(pick):
        if t not in free:
            _set(c, t, t + 1, CASES[i])
    for g, a in ACTS.items():
        c.fiber_set_activation(g, a)
    f = c.features()
    assert c.fiber_get()["n"] == nT - len(free)
    per, g = c.fiber_energy_per_elem(), c.fiber_gradient_add(1.0, True)
    c.set_zero()
    c.fiber_hessian_add(1.0, True)
    H = _dense_upper(c)
    E = c.fiber_energy()
    assert c.fiber_energy() == E
    worst, Eref, Etol = 0.0, 0.0, 0.0
    for t, i in enumerate(pick):
        sl = slice(12 * t, 12 * t + 12)
        if t in free:
            assert per[t] == 0.0 and not g[sl].any() and not H[sl, sl].any()
            continue
        case, ref = _reference(i, f["restTriInv"][t], f["triArea"][t])
        if case["overflow"]:
            assert per[t] == np.inf and not g[sl].any() and not H[sl, sl].any()
            continue
        Eref, Etol = Eref + ref["E"], Etol + float(fm.tolerance(ref, "E"))
        worst = max(worst, _worst(per[t], ref, case, "perW"), _worst(g[sl], ref, case, "g"),
                    float(np.max(fm.ratio(H[sl, sl] - np.triu(ref["H"]), fm.tolerance(ref, "H") / fm.M))) / fm.M)
    assert not np.any(H - np.triu(H)) and np.count_nonzero(H) <= 78 * nT
    print(f"nT {nT}: worst error / tolerance {worst:.3g}")
    assert worst <= 1.0
    if any(CASES[i]["overflow"] for t, i in enumerate(pick) if t not in free):
        assert E == np.inf
    else:
        assert abs(E - Eref) <= Etol
    pe, tot = c.fiber_state()
    on = np.array([t not in free for t in range(nT)])
    assert tot[0] == pe[on, 0].min() and tot[1] == pe[on, 0].max() and np.all(pe[~on, 0] == 1.0) and not pe[~on, 1:].any()
    c.close()


def block_mesh(n=2, h=0.05):
    """n x n x n cubes of six tets each (Kuhn's subdivision), side h"""
    V = np.array([[i, j, k] for k in range(n + 1) for j in range(n + 1) for i in range(n + 1)], dtype=np.float64) * h
    nid = lambda i, j, k: i + (n + 1) * j + (n + 1) ** 2 * k
    T = []
    for ck in range(n):
        for cj in range(n):
            for ci in range(n):
                for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                    q, tet = [0, 0, 0], [nid(ci, cj, ck)]
                    for ax in p:
                        q[ax] = 1
                        tet.append(nid(ci + q[0], cj + q[1], ck + q[2]))
                    if np.linalg.det(V[tet[1:]] - V[tet[0]]) < 0:
                        tet[2], tet[3] = tet[3], tet[2]
                    T.append(tet)
    return V, np.array(T, dtype=np.int32)


def _block_case(c, X, T, x, dbc, specs):
    """the assembled fiber_mp case of a context: specs = [(t0, t1, a, k, law, k2, tension_only, act)]"""
    f = c.features()
    elems = []
    for t0, t1, a, k, law, k2, to, act in specs:
        for t in range(t0, t1):
            elems.append(fm.elem_record(f["restTriInv"][t], f["triArea"][t], T[t], a, k, law, k2, to, act))
    return {"x": x, "elems": elems, "dbc": dbc}


def test_shared_node_block_with_dirichlet_nodes(gpu_lib):
    X, T = block_mesh()
    rng = np.random.default_rng(11)
    x = fm.deformed(X, [0.3, -0.5, 0.8], 1.15, 0.95, fm.OBLIQUE, (0.1, 0.2, -0.1)) + 2e-3 * rng.normal(size=X.shape)
    dbc = np.zeros(len(X), dtype=np.int32)
    dbc[X[:, 0] == 0.0] = 1  # a Dirichlet face
    dbc[len(X) - 1] = 2
    c = _ctx(gpu_lib, X, T, x, dbc=dbc)
    specs = [(0, 20, [0.3, -0.5, 0.8], 4e4, fm.SPRING, 0.0, False, 0.3), (20, 34, [1.0, 0.0, 0.0], 2e4, fm.EXP, 3.0, False, 0.0),
             (38, 48, [0.0, 1.0, 1.0], 3e4, fm.SPRING, 0.0, True, -0.2)]
    for t0, t1, a, k, law, k2, to, act in specs:
        c.set_fibers((t0, t1), a, k, law=law, k2=k2, tension_only=to, group=GROUP_OF_ACT[act])
    for g, a in ACTS.items():
        c.fiber_set_activation(g, a)
    case = _block_case(c, X, T, x, dbc, specs)
    ref = fm.evaluate(case)  # per-element sums: sens and scale add up over the elements that share a node
    for proj in (True, False):
        g = c.fiber_gradient_add(1.0, proj)
        c.set_zero()
        c.fiber_hessian_add(1.0, proj)
        H = _dense_upper(c)
        wg = _worst(g, ref, case, "g", 1.0, proj)
        wH = float(np.max(fm.ratio(H - np.triu(fm.expected(case, ref, "H", 1.0, proj)[0]), fm.tolerance(ref, "H") / fm.M))) / fm.M
        print(f"block, projectDBC {int(proj)}: worst error / tolerance: gradient {wg:.3g}, matrix {wH:.3g}")
        assert wg <= 1.0 and wH <= 1.0
        drop = np.repeat((dbc == 1) | ((dbc == 2) & proj), 3)
        assert not g[drop].any() and not H[drop, :].any() and not H[:, drop].any() and g[~drop].any()
    assert _worst(c.fiber_energy(), ref, case, "E") <= 1.0
    c.close()


def test_lanes_that_are_off_write_nothing(gpu_lib):
    X, T = block_mesh()
    a = np.array([0.3, -0.5, 0.8])
    x = fm.deformed(X, a, 0.8, 1.1, fm.OBLIQUE, (0.1, 0.2, -0.1))  # compressed along the fibres
    c = _ctx(gpu_lib, X, T, x)
    c.set_fibers((0, 30), a, 4e4)  # plain springs: a matrix and a gradient that are not zero
    g0 = c.fiber_gradient_add(1.0, True, np.random.default_rng(3).normal(size=3 * len(X)))
    c.set_zero()
    c.fiber_hessian_add(1.0, True)
    a0 = c.get_a().copy()
    assert a0.any() and g0.any()
    c.set_fibers((0, 12), a, 4e4, tension_only=True)  # the later call overwrites
    c.set_fibers((12, 24), a, 4e4, law="exp", k2=2.0)
    c.set_fibers((24, 48), a, 0.0)  # and k = 0 removes: a fibre-free range
    assert c.fiber_get()["n"] == 24
    assert c.fiber_energy() == 0.0 and not c.fiber_energy_per_elem().any()
    g1 = c.fiber_gradient_add(1.0, True, g0)
    c.fiber_hessian_add(1.0, True)
    assert np.array_equal(g1.view(np.int64), g0.view(np.int64)) and np.array_equal(c.get_a().view(np.int64), a0.view(np.int64))  # bit-identical
    pe, tot = c.fiber_state()
    assert np.all(pe[:24, 1] == 0.0) and np.all(np.abs(pe[:24, 0] - 0.8) < 1e-12) and tot[2] == 0.0
    c.close()
