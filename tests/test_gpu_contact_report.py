"""`ipcgpu_contact_report` on hand-placed tuples against the mpmath restatement (tests/contact_report_mp.py); the consistency checks on a real two-body
scene are in test_gpu_contact_report_scene.py.

Hand-placed: the carrier mesh of stencil_mp (isolated unit tets), components of 1, 2, 5 and 16 tets (and 1 000 tets of one component each); every tuple's
two primitives sit on DIFFERENT tets, the geometry is stencil_mp._active_geometry moved onto the two tets.  All four kinds, PP and PE with multiplicity
above 1, mollified tuples of both encodings, tuples at or beyond dHat (one at dHat exactly, one at the largest distance below it that its coordinate
reaches), rows of 1, 256, 257 and 600 tuples interleaved in set order, a row whose primitive 1 lies in the higher component, a == b rows, one half-space
with vertices in two components and one beyond dHat, a lagged friction set.  Integers are exact; a double column of a row may differ by the sum of its
tuples' stencil_mp.tol(sens, scale) plus n u sum |t_i|.  The worst observed error / tolerance is printed (profiles/contact_report_timing.json records it)."""
import numpy as np
import pytest

import contact_report_mp as crm
import stencil_mp as smp

pytestmark = pytest.mark.gpu

DHAT = 2.0 ** -20  # sqrt = 2^-10: a PP pair along z at exactly that distance has d == dHat in doubles and in mp
KAPPA = 2.5e4
EPS2, COEF = 1.0e-10, 0.3
U = smp.U
S = 0.1  # size of the placed primitives
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -4  # include/ipcgpu.h
INT_FIELDS = ("a", "b", "nPP", "nPE", "nPT", "nEE", "nMollified", "argmin")
DBL_FIELDS = ("FA", "FB", "TA", "TB", "RA", "RB")

# (kind, tet of primitive 1, tet of primitive 2, multiplicity, copies in the set, what[, first local node]) -- tets 0 | 1-2 | 3-7 | 8-23 are the components 0 .. 3
SITES = [
    (smp.K_PP, 0, 1, 3, 600, "active"),  # row (0, 1): 600 records
    (smp.K_PE, 2, 3, 2, 257, "active"),  # row (1, 2): 257
    (smp.K_PT, 4, 8, 1, 100, "active"),  # row (2, 3): 100 + 100 + 56 = 256
    (smp.K_EE, 9, 5, 1, 100, "active"),  # primitive 1 in the higher component: sides swapped
    (smp.K_EE, 12, 6, 1, 56, "moll_ee"),  # mollified, the tuple holds the four edge nodes; swapped too
    (smp.K_PT, 10, 11, 1, 1, "active"),  # row (3, 3), a == b
    (smp.K_PE, 13, 14, 1, 1, "moll_pe"),  # mollified, a PE distance inside the edge pair of paraEEeIeJ
    (smp.K_PP, 15, 16, 2, 1, "ulp_below"),
    (smp.K_PP, 17, 18, 1, 1, "at_dhat"),  # d == dHat: contributes nothing, is not counted
    (smp.K_PT, 19, 7, 1, 1, "beyond"),  # d = 4 dHat; its row (2, 3) does not count it
    (smp.K_PE, 1, 2, 1, 1, "active", 2),  # row (1, 1): one record (on the local nodes 2, 3: the tets' nodes 0 belong to the first two sites)
]
N1 = {smp.K_PP: 1, smp.K_PE: 1, smp.K_PT: 1, smp.K_EE: 2}


def _layout(n_tets):
    """positions, tuples in mp form, the arrays for contact_set, the half-space, the friction move"""
    V, F, SF = smp.carrier_mesh(n_tets)
    X = V.copy()
    move = np.zeros_like(X)  # the step after the friction lag
    rng = np.random.default_rng(5)
    placed = []
    for si, (kind, tA, tB, mult, copies, what, *base) in enumerate(SITES):
        n, n1, k0 = smp.NN[kind], N1[kind], (base[0] if base else 0)
        h = 5.0e-4 + 2.0e-5 * si
        if what == "beyond":
            h = 2.0 ** -9
        par = (0.5, 0.4, 0.01) if what.startswith("moll") else None  # nearly parallel edges: c = S^4 sin^2 < eps_x = 1e-3
        if what.startswith("moll"):
            geo = smp._active_geometry(smp.K_EE, range(4), h, S, par)
            nodes4 = [4 * tA, 4 * tA + 1, 4 * tB, 4 * tB + 1]
        else:
            geo = smp._active_geometry(kind, range(n), h, S, par)
            nodes4 = [4 * tA + k0 + k for k in range(n1)] + [4 * tB + k0 + k for k in range(n - n1)]
        if what in ("ulp_below", "at_dhat"):  # along z from z = 0: the coordinate differences, hence d, are exact
            z = 2.0 ** -10 if what == "at_dhat" else np.nextafter(2.0 ** -10, 0.0)
            X[nodes4[0]] = (5.0, 30.0 + si, 0.0)
            X[nodes4[1]] = (5.0, 30.0 + si, z)
        else:
            R, off = smp._rot(si), np.array([3.0, 2.0 * si + 3.0, 5.0])
            for k, g in enumerate(nodes4):
                X[g] = R @ geo[k] + off
                move[g] = 2.0e-5 * rng.standard_normal(3) * (1.0 if k < n1 else 0.0)  # primitive 1 slides a little
        placed.append((kind, nodes4, mult, copies, what))
    return V, F, SF, X, move, placed


class Placed:
    def __init__(self, gpu_lib, n_tets, comp_tets):
        V, F, SF, X0, move, placed = _layout(n_tets)
        self.nV = V.shape[0]
        self.X0, self.X1 = X0, X0 + move
        self.comp = np.repeat(np.repeat(np.arange(len(comp_tets)), np.diff([0] + list(comp_tets))), 4)
        c = self.c = gpu_lib.Context(0)
        c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
        c.set_components(4 * np.asarray(comp_tets), np.asarray(comp_tets))
        c.opt_init(0.01, False)
        c.set_surface(SF)
        sfe = np.asarray(c.get_surface()[1])
        edges = smp.edge_lookup(sfe)
        act, par, eiej = [], [], []
        self.t_act, self.t_par = [], []
        for kind, g, mult, copies, what in placed:
            if what == "moll_ee" or what == "moll_pe":
                eI, eJ = edges[(min(g[0], g[1]), max(g[0], g[1]))], edges[(min(g[2], g[3]), max(g[2], g[3]))]
                en = [int(sfe[eI][0]), int(sfe[eI][1]), int(sfe[eJ][0]), int(sfe[eJ][1])]
                tup = (g[0], g[1], g[2], g[3]) if what == "moll_ee" else (-g[0] - 1, g[2], g[3], -1)
                nodes = list(g) if what == "moll_ee" else [g[0], g[2], g[3]]
                for _ in range(copies):
                    par.append(tup)
                    eiej.append((eI, eJ))
                    self.t_par.append(dict(src="moll", kind=kind, nodes=nodes, mult=1, edges=en, eps_x=1.0e-3))  # rest edges of length 1
                continue
            n = smp.NN[kind]
            q = list(g) + [0, 0]
            tup = {smp.K_EE: (q[0], q[1], q[2], q[3]), smp.K_PT: (-q[0] - 1, q[1], q[2], q[3]), smp.K_PE: (-q[0] - 1, q[1], q[2], -mult),
                   smp.K_PP: (-q[0] - 1, q[1], -1, -mult)}[kind]
            for _ in range(copies):
                act.append(tup)
                self.t_act.append(dict(src="active", kind=kind, nodes=list(g[:n]), mult=mult))
        order = np.random.default_rng(9).permutation(len(act))  # tuples of different rows interleaved in set order
        self.act = np.array(act, dtype=np.int32)[order]
        self.t_act = [self.t_act[i] for i in order]
        self.par, self.eiej = np.array(par, dtype=np.int32), np.array(eiej, dtype=np.int32)
        for i, t in enumerate(self.t_act + self.t_par):
            t["idx"] = i
        # one half-space below everything, normal +z: a vertex of component 0, one of the last component, one beyond dHat
        self.hs_n, self.hs_o = np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -20.0])
        self.hs_verts = [3, 4 * 20 + 3, 4 * 21 + 3]
        for X in (self.X0, self.X1):
            X[3, 2], X[4 * 20 + 3, 2], X[4 * 21 + 3, 2] = -20.0 + 4.0e-4, -20.0 + 6.0e-4, -20.0 + 2.0e-3
        self.hs = c.add_half_space(self.hs_o, self.hs_n)
        c.halfspace_set(self.hs, self.hs_verts)
        self.t_hs = [dict(src="hs", kind=smp.K_PP, nodes=[v], mult=1, idx=v, h=self.hs, n=self.hs_n, D=20.0) for v in self.hs_verts]
        c.contact_set(self.act, self.par, self.eiej)
        c.set_positions(self.X0)
        c.friction_update(DHAT, KAPPA)  # lags the active list at X0
        c.set_positions(self.X1)
        self.t_fric = [dict(t, src="fric", idx=-1, lag=self.X0, lag_kappa=KAPPA, lag_dhat=DHAT, eps2=EPS2, coef=COEF) for t in self.t_act]

    def tuples(self):
        return self.t_act + self.t_par + self.t_hs + self.t_fric

    def report(self, **kw):
        return self.c.contact_report(DHAT, KAPPA, x_prev=self.X0, eps2=EPS2, coef=COEF, **kw)


def _key(t):
    return (t["src"], t["kind"], tuple(t["nodes"]), t["mult"])


def reference(P):
    """rows of the mp restatement with the tolerance of every double column; distinct tuples are evaluated once"""
    Xp, X0p = smp.perturbed(P.X1, 77), smp.perturbed(P.X0, 78)
    cache, recs, sens, scale = {}, [], [], []
    for t in P.tuples():
        k = _key(t)
        if k not in cache:
            r = crm.record(t, P.X1, P.X0, P.comp, DHAT, KAPPA)
            tp = dict(t, lag=X0p) if t["src"] == "fric" else t
            rp = crm.record(tp, Xp, X0p, P.comp, DHAT, KAPPA)
            if r is None:
                cache[k] = None
            else:
                v = [float(x) for x in crm.record_values(r)]
                vp = [float(x) for x in crm.record_values(rp)] if rp is not None else [0.0] * 19
                ds = abs(float(rp["d"] - r["d"])) if (rp is not None and r["d"] is not None) else 0.0
                cache[k] = (r, np.abs(np.array(vp) - np.array(v)), crm.column_scales(r), np.abs(v), ds)
        c = cache[k]
        recs.append(None if c is None else dict(c[0], idx=t["idx"]))
        sens.append(c)
    rows = crm.row_table(recs)
    for row in rows:
        tol, mag, dtol = np.zeros(19), np.zeros(19), 0.0
        for i in row["members"]:
            _r, s, sc, av, ds = sens[i]
            tol += smp.tol(s, sc)
            mag += av
            if recs[i]["src"] != "fric" and recs[i]["idx"] == row["argmin"]:
                dtol = float(smp.tol(ds, float(recs[i]["d"])))
        row["tol"] = tol + len(row["members"]) * U * mag
        row["dtol"] = dtol
    return rows


def compare(got, rows):
    assert len(got) == len(rows), ([(r["a"], r["b"]) for r in rows], got[["a", "b"]])
    worst = 0.0
    for g, r in zip(got, rows):
        want_i = [r["a"], r["b"]] + r["counts"] + [r["argmin"]]
        assert [int(g[k]) for k in INT_FIELDS] == want_i, (want_i, g)
        if r["argmin"] < 0:
            assert g["minD2"] == np.inf
        else:
            err = abs(float(g["minD2"]) - float(r["minD2"]))
            worst = max(worst, err / r["dtol"])
            assert err <= r["dtol"], (r["a"], r["b"], err, r["dtol"])
        gv = np.concatenate([g[k] for k in DBL_FIELDS] + [[g["W"]]])
        wv = np.array([float(x) for x in r["vals"]])
        err = np.abs(gv - wv)
        ok = r["tol"] > 0
        assert np.all(err[~ok] == 0.0), (r["a"], r["b"], err, r["tol"])
        worst = max(worst, float((err[ok] / r["tol"][ok]).max()) if ok.any() else 0.0)
        assert np.all(err <= r["tol"]), (r["a"], r["b"], err / np.where(ok, r["tol"], 1.0))
    return worst


@pytest.fixture(scope="module")
def placed24(gpu_lib):
    P = Placed(gpu_lib, 24, [1, 3, 8, 24])
    yield P
    P.c.close()


def test_hand_placed_rows_against_mpmath(placed24):
    P = placed24
    got = P.report()
    rows = reference(P)
    keys = [(r["a"], r["b"]) for r in rows]
    assert keys == [(0, 1), (0, -1), (1, 1), (1, 2), (2, 3), (3, 3), (3, -1)]
    by = {k: r for k, r in zip(keys, rows)}
    assert [len(by[k]["members"]) for k in ((0, 1), (1, 2), (1, 1))] == [1200, 514, 2]  # barrier + friction records: 600, 257 and 1 tuples
    assert by[(2, 3)]["counts"] == [0, 0, 100, 100, 56] and by[(3, 3)]["counts"] == [1, 0, 1, 0, 1]  # the tuple at dHat and the one beyond are not counted
    assert by[(3, -1)]["counts"][0] == 1 and by[(0, -1)]["counts"][0] == 1  # the third vertex of the plane's set is beyond dHat
    worst = compare(got, rows)
    print(f"contact report, 24 tets: {len(rows)} rows, worst error / tolerance {worst:.3g}")
    # sides: in row (2, 3) the EE and the mollified tuples have primitive 1 in component 3 -- the barrier pushes side A (component 2, above or below) away
    g = got[4]
    assert np.any(g["FA"] != 0.0) and np.any(g["RA"] != 0.0) and g["W"] <= 0.0


def test_report_is_reproducible_and_changes_nothing(placed24, gpu_lib):
    P = placed24
    before = (P.c.contact_held(), np.asarray(P.c.get_positions()).copy())
    a, b = P.report(), P.report()
    assert a.tobytes() == b.tobytes()
    Q = Placed(gpu_lib, 24, [1, 3, 8, 24])
    try:
        assert Q.report().tobytes() == a.tobytes()
    finally:
        Q.c.close()
    held = P.c.contact_held()
    assert all(np.array_equal(held[k], before[0][k]) for k in held) and np.array_equal(P.c.get_positions(), before[1])
    assert len(held["active"]) == len(P.act) and len(held["para"]) == len(P.par)
    # the handler's own scatter still works on counters the report left alone
    g1 = P.c.contact_gradient_add(DHAT, KAPPA, projectDBC=False)
    a2 = P.report()
    g2 = P.c.contact_gradient_add(DHAT, KAPPA, projectDBC=False)
    assert a2.tobytes() == a.tobytes() and g1.tobytes() == g2.tobytes()
    # without x_prev: no friction part, the barrier part unchanged; rows that exist through friction alone are gone
    nb = P.c.contact_report(DHAT, KAPPA)
    assert np.all(nb["RA"] == 0.0) and np.all(nb["W"] == 0.0) and np.all(nb["minD2"] < DHAT)
    keep = a[a["minD2"] < np.inf]
    for k in INT_FIELDS + ("minD2", "FA", "FB", "TA", "TB"):
        assert nb[k].tobytes() == keep[k].tobytes(), k


def test_default_components_and_error_codes(gpu_lib):
    import ctypes as C
    V, F, SF, X, _move, _placed = _layout(24)
    c = gpu_lib.Context(0)
    try:
        L = c._L
        n = C.c_int(-5)
        call = lambda cap, ri, rd: L.ipcgpu_contact_report(c.h, C.c_double(DHAT), C.c_double(KAPPA), None, C.c_double(0.0), C.c_double(0.0), C.c_int(cap),
                                                            C.byref(n), ri, rd)
        c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
        c.opt_init(0.01, False)
        assert call(0, None, None) == ERR_STATE  # before set_surface
        c.set_surface(SF)
        assert call(0, None, None) == 0 and n.value == 0  # nothing held: no row
    finally:
        c.close()
    P = Placed(gpu_lib, 24, [24])  # one component: a single (0, 0) row plus the half-space row
    try:
        got = P.report()
        assert [(int(r["a"]), int(r["b"])) for r in got] == [(0, 0), (0, -1)]
        assert int(got[0]["nPP"]) == 601 and int(got[0]["nMollified"]) == 57 and int(got[1]["nPP"]) == 2
        L = P.c._L
        n = C.c_int(-5)
        ri, rd = np.zeros((1, 8), dtype=np.int32), np.zeros((1, 20))
        rc = L.ipcgpu_contact_report(P.c.h, C.c_double(DHAT), C.c_double(KAPPA), None, C.c_double(0.0), C.c_double(0.0), C.c_int(1), C.byref(n),
                                     ri.ctypes.data_as(C.POINTER(C.c_int)), rd.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == ERR_ARG and n.value == 2  # capacity too small: the size comes back
        rc = L.ipcgpu_contact_report(P.c.h, C.c_double(DHAT), C.c_double(KAPPA), None, C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.byref(n), None, None)
        assert rc == ERR_ARG and n.value == 2
        P.c.set_shard(0, 2)
        rc = L.ipcgpu_contact_report(P.c.h, C.c_double(DHAT), C.c_double(KAPPA), None, C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.byref(n), None, None)
        assert rc == ERR_UNSUPPORTED
    finally:
        P.c.close()


def test_a_thousand_components(gpu_lib):
    """one component per tet: 501 500 keys, every row a pair of single tets"""
    P = Placed(gpu_lib, 1000, list(range(1, 1001)))
    try:
        got = P.report()
        rows = reference(P)
        assert [(r["a"], r["b"]) for r in rows][:3] == [(0, 1), (0, -1), (1, 2)] and len(rows) == 13
        worst = compare(got, rows)
        print(f"contact report, 1000 components: {len(rows)} rows, worst error / tolerance {worst:.3g}")
        # The record kernels restate the per-node terms of k_contact_gradient, the half-space gradient kernel and k_friction_gradient (those are inline in
        # their kernels).  Where a row holds ONE tuple whose nodes no other tuple touches, the report must be minus those kernels' output, the same doubles:
        # the PT tuple of tets (10, 11), the plane vertex of tet 20, and the same PT tuple in the lagged friction set.
        by = {(int(r["a"]), int(r["b"])): r for r in got}
        g = P.c.contact_gradient_add(DHAT, KAPPA, projectDBC=False).reshape(-1, 3)
        gh = P.c.halfspace_gradient_add(P.hs, DHAT, KAPPA).reshape(-1, 3)
        gf = P.c.friction_gradient_add(P.X0, EPS2, COEF).reshape(-1, 3)
        r = by[(10, 11)]
        assert int(r["nPT"]) == 1 and np.any(g[40] != 0.0) and np.any(gf[40] != 0.0)
        # (array_equal: the same doubles; an exact zero may differ in sign, 0.0 + -0.0 in the gradient's accumulation)
        assert np.array_equal(-g[40], r["FA"]) and np.array_equal(((-g[44]) + (-g[45])) + (-g[46]), r["FB"])
        assert np.array_equal(-gf[40], r["RA"]) and np.array_equal(((-gf[44]) + (-gf[45])) + (-gf[46]), r["RB"])
        assert np.array_equal(-gh[83], by[(20, -1)]["FA"]) and np.any(gh[83] != 0.0)
    finally:
        P.c.close()
