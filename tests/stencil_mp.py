"""Per-stencil reference of barrier contact and lagged friction in plain mpmath, the hand-placed cases and their carrier mesh.

A helper module (like pcg_numpy.py), used by test_stencil_mp.py, test_gpu_stencils_mp.py and tools/make_stencil_mp_golden.py.  Nothing here shares
code or arithmetic with ipc_amd/ or oracle/: squared distances, barrier, mollifier and the friction potential are written from their definitions on
the exact doubles handed to the GPU (mp.dps = 100), gradients and Hessians are central differences of those ENERGIES with a step of 1e-20 x the
stencil's size (truncation ~1e-30 relative, cancellation leaves > 40 digits), the PSD projection is mp.eigsy with negative eigenvalues clamped, and
blocks of projected Dirichlet nodes are dropped after the projection.

  d_PP = |a-b|^2        d_PE = |(p-a)x(b-a)|^2 / |b-a|^2        d_PT = ((p-a).n)^2 / n.n, n = (b-a)x(c-a)        d_EE = ((c-a).n)^2 / n.n, n = (b-a)x(d-c)
  b(d) = -(d-dHat)^2 ln(d/dHat)       c = |(a1-a0)x(b1-b0)|^2       eps_x = 1e-3 |a1-a0|^2 |b1-b0|^2 (rest)       e(c) = (2 - c/eps_x) c/eps_x below eps_x, else 1
  active stencil: kappa mult b(d(x))        mollified: kappa e(c(x_E)) b(d(x_S))        friction: coef lam f0(|u|), u = B^T sum_k wt_k (x_k - xt_k), lagged lam, wt, B fixed

Carrier mesh: N isolated unit tetrahedra, tet t owns nodes 4t..4t+3, 10 apart, the surface is all faces.  Every stencil lives on the nodes of ONE tet, so
the mesh pattern already couples its nodes and every output entry (12 gradient entries, the upper 12 x 12 of the tet) belongs to exactly one stencil.

Tolerance of a quantity q of one stencil:  tol(q) = M (sens(q) + u scale),  u = 2^-53, scale = the largest magnitude in that stencil's own gradient / block
(before the rows of Dirichlet nodes are dropped; |E| for an energy), sens(q) = |q_mp(x~) - q_mp(x)| with every input coordinate moved by a fixed random +-4 ulp (the conditioning: d - dHat at d ~ dHat and
(p-a).n at tiny gaps are ill-conditioned by nature).  M was measured on the CPU against the oracle (oracle/orc_contact.cpp, orc_friction.cpp: an independent
double implementation, not the code under test) over all cases of tests/golden/stencil_mp_cases.npz:
    worst err / (sens + u scale) of the oracle = 118 (ORACLE_WORST_RATIO),  M = 8 x that rounded up to a power of two = 1024.
The worst cases are the thin ones (sliver triangle, barycentric coordinate 1e-6, edges a few 1e-3 rad apart): the formula d = s^2 / q loses what the thin
direction costs, one random perturbation does not always show as much.  Cases the oracle missed by more than 128 were replaced, not excused (REPLACED below,
and the mollified cases of c / eps_x = 1e-8 sit on a compressed tet).  test_stencil_mp.py::test_oracle_meets_the_tolerance pins M.
"""
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 100

K_PP, K_PE, K_PT, K_EE = 0, 1, 2, 3
NN = (2, 3, 4, 4)
DHAT = 1.0e-6  # one squared activation distance for every case (the C ABI takes one per call); the gap ratios come from the stencils' sizes
KAPPAS = (1.0, 2.5e4)
U = 2.0 ** -53
ORACLE_WORST_RATIO = 118.0  # measured (tools/make_stencil_mp_golden.py --measure prints it): contact 118 (a sliver triangle's grad d), shared point 57.7, friction 20.1
M = 1024.0  # 8 x 118 = 944 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stencil_mp_cases.npz")

REST = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
PITCH = 10.0
TET_FACES = ((0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3))
EDGE_PAIRS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))


# ---- carrier mesh ----------------------------------------------------------------------------------------------------------------------------
def carrier_mesh(n):
    """(rest positions, tets, surface triangles) of n isolated unit tets"""
    V = np.tile(REST, (n, 1))
    V[:, 0] += PITCH * np.repeat(np.arange(n), 4)
    F = np.arange(4 * n, dtype=np.int32).reshape(n, 4)
    SF = np.array([[4 * t + a for a in f] for t in range(n) for f in TET_FACES], dtype=np.int32)
    return V, F, SF


def edge_lookup(sfe):
    """{(lo, hi): surface edge index} of get_surface()'s edge list"""
    return {(min(int(a), int(b)), max(int(a), int(b))): i for i, (a, b) in enumerate(np.asarray(sfe))}


def tuples_of(case, tet, edges=None):
    """(MMCVID tuple, para_eiej or None) of `case` placed on tet `tet`"""
    g = [4 * tet + int(k) for k in case["nodes"][:NN[case["kind"]]]]
    mult = -int(case["mult"])
    if case["kind"] == K_EE:
        t = (g[0], g[1], g[2], g[3])
    elif case["kind"] == K_PT:
        t = (-g[0] - 1, g[1], g[2], g[3])
    elif case["kind"] == K_PE:
        t = (-g[0] - 1, g[1], g[2], mult)
    else:
        t = (-g[0] - 1, g[1], -1, mult)
    if not case["para"]:
        return t, None
    e = [4 * tet + int(k) for k in case["edges"]]
    return t, (edges[(min(e[0], e[1]), max(e[0], e[1]))], edges[(min(e[2], e[3]), max(e[2], e[3]))])


def bin_of(case):
    return (4 if case["para"] else 0) + int(case["kind"])


# ---- mp primitives ---------------------------------------------------------------------------------------------------------------------------
def _pts(X):
    return [[mpf(float(v)) for v in p] for p in np.asarray(X, dtype=np.float64).reshape(-1, 3)]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dist2(kind, P):
    if kind == K_PP:
        r = _sub(P[0], P[1])
        return _dot(r, r)
    if kind == K_PE:
        e = _sub(P[2], P[1])
        n = _cross(_sub(P[0], P[1]), e)
        return _dot(n, n) / _dot(e, e)
    if kind == K_PT:
        n = _cross(_sub(P[2], P[1]), _sub(P[3], P[1]))
        s = _dot(_sub(P[0], P[1]), n)
        return s * s / _dot(n, n)
    n = _cross(_sub(P[1], P[0]), _sub(P[3], P[2]))
    s = _dot(_sub(P[2], P[0]), n)
    return s * s / _dot(n, n)


def barrier(d, dHat):
    return -(d - dHat) ** 2 * mp.log(d / dHat)


def barrier_d1(d, dHat):
    return -2 * (d - dHat) * mp.log(d / dHat) - (d - dHat) ** 2 / d


def cross_norm(P):
    n = _cross(_sub(P[1], P[0]), _sub(P[3], P[2]))
    return _dot(n, n)


def mollifier(c, eps_x):
    return (2 - c / eps_x) * (c / eps_x) if c < eps_x else mpf(1)


def eps_x_rest(edges):
    """on the carrier mesh's rest shape (exact: its coordinates are integers)"""
    la = float(((REST[edges[1]] - REST[edges[0]]) ** 2).sum())
    lb = float(((REST[edges[3]] - REST[edges[2]]) ** 2).sum())
    return mpf("1e-3") * mpf(la) * mpf(lb)


def f0(y, eps):
    """f0_SF_C1: |u| beyond eps, the C1 cubic below"""
    return y if y > eps else -y ** 3 / (3 * eps ** 2) + y ** 2 / eps + eps / 3


# ---- derivatives by central differences, projection ----------------------------------------------------------------------------------------
def _derivs(E, y, idx, h, hessian=True):
    """E(y), gradient (12) and Hessian (12 x 12, lists of mpf) of E over the coordinates idx of y"""
    def at(*shifts):
        z = list(y)
        for i, s in shifts:
            z[i] = z[i] + s * h
        return E(z)
    E0 = E(y)
    g = [mpf(0)] * 12
    H = [[mpf(0)] * 12 for _ in range(12)]
    Ep = {i: at((i, 1)) for i in idx}
    Em = {i: at((i, -1)) for i in idx}
    for i in idx:
        g[i] = (Ep[i] - Em[i]) / (2 * h)
    if hessian:
        for a, i in enumerate(idx):
            H[i][i] = (Ep[i] - 2 * E0 + Em[i]) / (h * h)
            for j in idx[a + 1:]:
                H[i][j] = H[j][i] = (at((i, 1), (j, 1)) - at((i, 1), (j, -1)) - at((i, -1), (j, 1)) + at((i, -1), (j, -1))) / (4 * h * h)
    return E0, g, H


def project_psd(H, idx):
    n = len(idx)
    A = mp.matrix(n, n)
    for a, i in enumerate(idx):
        for b, j in enumerate(idx):
            A[a, b] = H[i][j]
    ev, Q = mp.eigsy(A)
    P = [[mpf(0)] * 12 for _ in range(12)]
    for k in range(n):
        if ev[k] > 0:
            for a, i in enumerate(idx):
                for b, j in enumerate(idx):
                    P[i][j] += ev[k] * Q[a, k] * Q[b, k]
    return P


def _drop(g, H, dbc):
    for k in dbc:
        for c in range(3):
            g[3 * k + c] = mpf(0)
            for j in range(12):
                H[3 * k + c][j] = H[j][3 * k + c] = mpf(0)


def _f(v):
    return np.array([float(x) for x in v])


def _coords(nodes):
    return [3 * int(k) + c for k in nodes for c in range(3)]


def _size(case):
    return mpf(float(case["size"]))


def contact_reference(case, X):
    """d, grad d (12), E, gradient (12), projected Hessian (12 x 12) of `case` at the tet's node positions X (4 x 3 doubles), as doubles"""
    kind, nodes = int(case["kind"]), [int(k) for k in case["nodes"][:NN[int(case["kind"])]]]
    kappa, mult, dHat = mpf(float(case["kappa"])), mpf(int(case["mult"])), mpf(DHAT)
    y = [c for p in _pts(X) for c in p]
    h = mpf("1e-20") * _size(case)

    def dfun(z):
        return dist2(kind, [z[3 * k:3 * k + 3] for k in nodes])
    if case["para"]:
        edges = [int(k) for k in case["edges"]]
        ex = eps_x_rest(edges)
        used = sorted(set(edges))

        def E(z):
            return kappa * mollifier(cross_norm([z[3 * k:3 * k + 3] for k in edges]), ex) * barrier(dfun(z), dHat)
    else:
        used = sorted(set(nodes))

        def E(z):
            return kappa * mult * barrier(dfun(z), dHat)
    d, gd, _ = _derivs(dfun, y, _coords(nodes), h, hessian=False)
    E0, g, H = _derivs(E, y, _coords(used), h)
    P = project_psd(H, _coords(used))
    # the scale of the round-off: the stencil's own gradient and projected block BEFORE Dirichlet rows are dropped (what is left of a block after the
    # drop may be exactly zero in exact arithmetic, while the projection's round-off in it is relative to the block that was projected)
    gscale, Hscale = float(max(abs(v) for v in g)), float(max(abs(v) for r in P for v in r))
    _drop(g, P, [int(k) for k in case["dbc"] if k >= 0])
    return dict(d=float(d), gd=_f(gd), E=float(E0), g=_f(g), H=np.array([_f(r) for r in P]), gscale=gscale, Hscale=Hscale)


def _unit(a):
    l = mp.sqrt(_dot(a, a))
    return [a[0] / l, a[1] / l, a[2] / l]


def friction_lag(case, X):
    """lam, closest-point coordinates (2), node weights (4), tangent basis (two unit 3-vectors) at the lagged positions X, in mp"""
    kind, nodes = int(case["kind"]), [int(k) for k in case["nodes"][:NN[int(case["kind"])]]]
    P = [_pts(X)[k] for k in nodes]
    d = dist2(kind, P)
    lam = -2 * mpf(float(case["kappa"])) * mp.sqrt(d) * barrier_d1(d, mpf(DHAT)) * int(case["mult"])
    co = [mpf(0), mpf(0)]
    if kind == K_EE:  # closest points a0 + g0 (a1-a0), b0 + g1 (b1-b0): the 2 x 2 normal equations of their distance
        ea, eb, r = _sub(P[1], P[0]), _sub(P[3], P[2]), _sub(P[0], P[2])
        a, b, c = _dot(ea, ea), -_dot(ea, eb), _dot(eb, eb)
        r0, r1 = -_dot(r, ea), _dot(r, eb)
        det = a * c - b * b
        co = [(c * r0 - b * r1) / det, (a * r1 - b * r0) / det]
        wt = [1 - co[0], co[0], co[1] - 1, -co[1]]
        t0 = ea
        t1 = _cross(_cross(ea, eb), ea)
    elif kind == K_PT:  # closest point a + b1 (b-a) + b2 (c-a)
        e1, e2, w = _sub(P[2], P[1]), _sub(P[3], P[1]), _sub(P[0], P[1])
        a, b, c = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        r0, r1 = _dot(e1, w), _dot(e2, w)
        det = a * c - b * b
        co = [(c * r0 - b * r1) / det, (a * r1 - b * r0) / det]
        wt = [mpf(1), co[0] + co[1] - 1, -co[0], -co[1]]
        t0 = e1
        t1 = _cross(_cross(e1, e2), e1)
    elif kind == K_PE:
        e, w = _sub(P[2], P[1]), _sub(P[0], P[1])
        co[0] = _dot(w, e) / _dot(e, e)
        wt = [mpf(1), co[0] - 1, -co[0], mpf(0)]
        t0 = e
        t1 = _cross(e, w)
    else:  # cross with e_x or e_y, whichever gives the longer vector (e_y on a tie)
        v = _sub(P[1], P[0])
        xc, yc = _cross([mpf(1), mpf(0), mpf(0)], v), _cross([mpf(0), mpf(1), mpf(0)], v)
        t0 = xc if _dot(xc, xc) > _dot(yc, yc) else yc
        t1 = _cross(v, t0)
        wt = [mpf(1), mpf(-1), mpf(0), mpf(0)]
    return lam, co, wt, _unit(t0), _unit(t1)


def friction_reference(case, X, Xn):
    """lagged data at X and energy, gradient, projected Hessian of coef lam f0(|u|) at Xn, as doubles"""
    nodes = [int(k) for k in case["nodes"][:NN[int(case["kind"])]]]
    lam, co, wt, t0, t1 = friction_lag(case, X)
    xt = [c for p in _pts(X) for c in p]
    y = [c for p in _pts(Xn) for c in p]
    eps, coef = mp.sqrt(mpf(float(case["eps2"]))), mpf(float(case["coef"]))

    def slide(z):
        r = [sum(wt[a] * (z[3 * k + c] - xt[3 * k + c]) for a, k in enumerate(nodes)) for c in range(3)]
        return _dot(t0, r), _dot(t1, r)

    def E(z):
        u0, u1 = slide(z)
        return coef * lam * f0(mp.sqrt(u0 * u0 + u1 * u1), eps)
    E0, g, H = _derivs(E, y, _coords(nodes), mpf("1e-20") * _size(case))
    P = project_psd(H, _coords(nodes))
    u0, u1 = slide(y)
    return dict(lam=float(lam), coord=_f(co), basis=_f(t0 + t1), u2=u0 * u0 + u1 * u1, E=float(E0), g=_f(g), H=np.array([_f(r) for r in P]))


def perturbed(X, seed):
    """every coordinate moved by +-4 ulp, the signs fixed by `seed` (zeros stay: they have no ulp to speak of)"""
    X = np.asarray(X, dtype=np.float64)
    up = np.random.default_rng(seed).integers(0, 2, size=X.shape).astype(bool)
    Y = X.copy()
    for _ in range(4):
        Y = np.where(X == 0.0, Y, np.nextafter(Y, np.where(up, np.inf, -np.inf)))
    return Y


def tol(sens, scale):
    return M * (np.asarray(sens) + U * scale)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def _rot(seed):
    Q, _ = np.linalg.qr(np.random.default_rng(1000 + seed).normal(size=(3, 3)))
    return Q


def _place(pts, size, rot, shift=0.0):
    """4 x 3 positions of a tet's nodes: the given local nodes at pts, the others parked a few sizes away; rotated, then shifted"""
    X = np.zeros((4, 3))
    for k in range(4):
        X[k] = pts[k] if k in pts else np.array([3.0 + k, 2.0 - k, 4.0]) * size
    if rot is not None:
        X = X @ _rot(rot).T
    return X + shift


def _active_geometry(kind, nodes, h, s, par=None, asp=0.9):
    z = np.array([0.0, 0.0, h])
    if kind == K_PP:
        p = [np.zeros(3), z]
    elif kind == K_PE:
        t = 0.4 if par is None else par
        p = [z, np.array([-t * s, 0, 0]), np.array([(1 - t) * s, 0, 0])]
    elif kind == K_PT:
        w = np.array((0.3, 0.3, 0.4) if par is None else par)
        tri = np.array([[0, 0, 0], [s, 0, 0], [0.3 * s, asp * s, 0]])
        foot = w @ tri
        p = [z] + [q - foot for q in tri]
    else:
        sa, sb, th = (0.5, 0.4, 1.1) if par is None else par
        dr = np.array([np.cos(th), np.sin(th), 0.0])
        p = [np.array([-sa * s, 0, 0]), np.array([(1 - sa) * s, 0, 0]), -sb * s * dr + z, (1 - sb) * s * dr + z]
    return {int(k): q for k, q in zip(nodes, p)}


def _case(kind, nodes, X, size, kappa, mult=1, para=False, edges=(-1, -1, -1, -1), dbc=(), name=""):
    nodes = list(nodes) + [-1] * (4 - len(nodes))
    return dict(kind=kind, nodes=np.array(nodes), X=np.asarray(X, dtype=np.float64), size=float(size), kappa=float(kappa), mult=int(mult), para=bool(para),
                edges=np.array(edges), dbc=np.array(list(dbc) + [-1] * (2 - len(dbc))), name=name)


def _d_of(case, X):
    return dist2(case["kind"], [_pts(X)[int(k)] for k in case["nodes"][:NN[case["kind"]]]])


def _one_ulp_below(case):
    """move the coordinate d depends on most by single ulps until d is the largest value below dHat that this coordinate reaches"""
    X = case["X"]
    k0 = int(case["nodes"][0])
    best, gain = 0, -1.0
    for c in range(3):
        Y = X.copy()
        Y[k0, c] = np.nextafter(Y[k0, c], np.inf)
        dd = abs(float(_d_of(case, Y) - _d_of(case, X)))
        if dd > gain:
            best, gain = c, dd
    Y = X.copy()
    Y[k0, best] = np.nextafter(Y[k0, best], np.inf)
    up = np.inf if _d_of(case, Y) > _d_of(case, X) else -np.inf  # the direction in which d grows
    for _ in range(100000):
        if _d_of(case, X) < DHAT:
            break
        X[k0, best] = np.nextafter(X[k0, best], -up)
    for _ in range(100000):
        Y = X.copy()
        Y[k0, best] = np.nextafter(Y[k0, best], up)
        if not _d_of(case, Y) < DHAT:
            break
        X[k0, best] = Y[k0, best]
    assert _d_of(case, X) < DHAT
    return case


NODE_ORDERS = {K_PP: [(0, 1), (3, 1), (2, 0)], K_PE: [(0, 1, 2), (3, 0, 2), (1, 3, 0)], K_PT: [(0, 1, 2, 3), (2, 3, 0, 1), (3, 1, 0, 2)],
               K_EE: [(0, 1, 2, 3), (2, 0, 3, 1), (1, 3, 2, 0)]}


# cases whose first placement the ORACLE missed by more than 128 (sens + u scale) -- too ill-conditioned in that orientation to test anything: replaced by the
# same configuration under another rotation (number of replacements per (kind, running number))
REPLACED = {(K_PT, 12): 1, (K_PT, 14): 1, (K_PT, 15): 2, (K_PT, 18): 1, (K_EE, 8): 1}


def _active_cases(kind):
    out, n = [], 0

    def add(gap, ratio, par=None, asp=0.9, dbc=(), scale_shift=None, name="", ulp=False):
        nonlocal n
        nodes = NODE_ORDERS[kind][n % 3]
        h = float(np.sqrt(DHAT / ratio))
        s = h / gap
        shift = 0.0
        if scale_shift:
            shift = scale_shift
        X = _place(_active_geometry(kind, nodes, h, s, par, asp), s, rot=10 * kind + n + 500 * REPLACED.get((kind, n), 0), shift=shift)
        mult = (1, 2, 3)[n % 3] if kind in (K_PP, K_PE) else 1
        c = _case(kind, nodes, X, s, KAPPAS[n % 2], mult, dbc=dbc, name=f"{'PP PE PT EE'.split()[kind]} gap {gap:g} dHat/d {ratio:g} {name}".strip())
        out.append(_one_ulp_below(c) if ulp else c)
        n += 1
    for gap in (1e-1, 1e-3, 1e-5):
        for ratio in (1.0001, 2.0, 100.0):
            add(gap, ratio)
    add(1e-1, 1.0, name="d one ulp below dHat", ulp=True)
    add(1e-1, 2.0, scale_shift=1e2, name="small, translated by 1e2")  # sqrt(d) ~ 7e-4 at coordinates of 1e2
    add(1e-2, 2.0, scale_shift=1e2, name="small, translated by 1e2")
    if kind == K_PE:
        add(1e-3, 2.0, par=1e-6, name="foot at 1e-6 of the edge")
        add(1e-1, 100.0, par=1 - 1e-6, name="foot at 1 - 1e-6 of the edge")
    elif kind == K_PT:
        add(1e-3, 2.0, par=(1e-6, 0.5, 0.5 - 1e-6), name="barycentric coordinate 1e-6")
        add(1e-1, 100.0, par=(0.6 - 1e-6, 1e-6, 0.4), name="barycentric coordinate 1e-6")
        add(1e-3, 2.0, asp=1e-3, name="sliver triangle of aspect 1e-3")
        add(1e-1, 1.0001, asp=1e-3, name="sliver triangle of aspect 1e-3")
    elif kind == K_EE:
        add(1e-3, 2.0, par=(1e-6, 0.4, 1.1), name="crossing parameter 1e-6")
        add(1e-1, 100.0, par=(0.5, 1 - 1e-6, 0.7), name="crossing parameter 1 - 1e-6")
        add(1e-2, 2.0, par=(0.5, 0.5, 0.05), name="edges 0.05 rad apart")
    else:
        add(1e-2, 2.0)
        add(1e-4, 100.0)
    # Dirichlet copies: one or two type-1 nodes of the stencil
    for gap, ratio, nd in ((1e-1, 2.0, 1), (1e-3, 100.0, 1), (1e-2, 1.0001, 2), (1e-5, 2.0, 2)):
        nodes = NODE_ORDERS[kind][n % 3]
        add(gap, ratio, dbc=tuple(nodes[-nd:]) if nd < NN[kind] else tuple(nodes[:1]), name=f"{nd} Dirichlet node(s)")
    while len(out) < 20:
        add((3e-2, 3e-4)[n % 2], (1.5, 10.0, 1.01)[n % 3])
    return out


PARA_SUBS = {K_PP: [(0, 2), (0, 3), (1, 2), (1, 3)], K_PE: [(0, 2, 3), (1, 2, 3), (2, 0, 1), (3, 0, 1)], K_EE: [(0, 1, 2, 3)]}  # positions in (a0, a1, b0, b1)
C_RATIOS = (1e-8, 0.5, 1 - 1e-9, 1 + 1e-9, 10.0)


def _para_cases(kind):
    out, n = [], 0
    for rep in range(4):
        for r in C_RATIOS:
            sub = PARA_SUBS[kind][n % len(PARA_SUBS[kind])]
            pair = EDGE_PAIRS[n % 3]
            edges = (pair[0] + pair[1]) if (n // 3) % 2 == 0 else (pair[1][::-1] + pair[0])
            ratio = (2.0, 100.0, 1.0001, 1.5)[rep]
            s = (1.0, 0.6, 2.5, 1.0)[rep] * (0.02 if r < 1e-6 else 1.0)  # c / eps_x = 1e-8 at unit size is an angle of 4e-6: no double formula of d_EE survives it
            h = float(np.sqrt(DHAT / ratio))
            ex = float(eps_x_rest(edges))
            sin = np.sqrt(r * ex) / (s * s)
            th = float(np.arcsin(sin))
            sa, sb = 0.5, 0.4
            if kind == K_PP:
                sa, sb = float(sub[0]), float(sub[1] - 2)
            elif kind == K_PE:
                sa, sb = (float(sub[0]), 0.3) if sub[0] < 2 else (0.3, float(sub[0] - 2))
            z = np.array([0.0, 0.0, h])
            dr = np.array([np.cos(th), np.sin(th), 0.0])
            p = [np.array([-sa * s, 0, 0]), np.array([(1 - sa) * s, 0, 0]), -sb * s * dr + z, (1 - sb) * s * dr + z]
            X = _place({int(k): q for k, q in zip(edges, p)}, s, rot=100 + 10 * kind + n)
            dbc = ()
            if rep == 3 and r in (0.5, 10.0):
                dbc = (edges[0],) if r == 0.5 else (edges[1], edges[3])
            c = _case(kind, [edges[q] for q in sub], X, s, KAPPAS[(n + rep) % 2], 1, True, edges, dbc,
                      name=f"mollified {'PP PE PT EE'.split()[kind]} c/eps_x {r:.10g} dHat/d {ratio:g}" + (f" {len(dbc)} Dirichlet node(s)" if dbc else ""))
            got = cross_norm([_pts(X)[k] for k in edges]) / eps_x_rest(edges)
            assert (got < 1) == (r < 1) and abs(got / mpf(r) - 1) < 1e-6, (c["name"], got)
            assert (float(np.sum(np.cross(X[edges[1]] - X[edges[0]], X[edges[3]] - X[edges[2]]) ** 2)) < ex) == (r < 1)  # the double value falls on the same side
            out.append(c)
            n += 1
    return out


def contact_cases():
    cases = []
    for kind in (K_PP, K_PE, K_PT, K_EE):
        cases += _active_cases(kind)
    for kind in (K_PP, K_PE, K_EE):
        cases += _para_cases(kind)
    for c in cases:
        d = _d_of(c, c["X"])
        assert 0 < d < DHAT, c["name"]
    return cases


EPS_V = 1.0e-4  # nominal sliding threshold of the friction cases; their stencils have sqrt(d) = 0.1 size, dHat/d = 2


def friction_cases():
    out = []
    h = float(np.sqrt(DHAT / 2.0))
    s = h / 0.1

    def add(kind, rel, rot, mult=1, v01=None, name=""):
        n = len(out)
        nodes = NODE_ORDERS[kind][n % 3]
        if v01 is None:
            X = _place(_active_geometry(kind, nodes, h, s), s, rot=rot)
        else:
            v = np.array(v01, dtype=np.float64)
            X = _place({nodes[0]: np.zeros(3), nodes[1]: (h / np.sqrt(v @ v)) * v}, s, rot=None)
        c = _case(kind, nodes, X, s, KAPPAS[n % 2], mult, name=f"friction {'PP PE PT EE'.split()[kind]} |u| {rel:g} eps {name}".strip())
        c["eps2"], c["coef"] = EPS_V ** 2, 0.37
        # slide the first node (the point; an end of edge a) in the tangent plane
        p = [X[k] for k in nodes]
        if kind == K_PP:
            nrm = p[1] - p[0]
        elif kind == K_PE:
            nrm = np.cross(p[2] - p[1], np.cross(p[0] - p[1], p[2] - p[1]))
        elif kind == K_PT:
            nrm = np.cross(p[2] - p[1], p[3] - p[1])
        else:
            nrm = np.cross(p[1] - p[0], p[3] - p[2])
        t = np.cross(nrm, np.array([0.3, -0.5, 0.8]))
        t /= np.linalg.norm(t)
        Xn = X.copy()
        Xn[nodes[0]] = X[nodes[0]] + (rel * EPS_V) * t
        Xn[nodes[1]] = X[nodes[1]] - 0.25 * (rel * EPS_V) * np.cross(nrm / np.linalg.norm(nrm), t)
        c["Xn"] = Xn
        out.append(c)
        return c
    for kind in (K_PP, K_PE, K_PT, K_EE):
        for rel in (0.0, 1e-3, 0.5, 1e3):
            add(kind, rel, rot=200 + len(out), mult=(1 + len(out) % 3) if kind in (K_PP, K_PE) else 1)
    for v01, nm in (((1, 1, 0), "(1,1,0)"), ((1, 0, 0), "x"), ((0, 1, 0), "y"), ((0, 0, 1), "z"), ((-1, -1, 0), "-(1,1,0)")):
        add(K_PP, 0.5, None, v01=v01, name="v01 along " + nm)
    add(K_PP, 2.0, 231, mult=2, name="mult 2")
    add(K_PE, 0.7, 232, mult=3, name="mult 3")
    # |u|^2 == eps2 exactly and one ulp either side: eps2 is chosen from the exact |u|^2 of the doubles
    for kind in (K_PP, K_PT):
        base = add(kind, 1.0, 240 + kind, name="|u|^2 == eps2")
        u2 = float(friction_reference(base, base["X"], base["Xn"])["u2"])
        base["eps2"] = u2
        for e2, nm in ((np.nextafter(u2, 0.0), "|u|^2 one ulp above eps2"), (np.nextafter(u2, 1.0), "|u|^2 one ulp below eps2")):
            c = dict(base)
            c["eps2"], c["name"] = float(e2), base["name"].replace("|u|^2 == eps2", nm)
            out.append(c)
    return out


def high_mult_cases(n=300):
    """n PT stencils that share local node 0 of tet 0: the point at the origin, the faces (nodes 1..3) of tets 1..n round it at varied gaps"""
    rng = np.random.default_rng(77)
    out = []
    for t in range(n):
        ratio = (1.01, 1.5, 2.0, 10.0, 100.0)[t % 5]
        h = float(np.sqrt(DHAT / ratio))
        s = h / (0.1, 0.03, 0.01)[t % 3]
        w = rng.dirichlet([2, 2, 2])
        geo = _active_geometry(K_PT, (0, 1, 2, 3), h, s, par=tuple(w))
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        X = np.array([geo[k] for k in range(4)]) @ Q.T
        X -= X[0]  # the shared point sits at the origin exactly
        out.append(_case(K_PT, (0, 1, 2, 3), X, s, 1.0e3, name=f"shared point, face of tet {t + 1}"))
    return out


# ---- the stored file -------------------------------------------------------------------------------------------------------------------------
def evaluate_contact(case, seed):
    r = contact_reference(case, case["X"])
    p = contact_reference(case, perturbed(case["X"], seed))
    return r, {k: np.abs(np.asarray(p[k]) - np.asarray(r[k])) for k in ("d", "gd", "E", "g", "H")}


def evaluate_friction(case, seed):
    r = friction_reference(case, case["X"], case["Xn"])
    p = friction_reference(case, perturbed(case["X"], seed), perturbed(case["Xn"], seed))
    r.pop("u2")
    return r, {k: np.abs(np.asarray(p[k]) - np.asarray(r[k])) for k in ("lam", "coord", "basis", "E", "g", "H")}


_IN = ("kind", "nodes", "X", "size", "kappa", "mult", "para", "edges", "dbc")


def _triu(H):
    return np.asarray(H)[np.triu_indices(12)]


def untriu(v):
    H = np.zeros((12, 12))
    H[np.triu_indices(12)] = v
    return H + np.triu(H, 1).T


def _eval(job):
    fn, case, seed = job
    return fn(case, seed)


def pack(cases, fric, high, map_fn=map):
    """struct of arrays for np.savez_compressed; Hessians as their upper triangles (they are symmetric by construction)"""
    out = {}
    for pre, cs, ev, extra in (("c_", cases, evaluate_contact, ()), ("f_", fric, evaluate_friction, ("Xn", "eps2", "coef")), ("h_", high, evaluate_contact, ())):
        res = list(map_fn(_eval, [(ev, c, reference_seed(i)) for i, c in enumerate(cs)]))
        for k in _IN + extra:
            out[pre + k] = np.array([c[k] for c in cs])
        out[pre + "name"] = np.array([c["name"] for c in cs])
        for k in res[0][0]:
            f = _triu if k == "H" else np.asarray
            out[pre + "ref_" + k] = np.array([f(r[0][k]) for r in res])
            if k in res[0][1]:
                out[pre + "sens_" + k] = np.array([f(r[1][k]) for r in res])
    return out


def load(path=GOLDEN, prefix="c_"):
    """the cases of one family ('c_' contact, 'f_' friction, 'h_' shared point) with their references: a list of dicts"""
    Z = np.load(path)
    keys = [k[len(prefix):] for k in Z.files if k.startswith(prefix)]
    n = len(Z[prefix + "kind"])
    out = []
    for i in range(n):
        c = {k: Z[prefix + k][i] for k in keys}
        c["kind"], c["mult"], c["para"], c["name"], c["index"] = int(c["kind"]), int(c["mult"]), bool(c["para"]), str(c["name"]), i
        for k in ("ref_H", "sens_H"):
            c[k] = untriu(c[k])
        out.append(c)
    return out


def reference_seed(i):
    return 5000 + i


# ---- reading per-tet blocks out of the upper CSR, the oracle put together per stencil -------------------------------------------------------------
def tet_blocks(ia, ja, a, n_tets):
    """(n_tets, 12, 12): the stored (upper) entries of every tet's own block, zero elsewhere; entries that couple two tets are left out"""
    ia, ja, a = np.asarray(ia), np.asarray(ja), np.asarray(a)
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    own = rows // 12 == ja // 12
    B = np.zeros((n_tets, 12, 12))
    B[rows[own] // 12, rows[own] % 12, ja[own] % 12] = a[own]
    return B


def _embed(nodes, g, H):
    G, B = np.zeros(12), np.zeros((12, 12))
    for a, k in enumerate(nodes):
        G[3 * k:3 * k + 3] = g[3 * a:3 * a + 3]
        for b, l in enumerate(nodes):
            B[3 * k:3 * k + 3, 3 * l:3 * l + 3] = H[3 * a:3 * a + 3, 3 * b:3 * b + 3]
    return G, B


def oracle_contact(orc, case):
    """the same quantities as contact_reference from the oracle's pieces (stencil_distance, barrier, cross_sqnorm, mollifier, make_pd), in double"""
    kind = case["kind"]
    nodes = [int(k) for k in case["nodes"][:NN[kind]]]
    X, kappa = case["X"], float(case["kappa"])
    Xs = np.zeros((4, 3))
    Xs[:len(nodes)] = X[nodes]
    d, gS, HS = orc.stencil_distance(kind, Xs)
    b, gb, Hb = orc.barrier(d, DHAT)
    gd, W = _embed(nodes, gS, HS)
    if case["para"]:
        edges = [int(k) for k in case["edges"]]
        c, cgE, QE = orc.cross_sqnorm(X[edges])
        cg, Q = _embed(edges, cgE, QE)
        ex = 1.0e-3 * ((REST[edges[1]] - REST[edges[0]]) ** 2).sum() * ((REST[edges[3]] - REST[edges[2]]) ** 2).sum()
        e, eg, eH = orc.mollifier(c, ex)
        E = kappa * e * b
        g = kappa * (b * eg * cg + e * gb * gd)
        B = kappa * (gb * eg * (np.outer(gd, cg) + np.outer(cg, gd)) + b * (eg * Q + eH * np.outer(cg, cg)) + e * Hb * np.outer(gd, gd) + e * gb * W)
        used = sorted(set(edges))
    else:
        km = kappa * case["mult"]
        E, g, B = km * b, km * gb * gd, km * (Hb * np.outer(gd, gd) + gb * W)
        used = sorted(set(nodes))
    idx = _coords(used)
    H = np.zeros((12, 12))
    H[np.ix_(idx, idx)] = orc.make_pd(B[np.ix_(idx, idx)])
    for k in case["dbc"]:
        if k >= 0:
            g[3 * k:3 * k + 3] = 0.0
            H[3 * k:3 * k + 3, :] = 0.0
            H[:, 3 * k:3 * k + 3] = 0.0
    return dict(d=d, gd=gd, E=E, g=g, H=H)


def oracle_friction(orc, case):
    """orc.Friction on a carrier mesh of one tet"""
    V, F, SF = carrier_mesh(1)
    m = orc.Mesh(V, F)
    m.set_surface(SF)
    m.set_V(case["X"])
    act = np.array([tuples_of(case, 0)[0]], dtype=np.int32)
    fr = orc.Friction()
    lag = fr.update(m, act, DHAT, float(case["kappa"]))
    m.set_V(case["Xn"])
    e2, cf = float(case["eps2"]), float(case["coef"])
    ia, ja = m.pattern()
    H = tet_blocks(ia, ja, fr.hessian(m, case["X"], len(ja), e2, cf, True), 1)[0]
    H = H + np.triu(H, 1).T
    return dict(lam=lag["lam"][0], coord=lag["coord"][0], basis=lag["basis"][0], E=fr.energy(m, case["X"], e2, cf), g=fr.gradient(m, case["X"], e2, cf), H=H)


def scale_of(case, k):
    """the largest magnitude of the stencil's own gradient / block; |E| for the energy; the quantity's own size for d, lam, coordinates and unit vectors"""
    ref = {"g": "ref_g", "H": "ref_H", "gd": "ref_gd"}.get(k, "ref_" + k)
    if k in ("coord", "basis"):
        return 1.0
    if k in ("g", "H") and "ref_" + k + "scale" in case:
        return float(case["ref_" + k + "scale"])
    return float(np.abs(case[ref]).max())


def ratio(case, k, got):
    """worst |got - ref| / (sens + u scale) over the entries of quantity k"""
    err, den = np.abs(np.asarray(got) - case["ref_" + k]), case["sens_" + k] + U * scale_of(case, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf)).max())  # a quantity that is exactly 0 (dropped Dirichlet rows) must come out exactly 0


def oracle_ratios(orc, path=GOLDEN):
    out = {}
    for fam, pre, fn, keys in (("contact", "c_", oracle_contact, ("d", "gd", "E", "g", "H")), ("shared point", "h_", oracle_contact, ("d", "gd", "E", "g", "H")),
                               ("friction", "f_", oracle_friction, ("lam", "coord", "basis", "E", "g", "H"))):
        worst = (0.0, "")
        for c in load(path, pre):
            got = fn(orc, c)
            for k in keys:
                r = ratio(c, k, got[k])
                if not r <= worst[0]:
                    worst = (r, f"{c['name']} [{c['index']}] {k}")
        out[fam] = worst
    return out
