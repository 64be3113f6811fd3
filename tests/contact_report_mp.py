"""The contact report (`ipcgpu_contact_report`) restated in mpmath: a helper module like stencil_mp.py, used by test_contact_report_mp.py and
test_gpu_contact_report.py.  Nothing here shares code or arithmetic with ipc_amd/: the distances, barrier, mollifier and the friction lag are
stencil_mp's, forces are minus central differences of the ENERGIES (stencil_mp._derivs, step 1e-20 x the stencil's size, mp.dps = 100), the side sums,
torques and row sums are exact mp sums, rounded once at the end.

A tuple is a dict: `src` ("active", "moll", "hs", "fric"), `kind`, `nodes` (global node ids in stencil order), `mult`, `idx` (what argmin reports);
for "moll" also `edges` (the four edge nodes eI0 eI1 eJ0 eJ1) and `eps_x`; for "hs" `h` (the half-space id), `n` (unit normal) and `D`; for "fric" `lag`
(the positions the set was lagged at), `lag_kappa`, `lag_dhat`, `eps2`, `coef`.  Tuples are listed in the report's record order: active, mollified, half-spaces by id, friction.

Tolerance of a double output of a row (the rule of test_gpu_stencils_mp.py, summed): sum over the row's tuples of stencil_mp.tol(sens_i, scale_i) -- sens_i the
change of the tuple's own term when every coordinate moves by +-4 ulp, scale_i the largest magnitude among the tuple's force (torque) components -- plus
n u sum_i |t_i| for the n-term summation."""
import numpy as np
from mpmath import mp, mpf

import stencil_mp as smp

mp.dps = 100
NN = smp.NN


def _v(x):
    return [mpf(float(c)) for c in x]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _minus_grad(E, P, size):
    """-dE/dx per node (list of 3-vectors) of E(list of node positions) at the mp positions P, by central differences"""
    y = [c for p in P for c in p]
    n = len(P)
    _, g, _ = smp._derivs(lambda z: E([z[3 * k:3 * k + 3] for k in range(n)]), y + [mpf(0)] * (12 - 3 * n), list(range(3 * n)),
                          mpf("1e-20") * mpf(float(size)), hessian=False)
    return [[-g[3 * k + c] for c in range(3)] for k in range(n)]


def tuple_terms(t, X, dHat, kappa):
    """(d, [(node, side, position, force)]) of tuple t at the positions X (nV x 3 doubles); side 0 = primitive 1.  d is None for a friction tuple."""
    kind, nodes = int(t["kind"]), [int(k) for k in t["nodes"]]
    dH, kap = mpf(float(dHat)), mpf(float(kappa))
    n1 = 2 if kind == smp.K_EE else 1
    if t["src"] == "active":
        P = [_v(X[k]) for k in nodes]
        size = max(1e-300, float(np.abs(X[nodes] - X[nodes[0]]).max()))
        d = smp.dist2(kind, P)
        f = _minus_grad(lambda Q: kap * int(t["mult"]) * smp.barrier(smp.dist2(kind, Q), dH), P, size)
        return d, [(k, 0 if i < n1 else 1, P[i], f[i]) for i, k in enumerate(nodes)]
    if t["src"] == "moll":
        edges = [int(k) for k in t["edges"]]
        where = [edges.index(k) for k in nodes]
        P = [_v(X[k]) for k in edges]
        size = max(1e-300, float(np.abs(X[edges] - X[edges[0]]).max()))
        d = smp.dist2(kind, [P[w] for w in where])
        ex = mpf(float(t["eps_x"]))
        f = _minus_grad(lambda Q: kap * smp.mollifier(smp.cross_norm(Q), ex) * smp.barrier(smp.dist2(kind, [Q[w] for w in where]), dH), P, size)
        return d, [(k, 0 if i < 2 else 1, P[i], f[i]) for i, k in enumerate(edges)]
    if t["src"] == "hs":
        v = nodes[0]
        P = [_v(X[v])]
        nrm, D = _v(t["n"]), mpf(float(t["D"]))
        dist = lambda Q: nrm[0] * Q[0][0] + nrm[1] * Q[0][1] + nrm[2] * Q[0][2] + D
        d = dist(P) ** 2
        f = _minus_grad(lambda Q: kap * smp.barrier(dist(Q) ** 2, dH), P, max(1e-300, abs(float(dist(P)))))
        return d, [(v, 0, P[0], f[0])]
    # friction: the lag (multiplier, weights, basis) at t["lag"] with stencil_mp's rule, the force at X over the step from Xt = t["lag"]
    n = NN[kind]
    case = dict(kind=kind, nodes=np.arange(4), kappa=float(t["lag_kappa"]), mult=int(t["mult"]))
    Xl = np.zeros((4, 3))
    Xl[:n] = t["lag"][nodes]
    _lam, _co, wt, t0, t1 = smp.friction_lag(case, Xl)  # (its multiplier is for stencil_mp.DHAT: restated here for the lag's own dHat)
    dl = smp.dist2(kind, [_v(x) for x in Xl[:n]])
    lam = -2 * mpf(float(t["lag_kappa"])) * mp.sqrt(dl) * smp.barrier_d1(dl, mpf(float(t["lag_dhat"]))) * int(t["mult"]) * mpf(float(t.get("scale", 1.0)))
    eps, coef = mp.sqrt(mpf(float(t["eps2"]))), mpf(float(t["coef"]))
    Pt = [_v(t["lag"][k]) for k in nodes]
    P = [_v(X[k]) for k in nodes]

    def E(Q):
        r = [sum(wt[a] * (Q[a][c] - Pt[a][c]) for a in range(n)) for c in range(3)]
        u0, u1 = smp._dot(t0, r), smp._dot(t1, r)
        return coef * lam * smp.f0(mp.sqrt(u0 * u0 + u1 * u1), eps)
    size = max(1e-300, float(np.abs(t["lag"][nodes] - t["lag"][nodes[0]]).max()))
    f = _minus_grad(E, P, size)
    return None, [(k, 0 if i < n1 else 1, P[i], f[i]) for i, k in enumerate(nodes)]


def record(t, X, Xt, comp, dHat, kappa):
    """None (no contribution) or dict(key, src, kind, idx, d, F[2][3], T[2][3], W) in mp with side A first"""
    d, terms = tuple_terms(t, X, dHat, kappa)
    if d is not None and not d < mpf(float(dHat)):
        return None
    F = [[mpf(0)] * 3 for _ in range(2)]
    T = [[mpf(0)] * 3 for _ in range(2)]
    W = mpf(0)
    for k, side, x, f in terms:
        tq = _cross(x, f)
        for c in range(3):
            F[side][c] += f[c]
            T[side][c] += tq[c]
        if t["src"] == "fric":
            W += sum(f[c] * (x[c] - mpf(float(Xt[k][c]))) for c in range(3))
    if t["src"] == "hs":
        key = (int(comp[terms[0][0]]), -1 - int(t["h"]))
        swap = False
    else:
        first = {0: None, 1: None}
        for k, side, _x, _f in terms:
            if first[side] is None:
                first[side] = k
        c1, c2 = int(comp[first[0]]), int(comp[first[1]])
        swap = c1 > c2
        key = (min(c1, c2), max(c1, c2))
    if swap:
        F, T = F[::-1], T[::-1]
    return dict(key=key, src=t["src"], kind=int(t["kind"]), idx=int(t["idx"]), d=d, F=F, T=T, W=W)


def row_order(keys):
    """ascending a; a's component rows first, then its half-space rows ascending in h"""
    return sorted(keys, key=lambda ab: (ab[0], 0, ab[1]) if ab[1] >= 0 else (ab[0], 1, -1 - ab[1]))


def row_table(records):
    """records (None entries skipped) in record order -> list of rows in row order: dict(a, b, counts[5], argmin, minD2, vals[19] (FA FB TA TB RA RB W, mp), members)"""
    rows = {}
    for i, r in enumerate(records):
        if r is None:
            continue
        row = rows.setdefault(r["key"], dict(a=r["key"][0], b=r["key"][1], counts=[0] * 5, argmin=-1, minD2=mp.inf, vals=[mpf(0)] * 19, members=[]))
        row["members"].append(i)
        if r["src"] == "fric":
            v = r["F"][0] + r["F"][1] + [r["W"]]
            for q in range(7):
                row["vals"][12 + q] += v[q]
            continue
        row["counts"][4 if r["src"] == "moll" else (0 if r["src"] == "hs" else r["kind"])] += 1
        if r["d"] < row["minD2"]:
            row["minD2"], row["argmin"] = r["d"], r["idx"]
        v = r["F"][0] + r["F"][1] + r["T"][0] + r["T"][1]
        for q in range(12):
            row["vals"][q] += v[q]
    return [rows[k] for k in row_order(rows)]


def record_values(r):
    """the 19 double columns a single record adds to its row (mp)"""
    if r["src"] == "fric":
        return [mpf(0)] * 12 + r["F"][0] + r["F"][1] + [r["W"]]
    return r["F"][0] + r["F"][1] + r["T"][0] + r["T"][1] + [mpf(0)] * 7


def column_scales(r):
    """per column the largest magnitude of the record's group (force / torque / friction force / work): the `scale` of stencil_mp.tol"""
    v = [abs(float(x)) for x in record_values(r)]
    s = [max(v[0:6])] * 6 + [max(v[6:12])] * 6 + [max(v[12:18])] * 6 + [v[18]]
    return np.array(s)
