"""A numpy model of the two-level preconditioner of the iterative solver (IPCGPU_PRECOND_TWO_LEVEL): the prolongation P of six rigid-body modes per
aggregate, the Galerkin matrix P^T A P, and CG preconditioned additively, z = D^-1 r + P (P^T A P)^-1 P^T r, with the stopping rule of pcg_numpy.cg.
The aggregates are an input: the tests hand in the library's own."""
import numpy as np

import pcg_numpy


def cross_matrix(d):
    """(n, 3, 3): S(d) with S(d) w = d x w"""
    S = np.zeros((len(d), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -d[:, 2], d[:, 1]
    S[:, 1, 0], S[:, 1, 2] = d[:, 2], -d[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -d[:, 1], d[:, 0]
    return S


def node_blocks(agg_of, X, fixed):
    """(P_i as (n, 3, 6), free-node count per aggregate): [I | S(x_i - c_I)] with c_I the centroid of the aggregate's free nodes; zero for a fixed node;
    no rotation columns in an aggregate with fewer than 4 free nodes"""
    agg_of, fixed = np.asarray(agg_of), np.asarray(fixed, dtype=bool)
    n_agg = int(agg_of.max()) + 1
    free = ~fixed
    cnt = np.bincount(agg_of[free], minlength=n_agg)
    cen = np.zeros((n_agg, 3))
    np.add.at(cen, agg_of[free], X[free])
    cen /= np.maximum(cnt, 1)[:, None]
    P = np.zeros((len(agg_of), 3, 6))
    P[:, :, :3] = np.eye(3)
    P[:, :, 3:] = cross_matrix(X - cen[agg_of])
    P[cnt[agg_of] < 4, :, 3:] = 0.0
    P[fixed] = 0.0
    return P, cnt


def full_blocks(ia, ja, a):
    """(i, j, B) over every 3x3 node block of the full symmetric matrix behind the upper CSR"""
    r, c, v = pcg_numpy.upper_csr_to_full(np.asarray(ia), np.asarray(ja), np.asarray(a))
    n = (len(ia) - 1) // 3
    key = (r // 3).astype(np.int64) * n + c // 3
    uniq, inv = np.unique(key, return_inverse=True)
    B = np.zeros((len(uniq), 3, 3))
    np.add.at(B, (inv, r % 3, c % 3), v)
    return uniq // n, uniq % n, B


def galerkin(ia, ja, a, agg_of, X, fixed):
    """dense P^T A P, (6 nAgg)^2, aggregate I at rows 6 I .. 6 I + 5 (translation, rotation); the rotation block of an aggregate without rotation columns
    and the translation block of one without a free node are identities"""
    P, cnt = node_blocks(agg_of, X, fixed)
    n_agg = len(cnt)
    i, j, B = full_blocks(ia, ja, a)
    M = np.einsum("nki,nkl,nlj->nij", P[i], B, P[j])
    Ac = np.zeros((n_agg, n_agg, 6, 6))
    np.add.at(Ac, (np.asarray(agg_of)[i], np.asarray(agg_of)[j]), M)
    Ac = Ac.transpose(0, 2, 1, 3).reshape(6 * n_agg, 6 * n_agg)
    for I in np.nonzero(cnt < 4)[0]:
        Ac[6 * I + 3:6 * I + 6, 6 * I + 3:6 * I + 6] = np.eye(3)
    for I in np.nonzero(cnt < 1)[0]:
        Ac[6 * I:6 * I + 3, 6 * I:6 * I + 3] = np.eye(3)
    return Ac


def upper_csr_values(cia, cja, Ac):
    """the values of the dense coarse matrix at the entries of a coarse upper CSR"""
    rows = np.repeat(np.arange(len(cia) - 1), np.diff(cia))
    return Ac[rows, cja]


def cg(ia, ja, a, b, rel_tol, max_iter, agg_of=None, X=None, fixed=None):
    """CG from x = 0 with z = D^-1 r + P Ac^-1 P^T r (agg_of None: block Jacobi alone, z = D^-1 r) until |r|_2 <= rel_tol |b|_2 (the recurrence
    residual).  Returns (x, iterations)."""
    r_, c_, v_ = pcg_numpy.upper_csr_to_full(np.asarray(ia), np.asarray(ja), np.asarray(a))
    n = len(b)

    def mul(x):
        return np.bincount(r_, weights=v_ * x[c_], minlength=n)

    ii, jj, B = full_blocks(ia, ja, a)
    Dinv = np.linalg.inv(B[ii == jj])
    if agg_of is not None:
        P, cnt = node_blocks(agg_of, X, fixed)
        agg_of = np.asarray(agg_of)
        n_agg = len(cnt)
        Ainv = np.linalg.inv(galerkin(ia, ja, a, agg_of, X, fixed))
        Ainv = 0.5 * (Ainv + Ainv.T)

    def prec(r):
        r3 = r.reshape(-1, 3)
        z = np.einsum("nij,nj->ni", Dinv, r3)
        if agg_of is not None:
            rc = np.zeros((n_agg, 6))
            np.add.at(rc, agg_of, np.einsum("nki,nk->ni", P, r3))
            xc = (Ainv @ rc.reshape(-1)).reshape(n_agg, 6)
            z = z + np.einsum("nki,ni->nk", P, xc[agg_of])
        return z.reshape(-1)

    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    tol2 = rel_tol ** 2 * (b @ b)
    for it in range(1, max_iter + 1):
        Ap = mul(p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if r @ r <= tol2:
            return x, it
        z = prec(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_iter
