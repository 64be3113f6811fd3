"""A plain numpy conjugate-gradient solver on the symmetric-upper CSR of LinSysSolver.hpp:46-150: the yardstick the GPU's
preconditioned CG is counted against (tests/test_gpu_pcg.py) -- no preconditioner, or the inverses of the 3x3 diagonal node blocks."""
import numpy as np


def upper_csr_to_full(ia, ja, a):
    """(rows, cols, vals) of the full symmetric matrix behind an upper CSR"""
    n = len(ia) - 1
    rows = np.repeat(np.arange(n), np.diff(ia))
    off = rows != ja
    return np.concatenate([rows, ja[off]]), np.concatenate([ja, rows[off]]), np.concatenate([a, a[off]])


def symv(ia, ja, a, x):
    r, c, v = upper_csr_to_full(ia, ja, a)
    y = np.zeros_like(x)
    np.add.at(y, r, v * x[c])
    return y


def block_jacobi_inverse(ia, ja, a):
    """(n/3, 3, 3) inverses of the diagonal node blocks; entries the pattern does not hold count as zero"""
    n = len(ia) - 1
    D = np.zeros((n // 3, 3, 3))
    for r in range(n):
        for k in range(ia[r], ia[r + 1]):
            c = ja[k]
            if c // 3 == r // 3:
                D[r // 3, r % 3, c % 3] = a[k]
                D[r // 3, c % 3, r % 3] = a[k]
    return np.linalg.inv(D)


def cg(ia, ja, a, b, rel_tol, max_iter, block_jacobi=False):
    """CG from x = 0 until |r|_2 <= rel_tol |b|_2 (the recurrence residual).  Returns (x, iterations)."""
    r_, c_, v_ = upper_csr_to_full(ia, ja, a)

    def mul(x):
        y = np.zeros_like(x)
        np.add.at(y, r_, v_ * x[c_])
        return y

    Dinv = block_jacobi_inverse(ia, ja, a) if block_jacobi else None

    def prec(r):
        return np.einsum("nij,nj->ni", Dinv, r.reshape(-1, 3)).reshape(-1) if block_jacobi else r.copy()

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
