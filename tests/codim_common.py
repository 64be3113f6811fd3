"""What the GPU tests of the codimensional energies (shells, their strain limit, rods) share: the five-tet block they put beside a cloth or a rod, the
context the three step files start from, and the comparison of the three test_gpu_*_mp.py files against their mpmath references.  A helper module
(like shell_mp.py), imported by name."""
import numpy as np

from shell_limit_mp import ratio

NO_T = np.zeros((0, 4), dtype=np.int32)


def five_tet_cube(size, lo):
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64) * size + lo
    T = np.array([[1, 3, 4, 6], [0, 1, 3, 4], [2, 3, 1, 6], [5, 4, 6, 1], [7, 6, 4, 3]], dtype=np.int32)
    for t in T:  # positive volumes
        if np.linalg.det(P[t[1:]] - P[t[0]]) < 0:
            t[[2, 3]] = t[[3, 2]]
    return P, T


def step_context(gpu_lib, V, set_body, solver=0, T=None, YM=1e7, density=1000.0, dt=0.01, gravity=True, held=None, x0=None):
    """A context up to opt_init: the mesh (T=None: no tetrahedron), set_body(c) -- the shell, its limit or the rod --, positions x0, backward Euler, and
    `held` as fixed Dirichlet nodes"""
    c = gpu_lib.Context(0, solver=solver)
    c.set_mesh(V, NO_T if T is None else T, YM=YM, PR=0.4, density=density)
    set_body(c)
    if x0 is not None:
        c.set_positions(x0)
    c.opt_init(dt, gravity)
    c.set_time_integration("BE")
    if held is not None and len(held):
        c.add_dirichlet(np.asarray(held, dtype=np.int32))
    return c


def compare(mp, cases, k, got_of, coef, proj, worst, bad, where):
    """got_of(i) against mp.expected(cases[i], k, coef, proj) (mp: shell_mp, rod_mp or shell_limit_mp), k in "E", "g", "H": the largest err / (sens + u scale)
    goes into worst[k], a case over mp.M into bad.  Where the tolerance is 0 (nothing active, and the lower triangle of a Hessian) exact zeros are
    expected; a reference energy of +inf must be met by +inf.  The stored shell and rod cases have neither a zero tolerance nor an infinite energy, so for
    them this asks what their own earlier helpers asked, plus the zeros of the lower triangle; an infinite reference would have failed there."""
    for i, cs in enumerate(cases):
        ref, tol = mp.expected(cs, k, coef, proj)
        got = got_of(i)
        if k == "E" and ref == np.inf:
            if not got == np.inf:
                bad.append(f"{cs['name']} E {where}: {got} instead of +inf")
            continue
        if k == "H":
            ref = np.triu(ref)  # the upper CSR: the lower triangle of `got` is zero like the reference's here
            tol = np.triu(tol)
        assert np.all(np.isfinite(got)), (cs["name"], k)
        r = float(np.max(ratio(got - ref, tol / mp.M)))
        worst[k] = max(worst.get(k, 0.0), r)
        if not r <= mp.M:
            bad.append(f"{cs['name']} {k} {where}: err / (sens + u scale) = {r:.3g}")
