"""mpmath restatement of the air-drag potential (ipc_amd/csrc/aero_kernels.h), its gradient and its Hessian; a project extension, so there is no oracle to
compare with -- this file is the reference, pinned by tests/test_aero_mp.py (mp.diff, mp.eigsy, the momentum identity, the named cases).

Per triangle, with the LAGGED record (unit normal n, area A, start centroid c^n -- the kernels' INPUT: eight float64 numbers, `rest_record` restates the
host plan's arithmetic to the bit), the surface's Cn, Ct and oneSided, the wind w, the air density rho and the step dt:
  c = (x0 + x1 + x2) / 3,  u = (c - c^n) / dt - w,  u_n = u . n,  u_t = u - u_n n,  s_n = u_n or max(0, u_n)
  D = dt (rho A / 6) (Cn |s_n|^3 + Ct |u_t|^3)
  dD/dx_k = (rho A / 6) (Cn |s_n| s_n n + Ct |u_t| u_t)   for each node k (a third of dD/dc)
  d2D/dx_k dx_l = K / 9,  K = (rho A / (2 dt)) (2 Cn |s_n| n n^T + Ct (|u_t| (I - n n^T) + u_t u_t^T / |u_t|)),  the tangential part 0 at |u_t| = 0
Every formula is written once over an arithmetic `ops` (MP: mpmath at mp.dps digits; NP: float64 in the kernels' order): the float64 instance is the
"NumPy restatement" whose recorded error sizes the tolerance.

Tolerance of a quantity q (energy, gradient, dense Hessian, per-triangle force) of one case:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53  (as chamber_mp.py).
  sens   |q_mp(x~) - q_mp(x)| entrywise with every CURRENT coordinate moved by one ulp: all upward in the first pattern (the centroid then moves by a whole
         ulp, the size of its own rounding), signs from a seed in the other SENS_SAMPLES - 1; the largest.  This is where the cancellation in c - c^n lives:
         an ulp of |x| divided by dt.
  scale  q with every term behind u replaced by its magnitude (|u_a| |n_a| summed for u_n, |u_a| + that |n_a| for u_t, products of magnitudes, |u_t u_t^T| /
         |u_t| <= |u_t|; sums over the triangles that share a node), the largest entry for the gradient, the Hessian and the force: one number per case
         and quantity.  u itself enters with its true size: the rounding of c is what sens moves.
  M      the worst err / (sens + u scale) of the float64 restatement against mpmath over the stored cases (tools/make_aero_mp_golden.py --measure prints
         it), times 8 for what the restatement does not do -- another summation order (atomics), FMA contraction, the hardware's division and square root
         sequences --, rounded up to a power of two.  test_aero_mp.py::test_numpy_restatement_meets_the_tolerance pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = 2.0 ** -53
# measured (tools/make_aero_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored cases
# E 0.963 (pure tangential flow), gradient 1.836, Hessian 1.828, force 1.837 (all three: Dirichlet nodes moved, dt = 1e-4)
NUMPY_WORST_RATIO = 1.837
M = 16.0  # 8 x 1.837 = 14.7 rounded up to a power of two
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aero_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("E", "g", "H", "F")
STILL, DENSITY = (0.0, 0.0, 0.0), 1.225


class MP:
    @staticmethod
    def num(v):
        return mpf(float(v)) if not isinstance(v, mpf) else v
    sqrt = staticmethod(mp.sqrt)
    zero = mpf(0)


class NP:
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)
    zero = 0.0


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def rest_record(x0, x1, x2):
    """the host plan's lagged record of one triangle (aero_plan.h) in float64 and in its order: n (3), A, c (3), 0"""
    x0, x1, x2 = ([float(v) for v in p] for p in (x0, x1, x2))
    e1, e2 = [x1[a] - x0[a] for a in range(3)], [x2[a] - x0[a] for a in range(3)]
    m = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    l = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    ok = l > 0.0 and math.isfinite(l)
    return np.array([m[a] / l if ok else 0.0 for a in range(3)] + [0.5 * l if ok else 0.0] + [((x0[a] + x1[a]) + x2[a]) / 3.0 for a in range(3)] + [0.0])


def rest_records(X, tri):
    return np.array([rest_record(X[t[0]], X[t[1]], X[t[2]]) for t in np.asarray(tri)]).reshape(-1, 8)


def record_mp(x0, x1, x2):
    """the same record in mpmath (for the device's refresh and the plan's sums against a bound): n, A, c"""
    p = [[mpf(float(v)) for v in q] for q in (x0, x1, x2)]
    e1, e2 = [p[1][a] - p[0][a] for a in range(3)], [p[2][a] - p[0][a] for a in range(3)]
    m = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    l = mp.sqrt(_dot(m, m))
    return [v / l for v in m], l / 2, [(p[0][a] + p[1][a] + p[2][a]) / 3 for a in range(3)]


def triangle(ops, x, lag, cn, ct, one, w, rho, dt, magnitudes=False):
    """one triangle: x its three node positions, lag its record, all ops numbers.  -> dict E, g (3: the entry of EACH node), K9 (3 x 3: each nodal block),
    u, un, sn, lt, and the flags nOn / tOn of the parts that are there at all.  magnitudes: E, g, K9 with every term behind u replaced by its magnitude"""
    n, A, c0 = lag[0:3], lag[3], lag[4:7]
    c = [((x[0][a] + x[1][a]) + x[2][a]) / 3 for a in range(3)]
    u = [(c[a] - c0[a]) / dt - w[a] for a in range(3)]
    un = _dot(u, n)
    sn = ops.zero if (one and not un > 0) else un
    ut = [u[a] - un * n[a] for a in range(3)]
    lt = ops.sqrt(_dot(ut, ut))
    a6 = rho * A / 6
    nOn, tOn = bool(a6 > 0 and cn > 0 and sn != 0), bool(a6 > 0 and ct > 0 and lt > 0)
    out = {"u": u, "un": un, "sn": sn, "lt": lt, "nOn": nOn, "tOn": tOn, "a6": a6}
    if magnitudes:
        nm = [abs(v) for v in n]
        unm = sum(abs(u[a]) * nm[a] for a in range(3)) if nOn else ops.zero
        utm = [abs(u[a]) + sum(abs(u[b]) * nm[b] for b in range(3)) * nm[a] for a in range(3)] if tOn else [ops.zero] * 3
        ltm = ops.sqrt(_dot(utm, utm))
        out["E"] = dt * a6 * (cn * unm ** 3 + ct * ltm ** 3)
        out["g"] = [a6 * (cn * unm * unm * nm[a] + ct * ltm * utm[a]) for a in range(3)]
        out["K9"] = [[a6 / (3 * dt) * (2 * cn * unm * nm[r] * nm[c_] + ct * ltm * ((1 if r == c_ else 0) + nm[r] * nm[c_] + 1)) for c_ in range(3)] for r in range(3)]
        return out
    s = abs(sn)
    out["E"] = dt * a6 * (cn * (s * s * s) + ct * (lt * lt * lt))
    gn = cn * s * sn if nOn else ops.zero
    gt = ct * lt if tOn else ops.zero
    out["g"] = [a6 * (gn * n[a] + gt * ut[a]) for a in range(3)]
    kn = 2 * cn * s if nOn else ops.zero
    kq = ct / lt if tOn else ops.zero
    f = a6 / (3 * dt)
    out["K9"] = [[f * (((kn - gt) * n[r] * n[c_] + kq * ut[r] * ut[c_]) + (gt if r == c_ else ops.zero)) for c_ in range(3)] for r in range(3)]
    return out


def env_of(case, env=None):
    """(w, rho, dt) of a case, or the ones given instead"""
    return (case["w"], case["rho"], case["dt"]) if env is None else env


def reference(ops, case, x=None, env=None, magnitudes=False):
    """dict of the case at positions x (default: its own) in the environment env = (w, rho, dt) (default: its own): E, g[3 n], dense H[3 n][3 n], per (the
    per-triangle D), F (m x 3: the force on every triangle), power (sum -f . u), area (the loaded area), on (m: the triangle writes something)"""
    x = case["x"] if x is None else x
    w, rho, dt = env_of(case, env)
    nv = len(x)
    xn = [[ops.num(v) for v in row] for row in x]
    wn, rhon, dtn = [ops.num(v) for v in w], ops.num(rho), ops.num(dt)
    cn, ct, one = ops.num(case["cn"]), ops.num(case["ct"]), bool(case["one"])
    E, power, area = ops.zero, ops.zero, ops.zero
    g = [ops.zero] * (3 * nv)
    H = [[ops.zero] * (3 * nv) for _ in range(3 * nv)]
    per, F, on = [], [], []
    for t, lag in zip(case["tri"], case["lag"]):
        ids = [int(v) for v in t]
        r = triangle(ops, [xn[v] for v in ids], [ops.num(v) for v in lag], cn, ct, one, wn, rhon, dtn, magnitudes)
        E = E + r["E"]
        per.append(r["E"])
        F.append([3 * v if magnitudes else -3 * v for v in r["g"]])
        on.append(r["nOn"] or r["tOn"])
        if not on[-1]:
            continue
        power = power + 3 * (sum(r["g"][a] * abs(r["u"][a]) for a in range(3)) if magnitudes else _dot(r["g"], r["u"]))
        area = area + ops.num(lag[3])
        for k in ids:
            for a in range(3):
                g[3 * k + a] = g[3 * k + a] + r["g"][a]
                for l in ids:
                    for b in range(3):
                        H[3 * k + a][3 * l + b] = H[3 * k + a][3 * l + b] + r["K9"][a][b]
    return {"E": E, "g": g, "H": H, "per": per, "F": F, "power": power, "area": area, "on": on}


def _f(v):
    return np.array(v, dtype=object).astype(np.float64) if not isinstance(v, (float, mpf)) else float(v)


def perturbed(A, sample):
    """every entry moved by one ulp: upward for sample 0, by seeded signs otherwise"""
    A = np.asarray(A, dtype=np.float64)
    s = np.ones(A.shape, dtype=np.int64) if sample == 0 else np.random.default_rng(sample).integers(0, 2, size=A.shape) * 2 - 1
    return np.where(s > 0, np.nextafter(A, np.inf), np.nextafter(A, -np.inf))


def evaluate(case, env=None):
    """reference, sens and scale of E, g, H, F of one case in an environment (default: its own), the per-triangle energies, the totals of aero_state
    (float64; the differences are taken in mpmath)"""
    r = reference(MP, case, env=env)
    keys = {"E": "E", "g": "g", "H": "H", "F": "F", "power": "power"}
    sens = {k: np.zeros(np.shape(_f(r[v]))) for k, v in keys.items()}
    for s in range(SENS_SAMPLES):
        q = reference(MP, case, perturbed(case["x"], s), env=env)
        for k, v in keys.items():
            d = abs(q[v] - r[v]) if k in ("E", "power") else np.abs(np.array(q[v], dtype=object) - np.array(r[v], dtype=object))
            sens[k] = np.maximum(sens[k], _f(d))
    m = reference(MP, case, env=env, magnitudes=True)
    out = {"E": float(r["E"]), "g": _f(r["g"]), "H": _f(r["H"]), "F": _f(r["F"]).reshape(-1, 3), "perE": _f(r["per"]), "power": float(r["power"]),
           "area": float(r["area"]), "on": np.array(r["on"], dtype=bool)}
    for k in keys:
        out["sens_" + k] = float(sens[k]) if k in ("E", "power") else sens[k].reshape(np.shape(out[k]))
    out["scale_E"] = float(m["E"])
    out["scale_g"] = float(max(m["g"]))
    out["scale_H"] = float(max(max(row) for row in m["H"]))
    out["scale_F"] = float(max(max(row) for row in m["F"]))
    out["scale_power"] = float(m["power"])
    return out


def numpy_restatement(case):
    r = reference(NP, case)
    return {"E": float(r["E"]), "g": np.array(r["g"], dtype=np.float64), "H": np.array(r["H"], dtype=np.float64), "F": np.array(r["F"], dtype=np.float64).reshape(-1, 3)}


def ratio(err, tol_over_M):
    """err / (sens + u scale) entrywise; where that tolerance is 0 (nothing is written: exact zeros are expected) 0 for no error and infinity for any"""
    err, t = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol_over_M, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


def expected(case, k, coef=1.0, projectDBC=True):
    """(reference, tolerance) of quantity k at `coef` from an evaluated case (a stored one, or dict(case, **evaluate(case, env))); gradient entries, rows
    and columns of projected Dirichlet nodes dropped (type 1 always, 2 with projectDBC); where no triangle of the case writes anything the tolerance of
    gradient and Hessian is 0: exact zeros"""
    ref, tol = coef * np.array(case[k], dtype=np.float64), np.array(tolerance(case, k, coef), dtype=np.float64)
    if k in ("E", "power"):
        return float(ref), float(tol)
    if k == "F":
        return ref, tol
    if not np.any(case["on"]):
        tol = np.zeros_like(ref)
    proj = np.repeat((case["dbc"] == 1) | ((case["dbc"] == 2) & bool(projectDBC)), 3)
    ref[proj] = 0.0
    if k == "H":
        ref[proj, :] = 0.0
        ref[:, proj] = 0.0
    return ref, tol


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
WIND = (3.0, -1.0, 2.0)


def _case(name, X, tri, x=None, cn=1.28, ct=0.0, one=False, w=STILL, rho=DENSITY, dt=0.01, dbc=None):
    """X: the rest positions (the lagged records are taken there), x: the current ones (default: at rest)"""
    X = np.asarray(X, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    return {"name": name, "X": X, "x": X.copy() if x is None else np.asarray(x, dtype=np.float64), "tri": tri, "cn": np.float64(cn), "ct": np.float64(ct),
            "one": np.int32(bool(one)), "w": np.array(w, dtype=np.float64), "rho": np.float64(rho), "dt": np.float64(dt), "lag": rest_records(X, tri),
            "dbc": np.zeros(len(X), dtype=np.int32) if dbc is None else np.asarray(dbc, dtype=np.int32)}


def cases():
    rng = np.random.default_rng(47)
    T1 = [[0, 1, 2]]
    tri3 = lambda lo, size=0.25: np.array([[0, 0, 0], [1, 0.1, 0.05], [0.2, 0.9, -0.1]]) * size + np.asarray(lo, dtype=np.float64) + 0.02 * size * (rng.random((3, 3)) - 0.5)
    normal = lambda X: rest_record(*X)[:3]
    dt = 0.01
    out = [_case("u = 0", tri3([0.1, 0.2, 0.3]), T1, ct=0.3)]
    X = tri3([0.5, 0.1, 0.2])
    out.append(_case("pure normal flow", X, T1, X + dt * 2.5 * normal(X), ct=0.3))
    X = tri3([0.9, 0.2, 0.1])
    e = (X[1] - X[0]) / np.linalg.norm(X[1] - X[0])
    out.append(_case("pure tangential flow", X, T1, X + dt * 1.7 * e, ct=0.3))
    X = tri3([1.3, 0.1, 0.3])
    e = (X[2] - X[0]) / np.linalg.norm(X[2] - X[0])
    out.append(_case("oblique flow", X, T1, X + dt * np.array([0.4, -0.2, 0.3]), ct=0.2, one=True, w=0.8 * e - 2.0 * normal(X), rho=1.0))  # windward: u_n about 2
    X = tri3([1.7, 0.2, 0.2])
    out.append(_case("one-sided, leeward", X, T1, X - dt * 1.9 * normal(X) + dt * 0.05 * rng.standard_normal((3, 3)), ct=0.0, one=True))
    flat = np.array([[2.0, 0.125, 0.5], [2.25, 0.125, 0.5], [2.0625, 0.375, 0.5]])  # in the plane z = 1/2: n = (0, 0, 1) exactly
    out.append(_case("one-sided, exactly at u_n = 0", flat, T1, flat + np.array([0.0078125, 0.00390625, 0.0]), ct=0.4, one=True))
    b = 0.3
    sliver = np.array([[2.5, 0.1, 0.2], [2.5 + b, 0.1, 0.2], [2.5 + 0.4 * b, 0.1 + 2e-6 * b, 0.2]]) + 1e-9 * rng.random((3, 3))  # area / b^2 = 1e-6
    out.append(_case("sliver", sliver, T1, sliver + dt * np.array([0.3, 0.2, 1.1]), ct=0.3))
    X = tri3([0.1, 0.2, 0.3]) + [250.0, -250.0, 250.0]
    out.append(_case("far from the origin", X, T1, X + dt * np.array([0.5, 0.8, -0.6]), ct=0.25, w=WIND))
    quad = lambda lo: np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, -0.1]]) * 0.2 + np.asarray(lo, dtype=np.float64) + 0.004 * (rng.random((4, 3)) - 0.5)
    T2 = [[0, 1, 2], [0, 2, 3]]
    X = quad([3.0, 0.1, 0.2])
    out.append(_case("Dirichlet nodes", X, T2, X + dt * (np.array([0.6, 0.1, 0.9]) + 0.2 * rng.standard_normal((4, 3))), ct=0.3, w=WIND, dbc=[1, 0, 2, 0]))
    X = quad([3.5, 0.1, 0.2])
    moved = X.copy()
    moved[0] += 1e-4 * np.array([0.9, -0.3, 1.2])
    moved[2] += 1e-4 * np.array([-0.4, 0.5, 0.8])
    out.append(_case("Dirichlet nodes moved, dt = 1e-4", X, T2, moved, ct=0.3, w=(0.3, 0.1, -0.2), dt=1e-4, dbc=[1, 0, 2, 0]))
    return out


INPUTS = ("X", "x", "tri", "cn", "ct", "one", "w", "rho", "dt", "lag", "dbc")
SCALARS = ("E", "sens_E", "scale_E", "scale_g", "scale_H", "scale_F", "power", "sens_power", "scale_power", "area", "cn", "ct", "rho", "dt")


def pack():
    cs = cases()
    out = {"names": np.array([c["name"] for c in cs])}
    for i, c in enumerate(cs):
        r = evaluate(c)
        for k in INPUTS:
            out[f"c{i}_{k}"] = c[k]
        for k, v in r.items():
            out[f"c{i}_{k}"] = np.asarray(v)
    return out


def load(path=GOLDEN):
    z = np.load(path)
    res = []
    for i, name in enumerate(z["names"]):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        c["name"] = str(name)
        for k in SCALARS:
            c[k] = float(c[k])
        c["one"] = int(c["one"])
        res.append(c)
    return res


def environments(cs):
    """the distinct (w, rho, dt) of the cases, in order of appearance"""
    out = []
    for c in cs:
        e = (tuple(float(v) for v in c["w"]), float(c["rho"]), float(c["dt"]))
        if e not in out:
            out.append(e)
    return out


def in_environment(case, env):
    """the case evaluated in env: its stored results where env is its own, else evaluated now (a few dozen mpmath operations)"""
    own = (tuple(float(v) for v in case["w"]), float(case["rho"]), float(case["dt"]))
    return case if env == own and "sens_E" in case else dict(case, **evaluate(case, env))
