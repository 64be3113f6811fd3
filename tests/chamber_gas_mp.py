"""mpmath restatement of the gas law of the pressure chambers (ipc_amd/csrc/chamber_kernels.h), on top of chamber_mp.py; a project extension, so this file
is the reference, pinned by tests/test_chamber_gas_mp.py (mp.diff of W and of the gradient, the limit gamma -> 1, rigid motions, dW/dV = -gauge).

  V = 1/6 sum_t y0 . (y1 x y2), y = x - r;  P0 = p_amb + p_c;  P = P0 (V0 / V)^gamma;  gauge = P - p_amb;  beta = gamma P / V;
  W = -P0 V0 ln(V / V0) + p_amb (V - V0)  (gamma == 1),  W = P0 V0 / (gamma - 1) ((V0 / V)^(gamma - 1) - 1) + p_amb (V - V0)  (gamma > 1);
  u = gradV;  dW/dx = -gauge u;  d2W/dx2 = -gauge d2V/dx2 + beta u u^T.
p_c, p_amb, gamma, V0, r and x are the kernels' INPUTS: they enter mpmath as the float64 numbers they are.

Tolerance of a quantity q of one state, as chamber_mp.py:  tol(q) = M (sens(q) + u scale(q)),  u = 2^-53.
  sens   |q_mp(x~) - q_mp(x)| with every coordinate moved by ONE ulp, signs by a seed, the largest of SENS_SAMPLES patterns (entrywise for the vectors)
  scale  the magnitudes of the terms of the formula.  With Vmag = 1/6 sum_t (|y0| . (|y1| x| |y2|)) (every product taken positive), the absolute error of V
         is a multiple of u Vmag, its relative error dV = Vmag / V (in units of u), and
           V      Vmag
           gauge  P (1 + gamma dV) + p_amb + |p_c|          (P inherits gamma times the relative error of V; then one subtraction)
           beta   beta (1 + (gamma + 1) dV)
           W      |gauge| Vmag + P0 V0 |h| + p_amb (V + V0),   h = ln(V0 / V) or ((V0 / V)^(gamma - 1) - 1) / (gamma - 1)
           u      umag, the largest entry of 1/6 sum over the node's triangles of |y_a| x| |y_b|
           g      scale(gauge) max|u| + |gauge| umag
  M      the next power of two above the worst err / (sens + u scale) of the float64 NumPy restatement below (the kernel's formulas: log1p or log, and expm1)
         against mpmath over the stored states.  tools/make_chamber_gas_mp_golden.py --measure prints it; test_chamber_gas_mp.py pins it.
"""
import math
import os

import numpy as np
from mpmath import mp, mpf

import chamber_mp as cm

U = cm.U
# measured (tools/make_chamber_gas_mp_golden.py --measure): worst err / (sens + u scale) of the float64 restatement over the stored states, per quantity
# V 0.416, gauge 0.477, beta 0.498, W 0.688, u 0.329, g 0.326
NUMPY_WORST_RATIO = 0.688
M = 1.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chamber_gas_mp_cases.npz")
SENS_SAMPLES = 4
QUANT = ("V", "gauge", "beta", "W", "u", "g")


def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    X = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    T = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6],
                  [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int32)
    return X / np.linalg.norm(X[0]), T


def icosphere(levels):
    X, T = icosahedron()
    X = [tuple(v) for v in X]
    for _ in range(levels):
        mid, T2 = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v = np.array(X[a]) + np.array(X[b])
                X.append(tuple(v / np.linalg.norm(v)))
                mid[k] = len(X) - 1
            return mid[k]
        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            T2 += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        T = T2
    return np.array(X, dtype=np.float64), np.array(T, dtype=np.int32)


def _tri_terms(x, r, tri, mag):
    """per triangle the triple product and the three node gradients of it (lists of numbers of the arithmetic of x)"""
    out = []
    for t in tri:
        y = [[(abs(x[int(v)][a] - r[a]) if mag else x[int(v)][a] - r[a]) for a in range(3)] for v in t]
        c12, c20, c01 = cm._cross(y[1], y[2], mag), cm._cross(y[2], y[0], mag), cm._cross(y[0], y[1], mag)
        out.append((cm._dot(y[0], c12), (c12, c20, c01)))
    return out


def quantities(ops, ch, x, mag=False):
    """V, gauge, beta, W, u[3 n], g[3 n] of one chamber ch = {tri, r, p, ambient, gamma, V0} at the positions x (n x 3); ops: cm.MP or cm.NP.
    mag: the scales of the module text in place of the values."""
    n = len(x)
    xn = [[ops.num(v) for v in row] for row in x]
    r = [ops.num(v) for v in ch["r"]]
    pc, pa, gm, V0 = (ops.num(ch[k]) for k in ("p", "ambient", "gamma", "V0"))
    P0 = pa + pc
    terms = _tri_terms(xn, r, ch["tri"], False)
    V = sum((e for e, _ in terms), ops.zero) / 6
    u = [ops.zero] * (3 * n)
    for t, (_, gs) in zip(ch["tri"], terms if not mag else _tri_terms(xn, r, ch["tri"], True)):
        for k in range(3):
            for a in range(3):
                u[3 * int(t[k]) + a] = u[3 * int(t[k]) + a] + gs[k][a] / 6
    if ops is cm.MP:
        ratio = V0 / V
        P = P0 * ratio ** gm
        gauge = P - pa
        h = mp.log(ratio) if gm == 1 else (ratio ** (gm - 1) - 1) / (gm - 1)
    else:  # the kernel's formulas
        # (near V0 from the exact difference: no absolute error u where V is close to V0; far from it the quotient is better conditioned)
        lr = -math.log1p((V - V0) / V0) if abs(V - V0) <= 0.5 * V0 else math.log(V0 / V)
        grow = math.expm1(gm * lr)
        gauge = pc + P0 * grow
        P = P0 + P0 * grow
        h = lr if gm == 1.0 else math.expm1((gm - 1.0) * lr) / (gm - 1.0)
    beta = gm * P / V
    W = P0 * V0 * h + pa * (V - V0)
    if not mag:
        return V, gauge, beta, W, u, [-gauge * v for v in u]
    Vmag = sum((e for e, _ in _tri_terms(xn, r, ch["tri"], True)), ops.zero) / 6
    dV = Vmag / V
    umag = max(u)
    sg = P * (1 + gm * dV) + pa + abs(pc)
    umax = max(abs(v) for v in quantities(ops, ch, x)[4])
    return Vmag, sg, beta * (1 + (gm + 1) * dV), abs(gauge) * Vmag + P0 * V0 * abs(h) + pa * (V + V0), umag, sg * umax + abs(gauge) * umag


def evaluate(ch, x):
    """reference, sens and scale of the six quantities of one chamber at x (float64; the differences are taken in mpmath)"""
    ref = quantities(cm.MP, ch, x)
    sens = [0.0, 0.0, 0.0, 0.0, np.zeros(3 * len(x)), np.zeros(3 * len(x))]
    for s in range(SENS_SAMPLES):
        q = quantities(cm.MP, ch, cm.perturbed(x, s + 1))
        for i in range(4):
            sens[i] = max(sens[i], float(abs(q[i] - ref[i])))
        for i in (4, 5):
            sens[i] = np.maximum(sens[i], cm._f([abs(a - b) for a, b in zip(q[i], ref[i])]))
    scale = quantities(cm.MP, ch, x, mag=True)
    out = {}
    for i, k in enumerate(QUANT):
        out[k] = cm._f(ref[i]) if i >= 4 else float(ref[i])
        out["sens_" + k] = sens[i]
        out["scale_" + k] = float(scale[i])
    return out


def tolerance(ref, k, coef=1.0):
    return M * abs(coef) * (np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])


def numpy_restatement(ch, x):
    q = quantities(cm.NP, ch, x)
    return {k: (np.array(q[i], dtype=np.float64) if i >= 4 else float(q[i])) for i, k in enumerate(QUANT)}


# ---- the scene of the GPU test: three chambers in one context -------------------------------------------------------------------------------
def scene():
    """rest positions X (n x 3), the chambers [{tri (global ids), p, gas, ambient, gamma}] -- a 12-triangle cube (constant), a 320-triangle icosphere (gas,
    gamma 1.4: two slices, the second a ragged tail of 64) and a 20-triangle icosahedron (gas, gamma 1) -- and the node range of each.  The ranges of the gas
    chambers start at triangle 12 and 332: off every wave and slice boundary."""
    rng = np.random.default_rng(77)
    cube = cm.CUBE_X * 0.2 + [0.1, 0.1, 0.1] + 0.004 * (rng.random((8, 3)) - 0.5)
    sx, st = icosphere(2)
    sx = sx * 0.15 * (1 + 0.02 * (rng.random((len(sx), 1)) - 0.5)) + [0.6, 0.2, 0.3]
    ix, it = icosahedron()
    ix = ix * 0.1 * (1 + 0.05 * (rng.random((len(ix), 1)) - 0.5)) + [1.0, 0.3, 0.2]
    X = np.vstack([cube, sx, ix])
    off = [0, 8, 8 + len(sx), 8 + len(sx) + len(ix)]
    ch = [dict(tri=cm.CUBE_TRI + off[0], p=1500.0, gas=False, ambient=0.0, gamma=1.0),
          dict(tri=st + off[1], p=2.0e3, gas=True, ambient=1.0e5, gamma=1.4),
          dict(tri=it + off[2], p=-300.0, gas=True, ambient=2.5e4, gamma=1.0)]
    for c in ch:
        c["tri"] = np.asarray(c["tri"], dtype=np.int32)
        c["r"] = cm.ref_point(X, c["tri"])
        c["V0"] = cm.rest_volume(X, c["tri"], c["r"])
        assert c["V0"] > 0
    return X, ch, off


def states(X, ch, off):
    """name -> positions: rest, a random perturbation, every gas chamber compressed uniformly to V = 0.3 V0 about its centroid, and a translation by 1e3"""
    rng = np.random.default_rng(78)
    squeezed = X.copy()
    for c, a, b in zip(ch, off[:-1], off[1:]):
        if c["gas"]:
            m = X[a:b].mean(axis=0)
            squeezed[a:b] = m + (X[a:b] - m) * 0.3 ** (1.0 / 3.0)
    return {"rest": X.copy(), "perturbed": X + 0.01 * (rng.random(X.shape) - 0.5), "compressed": squeezed, "translated": X + np.array([1e3, -1e3, 1e3])}


def pack():
    X, ch, off = scene()
    out = {"X": X, "off": np.array(off), "states": np.array(list(states(X, ch, off)))}
    for s, (name, x) in enumerate(states(X, ch, off).items()):
        out[f"s{s}_x"] = x
        for i, c in enumerate(ch):
            if not c["gas"]:
                continue
            for k, v in evaluate(c, x).items():
                out[f"s{s}_c{i}_{k}"] = np.asarray(v)
    return out


def load(path=GOLDEN):
    """[(state name, x, {chamber index: reference dict})] as stored"""
    z = np.load(path)
    res = []
    for s, name in enumerate(z["states"]):
        refs = {}
        for k in z.files:
            if k.startswith(f"s{s}_c"):
                i, q = k[len(f"s{s}_c"):].split("_", 1)
                refs.setdefault(int(i), {})[q] = z[k] if z[k].ndim else float(z[k])
        res.append((str(name), z[f"s{s}_x"], refs))
    return res


def ratio(err, ref, k):
    return float(np.max(cm.ratio(err, np.asarray(ref["sens_" + k]) + U * ref["scale_" + k])))
