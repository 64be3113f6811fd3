"""Pins tests/round_collider_mp.py (the reference of the round-collider kernels) on the CPU: the closed forms against mp.diff of the energy, the
two-coefficient clamp against the eigen-projection of the exact Hessian in every region, the step bound against mp.findroot, and the float64
restatement against the tolerance M (sens + u scale) that the GPU test uses."""
import numpy as np
import pytest
from mpmath import mp, mpf

import round_collider_mp as rc

# one vertex per region, away from the end planes (the distance is only C^1 across them, mp.diff must stay inside one region)
SHAPES = rc.cases()
POINTS = [("solid_sphere", 0), ("solid_sphere", 9), ("hollow_sphere", 0), ("hollow_sphere", 15), ("capsule_aligned", 1), ("capsule_aligned", 6),
          ("capsule_aligned", 7), ("capsule_skew", 0), ("capsule_skew", 8), ("capsule_skew", 9), ("capsule_skew", 37)]


def _region(c, x):
    s, r, m, a, sideRegion, side = rc.evaluate(rc.MP, c, x)
    return "side" if sideRegion else "cap"


def test_the_points_cover_every_region_and_lie_inside_dhat():
    seen = set()
    for name, v in POINTS:
        c, P, dbc = SHAPES[name]
        assert rc.active(c, P[v], 0, rc.DHAT), (name, v)
        seen.add((name.split("_")[0] if "capsule" in name else name, _region(c, P[v])))
    assert {("capsule", "side"), ("capsule", "cap"), ("solid_sphere", "cap"), ("hollow_sphere", "cap")} <= seen


@pytest.mark.parametrize("name,v", POINTS)
def test_gradient_and_projected_hessian_equal_mp_diff(name, v):
    c, P, dbc = SHAPES[name]
    x = P[v]
    E, g, H = rc.vertex_terms(rc.MP, c, x, rc.DHAT, rc.KAPPA)
    assert abs(E - rc.energy_mp(c, [mpf(q) for q in x], rc.DHAT, rc.KAPPA)) == 0
    gd = rc.gradient_mp_diff(c, x, rc.DHAT, rc.KAPPA)
    gs = max(abs(q) for q in gd)
    assert max(abs(a - b) for a, b in zip(g, gd)) <= mpf(10) ** -30 * gs
    Hx = rc.exact_hessian_mp(c, x, rc.DHAT, rc.KAPPA)
    Hp = rc.psd_project_mp(Hx)
    hs = max(abs(Hx[i, j]) for i in range(3) for j in range(3))
    assert max(abs(H[i][j] - Hp[i, j]) for i in range(3) for j in range(3)) <= mpf(10) ** -25 * hs
    # what the clamp does: nothing inside a hollow sphere (the exact Hessian is PSD there), the curvature term dropped on a solid collider
    ev = mp.eigsy(Hx, eigvals_only=True)
    if c["hollow"]:
        assert min(ev) > 0
    else:
        assert min(ev) < 0 and sum(1 for e in ev if e > mpf(10) ** -20 * hs) == 1


def test_the_end_plane_belongs_to_the_cap_region():
    c = SHAPES["capsule_aligned"][0]
    for x in ([0.0, 0.5625, 0.0], [1.0, 0.0, -0.53125]):
        assert _region(c, x) == "cap" and rc.active(c, x, 0, rc.DHAT)
    assert _region(c, [2.0 ** -40, 0.5625, 0.0]) == "side"


def test_no_state_yields_nan():
    for name, (c, P, dbc) in SHAPES.items():
        for x in (c["p0"], c["p1"]):  # r = 0: on the segment
            s, r, m, a, sideRegion, side = rc.evaluate(rc.NP, c, x)
            assert r == 0.0 and m == [0.0, 0.0, 0.0] and s == -side * c["R"]
            assert rc.step_bound(rc.NP, c, x, [1.0, 0.0, 0.0], 0.9) is None or c["hollow"]
    c = SHAPES["hollow_sphere"][0]
    assert c["R"] ** 2 > rc.DHAT and not rc.active(c, c["p0"], 0, rc.DHAT)  # R^2 > dHat: the centre is never active


@pytest.mark.parametrize("name", list(SHAPES))
def test_step_bound_agrees_with_findroot(name):
    c = SHAPES[name][0]
    hits = 0
    for x, p, label in rc.rays(name):
        t = rc.step_bound(rc.MP, c, x, p, 0.9)
        s0 = rc.evaluate(rc.MP, c, x)[0]
        f = lambda q: rc.gap_along_ray_mp(c, x, p, q) - (1 - mpf(0.9)) * s0  # (the slackness is the double 0.9)
        if t is None:
            # never down to a tenth of the gap along the whole ray (sampled: the gap is a smooth function with one minimum)
            assert all(f(mpf(k) / 64) > 0 for k in range(0, 64 * 40)), (name, label)
            continue
        hits += 1
        root = mp.findroot(f, t)
        assert abs(root - t) <= mpf(10) ** -30 * max(abs(t), 1), (name, label)
        # the FIRST such t: the gap stays above the target before it
        assert all(f(t * k / 257) > 0 for k in range(0, 257)), (name, label)
        assert rc.gap_along_ray_mp(c, x, p, t) > 0
    assert hits >= 3


def test_friction_terms_equal_mp_diff():
    n = [mpf(3) / 5, mpf(0), mpf(4) / 5]  # a unit vector in mpmath, not only in float64
    lam, mu, eps2 = mpf("12.5"), mpf("0.4"), mpf("1e-6")
    xt = [0.1, 0.2, 0.3]
    for x in ([0.13, 0.19, 0.33], [0.1002, 0.2001, 0.2999]):
        E, g, H = rc.friction_terms(rc.MP, n, lam, x, xt, mu, eps2)
        f = lambda *y: rc.friction_terms(rc.MP, n, lam, list(y), xt, mu, eps2)[0]
        for i in range(3):
            gd = mp.diff(f, tuple(mpf(q) for q in x), tuple(1 if k == i else 0 for k in range(3)))
            assert abs(g[i] - gd) <= mpf(10) ** -30 * abs(mu * lam)
        assert min(mp.eigsy(mp.matrix(H), eigvals_only=True)) >= -mpf(10) ** -40 * abs(mu * lam / mp.sqrt(eps2))


def test_numpy_restatement_meets_the_tolerance():
    worst = rc.numpy_worst_ratio()
    print("float64 restatement, worst err / (sens + u scale): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    top = max(worst.values())
    assert top <= rc.M and rc.M == 2.0 ** np.ceil(np.log2(top))  # M: the worst ratio rounded up to a power of two
    assert abs(top - rc.NUMPY_WORST_RATIO) <= 5e-3
