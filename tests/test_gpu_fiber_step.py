"""Fibres through the stepper: the analytic equilibrium of a free block, actuation by a ramped activation, anisotropy of a gripped block, the status file, and
the refusals (plastic elements, sharded contexts, act >= 1, activation on exp)."""
import numpy as np
import pytest
from mpmath import mp, mpf

import elastic_mp as emp
import fiber_mp as fm
from test_gpu_fiber_mp import block_mesh

pytestmark = pytest.mark.gpu

YM, PR, K, ACT, H = 1e5, 0.4, 5e4, 0.3, 0.05
EX = np.array([1.0, 0.0, 0.0])


def roots(act, k=K):
    """the homogeneous equilibrium F = diag(l, s, s) of an NH block with spring fibres along x: d/dl and d/ds of psi_NH(l, s, s) + k (l - l0)^2 / 2 vanish"""
    with mp.workdps(50):
        mu, lam = emp.lame(YM, PR)
        W = lambda l, s: emp.psi_sigma(emp.NH, [l, s, s], mu, lam) + mpf(k) * (l - (1 - mpf(act))) ** 2 / 2
        f = lambda l, s: (mp.diff(W, (l, s), (1, 0)), mp.diff(W, (l, s), (0, 1)))
        l, s = mp.findroot(f, (mpf(1) - mpf(act) / 2, mpf(1) + mpf(act) / 4), tol=mpf(10) ** -40)
        return l, s, mu, lam


def _block(gpu_lib, X, T, dt=0.01, density=1000.0):
    c = gpu_lib.Context(0)
    c.set_mesh(X, T, YM=YM, PR=PR, density=density)
    c.opt_init(dt, False)  # no gravity; no contact
    c.set_time_integration("BE")
    return c


@pytest.mark.parametrize("rotated", [False, True], ids=["axis", "oblique"])
def test_analytic_equilibrium(gpu_lib, rotated):
    """At x = F X, F = diag(l, s, s) with the mp roots, the elastic and the fibre gradient cancel at EVERY node (linear tets represent the state exactly).
    Tolerance per gradient entry, summed over the incident elements:
      fibre part    fiber_mp's M (sens + u scale) of the assembled case;
      elastic part  elastic_mp's M = 256 times (u scale + 2 sens): scale = vol Pm sum|A| with Pm = mu sigma + mu / sigma + lam |ln J| / sigma the
                    first Piola stress with its terms replaced by their magnitudes; sens = vol Km dF sum|A|, Km = mu + (mu + lam (1 + |ln J|)) / sigma_min^2
                    the magnitude of dP/dF and dF = u |x|_max sum|A| what one ulp in every coordinate does to F -- twice, once for the kernel's rounding of F
                    and once for x = fl(F X) not being the exact equilibrium."""
    X, T = block_mesh(2, H)
    l, s, mu, lam = roots(ACT)
    R = fm.OBLIQUE if rotated else np.eye(3)
    F = np.diag([float(l), float(s), float(s)])
    Xr, x, a = X @ R.T, (X @ F.T) @ R.T, R @ EX
    c = _block(gpu_lib, Xr, T)
    c.set_fibers((0, len(T)), a, K)
    c.fiber_set_activation(0, ACT)
    c.set_positions(x)
    g = c.elastic_gradient(1.0, False) + c.fiber_gradient_add(1.0, False)
    gf = c.fiber_gradient_add(1.0, False)
    f = c.features()
    case = {"x": x, "elems": [fm.elem_record(f["restTriInv"][t], f["triArea"][t], T[t], a, K, act=ACT) for t in range(len(T))]}
    ref = fm.evaluate(case)
    tol = np.array(fm.tolerance(ref, "g"), dtype=np.float64)
    lnJ, sig = abs(float(mp.log(l * s * s))), min(float(l), float(s))
    Pm = float(mu) * max(float(l), float(s)) + float(mu) / sig + float(lam) * lnJ / sig
    Km = float(mu) + (float(mu) + float(lam) * (1 + lnJ)) / sig ** 2
    for t in range(len(T)):
        sA = float(np.abs(f["restTriInv"][t]).sum())
        e = emp.M * f["triArea"][t] * (emp.U * Pm * sA + 2 * Km * emp.U * float(np.abs(x).max()) * sA * sA)
        for v in T[t]:
            tol[3 * v:3 * v + 3] += e
    worst = float(np.max(np.abs(g) / tol))
    print(f"rotated {rotated}: l {float(l):.12f} s {float(s):.12f}; largest fibre force {np.abs(gf).max():.3g}, worst |residual| / tolerance {worst:.3g}")
    assert np.abs(gf).max() > 1e3 * tol.max()  # the two parts are far from zero on their own
    assert worst <= 1.0
    pe, tot = c.fiber_state()
    assert np.all(np.abs(pe[:, 0] - float(l)) <= 64 * fm.U * np.abs(f["restTriInv"]).sum(1) * np.abs(x).max())
    c.close()


RHO, DT, REL = 0.1, 1.0, 1e-9
RAMP = 6


def _actuated(gpu_lib):
    X, T = block_mesh(2, H)
    c = _block(gpu_lib, X, T, dt=DT, density=RHO)
    c.set_rel_tol(REL)
    c.set_fibers((0, len(T)), EX, K)
    c.precompute()
    return c, X, T


def _step(c, act):
    """one time step by hand: the incremental potential falls across every accepted line-search step, and the step converges"""
    c.fiber_set_activation(0, act)
    c.begin_timestep()
    E = c.state()["E"]
    for it in range(100):
        if c.newton_iter():
            break
        E1 = c.state()["E"]
        assert np.isfinite(E1) and E1 <= E, (act, it, E, E1)
        E = E1
    else:
        raise AssertionError("no convergence in 100 iterations")
    c.end_timestep()


def test_actuation_through_the_stepper(gpu_lib):
    """A free block, no gravity, act ramped 0 -> 0.3 over RAMP steps, then held for two.  Inertia's share: a node's mass is at most rho h^3 = 0.1 x 1.25e-4 kg,
    the fibre stiffness along the block k L = 5e4 x 0.1 N/m, so m / (dt^2 k L) = 1.25e-5 / 5e3 = 2.5e-9 < 1e-8: every step ends at the static equilibrium of its
    activation up to that share of the step's travel (< 0.005), 1.3e-11.
    Tolerance on the x-extent over the rest extent L = 0.1: the solver stops when the Newton step |p|_inf < targetGRes = REL x (bounding-box diagonal) x dt, with
    p = H_p^-1 g and H_p the projected Hessian.  At the equilibrium the fibres are in tension (l > l0: neither clamp of the fibre term acts) and the stretch
    modes of NH are positive definite; what the projection changes are the twist modes of the elements (the matrix is under compression along the fibres), and
    a twist leaves the extent of the block along its axis unchanged to first order.  So in the modes that set the extent p is the error of the iterate to first
    order; twice that for the second-order remainder, on each of the two faces: 4 targetGRes, plus the inertial lag on each face and 64 u L of rounding."""
    c, X, T = _actuated(gpu_lib)
    for n in range(RAMP + 2):
        _step(c, ACT * min(1.0, (n + 1) / RAMP))
    l, s, _, _ = roots(ACT)
    st = c.state()
    V, L = st["V"], X[:, 0].max() - X[:, 0].min()
    got = (V[:, 0].max() - V[:, 0].min()) / L
    tol = (4 * st["targetGRes"] + 2 * 2.5e-9 * 0.005 + 64 * fm.U * L) / L
    assert abs(st["targetGRes"] - REL * np.sqrt(3) * L * DT) <= 1e-12 * st["targetGRes"]
    print(f"actuated block: extent ratio {got:.12f}, mp root {float(l):.12f}, |difference| {abs(got - float(l)):.3g}, tolerance {tol:.3g}")
    assert abs(got - float(l)) <= tol
    assert abs((V[:, 1].max() - V[:, 1].min()) / L - float(s)) <= tol  # and it bulges sideways by the second root
    assert float(l) < 0.95  # the block did contract (fibres in series with the matrix: about 1 - act k / (k + E) = 0.9)
    c.close()


HG = 0.0625  # a power of two: restTriInv is +-16 exactly, and an element edge along y that lies in a grip keeps l = 1 EXACTLY across the fibres


def _gripped(gpu_lib, a, tension_only):
    """the block gripped on its faces x = 0 and x = L, the second moved 10 % out in two steps: the same scripted Dirichlet displacement for every fibre direction"""
    X, T = block_mesh(2, HG)
    c = _block(gpu_lib, X, T, dt=0.02)
    c.set_rel_tol(1e-7)
    face = lambda xv: np.flatnonzero(X[:, 0] == xv).astype(np.int32)
    c.add_dirichlet(face(0.0))
    c.add_dirichlet(face(2 * HG), lin_vel=(0.1 * 2 * HG / (2 * 0.02), 0.0, 0.0))
    c.set_fibers((0, len(T)), a, K, tension_only=tension_only)
    c.precompute()
    for _ in range(2):
        assert c.solve_timestep(200) < 200
    pe, tot = c.fiber_state()
    E = c.fiber_energy()
    assert np.all(np.abs(c.state()["V"][face(2 * HG), 0] - 2.2 * HG) <= 1e-15)
    c.close()
    return E, pe, tot


def test_anisotropy(gpu_lib):
    along, pe_a, tot_a = _gripped(gpu_lib, EX, False)
    across, pe_c, tot_c = _gripped(gpu_lib, [0.0, 1.0, 0.0], False)
    print(f"fibre energy along {along:.6g}, across {across:.6g}; tension sum along {pe_a[:, 1].sum():.6g}, across {pe_c[:, 1].sum():.6g}")
    # the reaction is larger along the fibres (10 % of stretch against the 4 % of Poisson contraction across them); across them the fibres are compressed
    assert along > across > 0 and pe_a[:, 1].sum() > abs(pe_c[:, 1].sum()) and pe_a[:, 1].min() > 0 and pe_c[:, 1].max() <= 0 and pe_c[:, 1].sum() < 0
    assert tot_a[2] == along and tot_a[1] > 1.05 and tot_c[1] <= 1.0 and tot_c[0] < 0.99  # stretched along, contracted across (1 exactly in the grips)
    E, pe, tot = _gripped(gpu_lib, [0.0, 1.0, 0.0], True)
    assert E == 0.0 and tot[2] == 0.0 and not pe[:, 1].any() and tot[1] <= 1.0  # across the fibres the tension-only bar's fibre energy is exactly 0


def test_status_round_trip(gpu_lib, tmp_path):
    """save after step 3, load into a fresh context, take step 4: positions and fiber_get equal the uninterrupted run's to the bit (the standard
    tests/test_gpu_plastic_step.py holds its section to)"""
    def fresh():
        X, T = block_mesh(2, H)
        c = _block(gpu_lib, X, T, dt=0.02)
        c.set_rel_tol(1e-4)  # (what is compared is bit-equality of two runs, not how far each step is converged)
        c.add_dirichlet(np.flatnonzero(X[:, 0] == 0.0).astype(np.int32))
        return c, T
    c, T = fresh()
    c.set_fibers((0, 30), [0.3, -0.5, 0.8], K, group=2)
    c.set_fibers((30, 40), EX, 2e4, law="exp", k2=3.0, group=1)
    c.set_fibers((40, 44), [0.0, 0.0, 1.0], 1e4, tension_only=True, group=5)
    c.precompute()
    for n in range(4):
        c.fiber_set_activation(2, 0.1 * (n + 1))
        assert c.solve_timestep(200) < 200
        if n == 2:
            c.save_status(tmp_path / "status")
    want, fg = c.state()["V"].copy(), c.fiber_get()
    c.close()
    txt = open(tmp_path / "status").read().split()
    i = txt.index("fiber")
    assert txt[i + 1:i + 4] == [str(len(T)), "7", "64"] and len(txt) == i + 4 + 64 + 7 * len(T) and txt.index("dx_Elastic") < i
    c2, _ = fresh()
    c2.load_status(tmp_path / "status")
    c2.precompute()
    assert c2.fiber_get()["act"][2] == 0.1 * 3  # (the file carries 20 significant digits)
    c2.fiber_set_activation(2, 0.1 * 4)
    assert c2.solve_timestep(200) < 200
    fg2 = c2.fiber_get()
    assert np.array_equal(c2.state()["V"], want)
    assert fg2["n"] == fg["n"] == 44 and all(np.array_equal(fg[k], fg2[k]) for k in ("k", "k2", "law", "tensionOnly", "group", "dir", "act"))
    lines = open(tmp_path / "status").read().splitlines()
    open(tmp_path / "cut", "w").write("\n".join(lines[:-3]) + "\n")
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*fiber"):
        c2.load_status(tmp_path / "cut")
    # an edited file goes through the rules of set_fibers / fiber_set_activation: an activation on the group of the exp elements, a direction that is no unit vector
    h = next(i for i, ln in enumerate(lines) if ln.startswith("fiber "))
    acts = lines[h + 1].split()
    acts[1] = "0.2"
    open(tmp_path / "act", "w").write("\n".join(lines[:h + 1] + [" ".join(acts)] + lines[h + 2:]) + "\n")
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*exp"):
        c2.load_status(tmp_path / "act")
    row = lines[h + 2].split()
    row[4] = "2.0"
    open(tmp_path / "dir", "w").write("\n".join(lines[:h + 2] + [" ".join(row)] + lines[h + 3:]) + "\n")
    with pytest.raises(gpu_lib.IpcGpuError, match="ipcgpu error -3.*unit vector"):
        c2.load_status(tmp_path / "dir")
    assert all(np.array_equal(fg[k], c2.fiber_get()[k]) for k in ("k", "dir", "act"))  # the refused files changed nothing
    c2.close()
    # a run without fibres writes the file it always wrote
    c3, _ = fresh()
    c3.precompute()
    c3.save_status(tmp_path / "plain")
    assert "fiber" not in open(tmp_path / "plain").read().split()
    c3.close()


def test_refusals(gpu_lib):
    X, T = block_mesh(2, H)
    E = gpu_lib.IpcGpuError
    c = gpu_lib.Context(0)
    c.set_mesh(X, T, YM=YM, PR=PR, density=1000.0)
    c.set_plasticity((10, 20), 0.05)
    with pytest.raises(E, match="ipcgpu error -4.*plastic"):
        c.set_fibers((0, 11), EX, K)  # element 10 is plastic
    assert c.fiber_get()["n"] == 0
    c.set_fibers((0, 10), EX, K)
    with pytest.raises(E, match="ipcgpu error -4.*fibred"):
        c.set_plasticity((9, 12), 0.05)  # element 9 is fibred
    assert int(np.sum(c.plastic_get()["yield"] < np.inf)) == 10
    c.set_plasticity((0, 10), np.inf)  # switching plasticity OFF on fibred elements is no conflict
    with pytest.raises(E, match="ipcgpu error -1"):
        c.fiber_set_activation(0, 1.0)
    with pytest.raises(E, match="ipcgpu error -1"):
        c.fiber_set_activation(0, 1.5)
    c.set_fibers((20, 30), EX, K, law="exp", k2=2.0, group=4)
    with pytest.raises(E, match="ipcgpu error -1.*exp"):
        c.fiber_set_activation(4, 0.2)
    c.fiber_set_activation(7, 0.2)
    with pytest.raises(E, match="ipcgpu error -1.*exp"):
        c.set_fibers((30, 32), EX, K, law="exp", k2=2.0, group=7)
    for bad in (dict(tet_range=(-1, 4)), dict(tet_range=(0, len(T) + 1)), dict(direction=[0.0, 0.0, 0.0]), dict(direction=[np.nan, 0.0, 1.0]), dict(k=-1.0),
                dict(law="exp", k2=0.0), dict(law=2), dict(group=64), dict(group=-1)):
        kw = dict(tet_range=(0, 4), direction=EX, k=K)
        kw.update(bad)
        with pytest.raises(E, match="ipcgpu error -1"):
            c.set_fibers(**kw)
    assert c.fiber_get()["n"] == 20 and c.fiber_get()["act"][7] == 0.2  # the refused calls changed nothing
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_shard(0, 2)
    c.close()
    c = gpu_lib.Context(0)
    c.set_mesh(X, T, YM=YM, PR=PR, density=1000.0)
    c.set_shard(0, 2)
    with pytest.raises(E, match="ipcgpu error -4"):
        c.set_fibers((0, 4), EX, K)
    c.close()
    c = gpu_lib.Context(0)
    c.set_mesh(X, T, YM=YM, PR=PR, density=1000.0)
    with pytest.raises(E, match="ipcgpu error -3"):
        c.fiber_set_activation(0, 0.1)  # before any fibre
    c.close()
