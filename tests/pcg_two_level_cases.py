"""The shapes the two-level preconditioner is tested on (tests/test_pcg_coarse.py, tests/test_gpu_pcg_two_level.py): the twisted 16 x 3 x 3 bar of
tests/test_gpu_pcg.py (272 nodes: correctness only, a coarse space hardly helps it) and a thin stiff 40 x 1 x 40 sheet (3362 nodes: the convergence shape)."""
import numpy as np

from ipc_amd import scene

DTSQ = 0.025 ** 2
MATERIAL = dict(YM=1e5, PR=0.4, density=1000.0)


def make(orc, which):
    if which == "bar":
        V, F = scene.make_bar(16, 3, 3, size=(6.0, 0.75, 1.0))
        Vt = scene.twist_state(scene.jitter(V, F), 0.25)
    elif which == "sheet":
        V, F = scene.make_bar(40, 1, 40, size=(1.0, 0.025, 1.0))
        Vt = scene.twist_state(scene.jitter(V, F), 0.1)
    else:
        raise ValueError(which)
    left, right = scene.border_verts(V, 0.01)
    dbc = np.concatenate([left, right])
    m = orc.Mesh(V, F, **MATERIAL)
    m.set_dbc(dbc, 2)
    m.set_V(Vt)
    ia, ja = m.pattern()
    fixed = np.zeros(V.shape[0], dtype=bool)
    fixed[dbc] = True
    return dict(V=V, F=F, Vt=Vt, m=m, dbc=dbc, ia=ia, ja=ja, fixed=fixed)


def rhs(case, seed=14):
    return np.random.default_rng(seed).normal(size=len(case["ia"]) - 1)
