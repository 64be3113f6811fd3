"""The plumbing around the codimensional energies changes no result: the scene of tools/make_codim_parity_golden.py (a five-tet cube over the ground, a
strain-limited cloth, a rod, gravity and lagged damping -- shell, limit and rod live in each of the five assemblies: the atomic gradient taken before
the pattern exists, the patch gradient, the Newton system, the damping matrix, and the speculative system in the case without damping and ground), replayed on the built library,
against what the commit BEFORE the plumbing was unified recorded (tests/golden/codim_parity.npz).

Tolerance: measured on that earlier commit, never on the code under test.  Five runs of the generator there agree bit for bit in every recorded array
(d = 0 for all of them, stored in the golden as d_<array> with the ten pairwise deviations as spread_<array>, and in
profiles/codim_refactor_parity.json), and their Newton counts agree; so equality is asserted.  (Had the runs differed, the bound would be 8 d per array,
relative to its largest magnitude: the factor for the tail that five samples under-estimate.)

What the equality rests on: the kernels are the same machine code as on that commit.  With the views' shared fields (CodimBase) in front of each view's
own the compiler ordered the loads and atomic adds of four scatter kernels differently, and the replay differed in the last bit of a few CSR values
(8.3e-17 of the largest) and, with the iterative solver, by one Newton iteration in the second step; hence the base lies behind the own fields
(codim_view.h).  A shared helper for the pair loops of k_rod_bend / k_shell_limit changed the code of those two kernels as well (its effect on the
sums was not measured by itself), so the two loops are written out."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_codim_parity_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "codim_parity.npz")


@pytest.mark.parametrize("case", sorted(gen.CASES))
def test_replay_matches_the_recording_of_the_commit_before_the_unification(gpu_lib, case):
    G = np.load(GOLDEN)
    got = gen.replay(gpu_lib, **gen.CASES[case])
    print(f"{case}: Newton iterations {got['iters'].tolist()} (recorded {G[case + '_iters'].tolist()})")
    bad = []
    for k in gen.FIELDS:
        want, d = G[f"{case}_{k}"], float(G[f"d_{case}_{k}"])
        dev = gen.rel_dev(got[k], want)
        print(f"{case} {k}: deviation {dev:.3g} of the largest magnitude {np.abs(want).max():.6g}, allowed {gen.FACTOR * d:.3g}")
        assert got[k].shape == want.shape
        if not dev <= gen.FACTOR * d:
            bad.append(f"{k}: {dev:.3g} > {gen.FACTOR * d:.3g}")
    assert np.array_equal(got["iters"], G[case + "_iters"])
    assert not bad, "; ".join(bad)
