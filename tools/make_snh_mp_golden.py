"""Writes tests/golden/snh_mp_cases.npz: the hand-placed stable-neo-Hookean elements of tests/snh_mp.py and the 48 tets of the block mesh (inputs as exact doubles),
their mpmath references rounded to double and the per-quantity sensitivities.  Inputs and mp results only.  Deterministic: a second run writes the same bytes.

    python tools/make_snh_mp_golden.py [-j N] [--out FILE]      write the file
    python tools/make_snh_mp_golden.py --measure                print the worst and median err / (sens + u scale) per quantity of the float64 NumPy restatement over
                                                                the stored cases (the margin M of snh_mp.py)
"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import snh_mp as smp  # noqa: E402
from make_stencil_mp_golden import save_npz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--out", default=smp.GOLDEN)
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        for k, (worst, name, median) in smp.numpy_ratios(a.out).items():
            print(f"{k}: worst err / (sens + u scale) = {worst:.3g} ({name}), median {median:.3g}")
        return
    with multiprocessing.Pool(min(a.j, 16)) as pool:
        Z = smp.pack(map_fn=lambda f, jobs: pool.map(f, jobs, chunksize=1))
    save_npz(a.out, Z)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; {len(Z['e_name'])} elements, {len(Z['b_name'])} block tets")


if __name__ == "__main__":
    main()
