"""Writes tests/golden/elastic_mp_cases.npz: the hand-placed elastic elements and step-bound cases of tests/elastic_mp.py (inputs as exact doubles), their
mpmath references rounded to double and the per-quantity sensitivities.  Deterministic: a second run writes the same bytes.

    python tools/make_elastic_mp_golden.py [-j N] [--out FILE]      write the file
    python tools/make_elastic_mp_golden.py --measure                print the oracle's worst and median err / (sens + u scale) per quantity over the stored cases
                                                                    (the margin M of elastic_mp.py)
"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import elastic_mp as emp  # noqa: E402
from make_stencil_mp_golden import save_npz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--out", default=emp.GOLDEN)
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        from oracle import orc
        orc.build()
        for k, (worst, name, median) in emp.oracle_ratios(orc, a.out).items():
            print(f"{k}: worst err / (sens + u scale) = {worst:.3g} ({name}), median {median:.3g}")
        return
    with multiprocessing.Pool(min(a.j, 16)) as pool:
        Z = emp.pack(emp.element_cases(), emp.step_cases(), map_fn=lambda f, jobs: pool.map(f, jobs, chunksize=1))
    save_npz(a.out, Z)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; {len(Z['e_name'])} elements, {len(Z['s_name'])} step bounds")


if __name__ == "__main__":
    main()
