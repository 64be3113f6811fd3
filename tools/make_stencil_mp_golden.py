"""Writes tests/golden/stencil_mp_cases.npz: the hand-placed contact / friction stencils of tests/stencil_mp.py (inputs as exact doubles), their mpmath
references rounded to double and the per-quantity sensitivities.  Deterministic: a second run writes the same bytes.

    python tools/make_stencil_mp_golden.py [-j N] [--out FILE]      write the file
    python tools/make_stencil_mp_golden.py --measure                print the oracle's worst err / (sens + u scale) over the stored cases (the margin M of stencil_mp.py)
"""
import argparse
import io
import zipfile
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stencil_mp as smp  # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--out", default=smp.GOLDEN)
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        so = smp
        from oracle import orc
        orc.build()
        for fam, worst in so.oracle_ratios(orc).items():
            print(f"{fam}: worst err / (sens + u scale) = {worst[0]:.3g}  ({worst[1]})")
        return
    with multiprocessing.Pool(a.j) as pool:
        Z = smp.pack(smp.contact_cases(), smp.friction_cases(), smp.high_mult_cases(), map_fn=lambda f, jobs: pool.map(f, jobs, chunksize=1))
    save_npz(a.out, Z)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; cases per bin {np.bincount(4 * Z['c_para'] + Z['c_kind'], minlength=8).tolist()}, "
          f"{len(Z['f_kind'])} friction, {len(Z['h_kind'])} shared-point")


if __name__ == "__main__":
    main()
