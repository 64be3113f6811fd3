"""Writes tests/golden/stress_cases.npz: the element cases of tests/stress_mp.py (inputs as exact doubles), their mpmath stress records rounded to double, the
scales, and the error of the plain float64 NumPy restatement in units of eps x scale -- per case and the worst per energy, the baseline of the GPU
tolerance.  Deterministic: a second run writes the same bytes.

    python tools/make_stress_mp_golden.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import stress_mp as smp  # noqa: E402
from make_stencil_mp_golden import save_npz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=smp.GOLDEN)
    a = ap.parse_args()
    Z = smp.pack()
    save_npz(a.out, Z)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; {len(Z['name'])} cases")
    for nm in ("NH", "FCR"):
        w = float(Z["numpy_worst_" + nm])
        i = int(max((i for i in range(len(Z["name"])) if str(Z["name"][i]).startswith(nm)), key=lambda i: Z["numpy_ratio"][i]))
        print(f"{nm}: NumPy restatement worst err / (eps scale) = {w:.4g} ({Z['name'][i]}), K = {smp.margin(w):g}")


if __name__ == "__main__":
    main()
