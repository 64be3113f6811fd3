#!/usr/bin/env python3
"""Writes tests/golden/shell_mp_cases.npz from tests/shell_mp.py (the project's own mpmath restatement of the shell energies; nothing of the reference is
involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind shell_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shell_mp as smp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in smp.QUANT}
        for c in smp.load():
            n = smp.numpy_restatement(c)
            for k in smp.QUANT:
                r = float(np.max(np.abs(n[k] - c[k]) / (np.asarray(c["sens_" + k]) + smp.U * c["scale_" + k])))
                print(f"{c['name']:45s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = smp.pack()
    os.makedirs(os.path.dirname(smp.GOLDEN), exist_ok=True)
    np.savez_compressed(smp.GOLDEN, **out)
    print(smp.GOLDEN, os.path.getsize(smp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
