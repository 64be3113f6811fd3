#!/usr/bin/env python3
"""Writes tests/golden/rod_mp_cases.npz from tests/rod_mp.py (the project's own mpmath restatement of the rod energies; nothing of the reference is
involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind rod_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rod_mp as rmp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in rmp.QUANT}
        for c in rmp.load():
            n = rmp.numpy_restatement(c)
            for k in rmp.QUANT:
                r = float(np.max(np.abs(n[k] - c[k]) / (np.asarray(c["sens_" + k]) + rmp.U * c["scale_" + k])))
                print(f"{c['name']:45s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = rmp.pack()
    os.makedirs(os.path.dirname(rmp.GOLDEN), exist_ok=True)
    np.savez_compressed(rmp.GOLDEN, **out)
    print(rmp.GOLDEN, os.path.getsize(rmp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
