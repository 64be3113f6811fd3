#!/usr/bin/env python3
"""Writes tests/golden/aero_mp_cases.npz from tests/aero_mp.py (the project's own mpmath restatement of the air-drag potential; nothing of the
reference is involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind aero_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aero_mp as cmp_  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in cmp_.QUANT}
        for c in cmp_.load():
            n = cmp_.numpy_restatement(c)
            for k in cmp_.QUANT:
                r = float(np.max(cmp_.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + cmp_.U * c["scale_" + k])))
                print(f"{c['name']:45s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = cmp_.pack()
    os.makedirs(os.path.dirname(cmp_.GOLDEN), exist_ok=True)
    np.savez_compressed(cmp_.GOLDEN, **out)
    print(cmp_.GOLDEN, os.path.getsize(cmp_.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
