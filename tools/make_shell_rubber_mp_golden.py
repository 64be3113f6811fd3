#!/usr/bin/env python3
"""Writes tests/golden/shell_rubber_mp_cases.npz from tests/shell_rubber_mp.py (the project's own mpmath restatement of the shells' rubber membrane; nothing
of the reference is involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind
shell_rubber_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shell_rubber_mp as rmp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in rmp.QUANT}
        for c in rmp.load():
            n = rmp.numpy_restatement(c)
            for k in rmp.QUANT:
                if k == "E" and c["E"] == np.inf:
                    r = 0.0 if n["E"] == np.inf else np.inf
                else:
                    r = float(np.max(rmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + rmp.U * c["scale_" + k])))
                print(f"{c['name']:55s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = rmp.pack()
    os.makedirs(os.path.dirname(rmp.GOLDEN), exist_ok=True)
    np.savez_compressed(rmp.GOLDEN, **out)
    print(rmp.GOLDEN, os.path.getsize(rmp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
