#!/usr/bin/env python3
"""Writes tests/golden/shell_limit_mp_cases.npz from tests/shell_limit_mp.py (the project's own mpmath restatement of the shells' strain limit; nothing of
the reference is involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind shell_limit_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shell_limit_mp as lmp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in lmp.QUANT}
        for c in lmp.load():
            n = lmp.numpy_restatement(c)
            for k in lmp.QUANT:
                if k == "E" and c["E"] == np.inf:
                    r = 0.0 if n["E"] == np.inf else np.inf
                else:
                    r = float(np.max(lmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + lmp.U * c["scale_" + k])))
                print(f"{c['name']:50s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = lmp.pack()
    os.makedirs(os.path.dirname(lmp.GOLDEN), exist_ok=True)
    np.savez_compressed(lmp.GOLDEN, **out)
    print(lmp.GOLDEN, os.path.getsize(lmp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
