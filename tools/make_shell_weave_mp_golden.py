#!/usr/bin/env python3
"""Writes tests/golden/shell_weave_mp_cases.npz from tests/shell_weave_mp.py (the project's own mpmath restatement of the shells' woven cloth; nothing of the
reference is involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind shell_weave_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shell_weave_mp as wmp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in wmp.QUANT}
        for c in wmp.load():
            n = wmp.numpy_restatement(c)
            for k in wmp.QUANT:
                r = float(np.max(wmp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + wmp.U * np.asarray(c["scale_" + k]))))
                print(f"{c['name']:65s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = wmp.pack()
    os.makedirs(os.path.dirname(wmp.GOLDEN), exist_ok=True)
    np.savez_compressed(wmp.GOLDEN, **out)
    print(wmp.GOLDEN, os.path.getsize(wmp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
