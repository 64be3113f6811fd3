#!/usr/bin/env python3
"""Writes tests/golden/attach_mp_cases.npz from tests/attach_mp.py (the project's own mpmath restatement of the attachment energy; nothing of the reference
is involved).  --measure: prints err / (sens + u scale) of the float64 restatement per case and quantity, the figure behind attach_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attach_mp as amp  # noqa: E402


def main():
    if "--measure" in sys.argv:
        worst = {k: (0.0, "") for k in amp.QUANT}
        for c in amp.load():
            n = amp.numpy_restatement(c)
            for k in amp.QUANT:
                r = float(np.max(amp.ratio(n[k] - c[k], np.asarray(c["sens_" + k]) + amp.U * c["scale_" + k])))
                print(f"{c['name']:45s} {k} {r:.3g}")
                worst[k] = max(worst[k], (r, c["name"]))
        print({k: v for k, v in worst.items()})
        return
    out = amp.pack()
    os.makedirs(os.path.dirname(amp.GOLDEN), exist_ok=True)
    np.savez_compressed(amp.GOLDEN, **out)
    print(amp.GOLDEN, os.path.getsize(amp.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
