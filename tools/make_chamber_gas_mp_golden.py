"""Writes tests/golden/chamber_gas_mp_cases.npz: the states of tests/chamber_gas_mp.py (three chambers in one scene, four states) with V, gauge, beta, W,
gradV and the gradient of every gas chamber in mpmath, their one-ulp sensitivities and their scales.  --measure prints the worst
err / (sens + u scale) of the float64 NumPy restatement per quantity: the number behind chamber_gas_mp.M."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamber_gas_mp as gm  # noqa: E402

if __name__ == "__main__":
    if "--measure" in sys.argv:
        X, ch, off = gm.scene()
        worst = {}
        for name, x, refs in gm.load():
            for i, ref in refs.items():
                got = gm.numpy_restatement(ch[i], x)
                for k in gm.QUANT:
                    worst[k] = max(worst.get(k, 0.0), gm.ratio(np.asarray(got[k]) - np.asarray(ref[k]), ref, k))
        print("worst err / (sens + u scale) of the float64 restatement: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    else:
        np.savez_compressed(gm.GOLDEN, **gm.pack())
        print(gm.GOLDEN, os.path.getsize(gm.GOLDEN), "bytes")
