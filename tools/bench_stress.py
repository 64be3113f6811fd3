"""Times `ipcgpu_elastic_stress` at mat150 (twisted state after three time steps), NH and FCR, beside `ipcgpu_elastic_energy`: HIP events recorded on the
context's stream (`ipcgpu_ctx_get_stream`) around the blocking call, and the wall clock around the same call.  Variants: pass 1 alone (every output
pointer but the count null: kernel, the count through mapped host memory, one synchronisation); both passes with the nodal array read back; the whole call
with both arrays.  Prints one JSON object.  For the two kernels' own durations run it under `rocprofv3 --kernel-trace --stats` (tools/rocprof_summary.py).
    python tools/bench_stress.py [out.json] [--reps N]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ipc_amd  # noqa: E402
from ipc_amd import scene  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
ipc_amd.load_library()
hip = C.CDLL("libamdhip64.so")
V, F = scene.make_mat(150)
left, right = scene.border_verts(V, 0.01)
c = ipc_amd.Context(0)
c.set_mesh(V, F, YM=1e5, PR=0.4, density=1000.0)
c.opt_init(0.04, False)
c.set_twist(left, right)
c.set_rel_tol(1e-2)
c.precompute()
for _ in range(3):
    c.solve_timestep(50)
nV, nT = c.nV, c.nT
L, dp = c._L, ipc_amd.lib._dp
stream = C.c_void_p()
assert L.ipcgpu_ctx_get_stream(c.h, C.byref(stream)) == 0
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0
elem, node, cnt = np.zeros((nT, 8), order="F"), np.zeros((nV, 8), order="F"), C.c_int()


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    wall, dev = [], []
    ms = C.c_float()
    for _ in range(REPS):
        assert hip.hipEventRecord(ev[0], stream) == 0
        t0 = time.perf_counter()
        rc = fn()
        wall.append(1e6 * (time.perf_counter() - t0))
        assert rc == 0 and hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        dev.append(1e3 * ms.value)
    wall, dev = np.array(wall), np.array(dev)
    return dict(event_us_median=float(np.median(dev)), event_us_min=float(dev.min()), event_us_max=float(dev.max()), wall_us_median=float(np.median(wall)), reps=REPS)


out = {"nV": nV, "nT": nT}
for name in ("NH", "FCR"):
    c.set_energy_type(name)
    r = {}
    r["pass1_count_only"] = timed(lambda: L.ipcgpu_elastic_stress(c.h, None, None, C.byref(cnt)))
    r["both_passes_nodal_readback"] = timed(lambda: L.ipcgpu_elastic_stress(c.h, None, dp(node), C.byref(cnt)))
    r["pass1_element_readback"] = timed(lambda: L.ipcgpu_elastic_stress(c.h, dp(elem), None, C.byref(cnt)))
    r["full_call_both_readbacks"] = timed(lambda: L.ipcgpu_elastic_stress(c.h, dp(elem), dp(node), C.byref(cnt)))
    E = C.c_double()
    r["elastic_energy"] = timed(lambda: L.ipcgpu_elastic_energy(c.h, C.c_double(1.0), C.byref(E)))
    r["n_invalid"] = cnt.value
    r["von_mises_max"] = float(np.nanmax(elem[:, 6]))
    out[name] = r
c.set_energy_type("NH")
for e in ev:
    hip.hipEventDestroy(e)
c.close()
if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
