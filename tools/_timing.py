"""HIP-event timing on a context's own stream, shared by the kernel bench tools (bench_shell.py, bench_rod.py, bench_shell_limit.py)."""
import ctypes as C

import numpy as np
import torch


def stream_of(c):
    p = C.c_void_p()
    c._chk(c._L.ipcgpu_ctx_get_stream(c.h, C.byref(p)))
    return torch.cuda.ExternalStream(p.value)


def timed(c, fn, reps):
    """(median, minimum) in ms of fn() over reps calls after one warm-up call, between two events on the stream of context c"""
    s = stream_of(c)
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))
