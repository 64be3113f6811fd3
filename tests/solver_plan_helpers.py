"""The launch plan of the multifrontal solver for the pattern a GPU context holds, from the host planner: one place for the GPU tests that need to know which
kernels a mesh takes (the shim of tests/mf_symbolic, read the way tests/test_mf_plan.py reads it)."""
import numpy as np


def host_plan(c, V, **tune):
    """analysis + both planner steps on the context's own CSR pattern; asserts that the analysis is the device's (entry destinations, bit for bit)"""
    from test_mf_plan import make_plan
    from test_mf_symbolic import analyze
    from test_sharding_gloo import _shim_lib
    shim = _shim_lib()
    ia, ja = c.get_pattern()
    o = analyze(shim, np.ascontiguousarray(ia, np.int32), np.ascontiguousarray(ja, np.int32), V, leaf=12)
    assert np.array_equal(c.entry_destinations(), o["aDst"])
    p = make_plan(shim, o, **tune)
    p["sym"] = o
    return p
