"""The entry points that half-spaces and round colliders share check their arguments alike (one body each in capi.cpp)."""
import numpy as np
import pytest

from test_gpu_collider_walk import bar_context

pytestmark = pytest.mark.gpu


def test_both_kinds_refuse_the_same_arguments(gpu_lib):
    """the entry points the two kinds share check their arguments alike: a null result, gradient, vertex list, direction or move, a non-finite move and
    an index out of range come back as IPCGPU_ERR_ARG (-1) from ipcgpu_halfspace_* as from ipcgpu_round_*, and the obstacle stays where it was"""
    import ctypes as C
    c, V = bar_context(gpu_lib)
    c.set_pattern()
    hs, rc = c.add_half_space([0.0, -0.6, 0.0], [0.0, 1.0, 0.0]), c.add_sphere_collider([0.0, -2.0, 0.0], 1.4)
    L, d = c._L, C.c_double
    nan3, ok3 = (d * 3)(0.0, float("nan"), 0.0), (d * 3)(0.0, 0.01, 0.0)
    for kind, idx in (("halfspace", hs), ("round", rc)):
        f = lambda name: getattr(L, f"ipcgpu_{kind}_{name}")  # noqa: E731
        i = C.c_int(idx)
        assert f("energy")(c.h, i, d(1.0), d(1.0), None) == -1, kind
        assert f("gradient_add")(c.h, i, d(1.0), d(1.0), None) == -1, kind
        assert f("set")(c.h, i, C.c_int(3), None) == -1, kind
        assert f("set")(c.h, i, C.c_int(-1), None) == -1, kind
        assert f("step_bound")(c.h, i, None, d(0.9), C.byref(d(1.0))) == -1, kind
        assert f("move")(c.h, i, None, d(0.5), None) == -1, kind
        assert f("move")(c.h, i, nan3, d(0.5), None) == -1, kind
        assert f("move")(c.h, i, ok3, d(1.5), None) == -1, kind
        assert f("energy")(c.h, C.c_int(7), d(1.0), d(1.0), C.byref(d())) == -1, kind
        assert f("set")(c.h, i, C.c_int(0), None) == 0, kind  # (an empty list needs no pointer)
    assert np.array_equal(c.round_get(rc)["p0"], [0.0, -2.0, 0.0])
    assert c.halfspace_build(hs, 0.11 ** 2).size == 49 and c.halfspace_build(hs, 0.09 ** 2).size == 0  # the plane is still 0.1 under the bar
    c.close()
