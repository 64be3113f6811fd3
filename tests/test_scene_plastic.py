"""The shape-line keyword `plastic <yield> [creep <rate>] [harden <K>]` of a scene (this project's keyword, not the reference's): what it parses to, the
defaults, where it is refused, and what the backend receives (a recording stub: no GPU).  A scene without it never calls set_plasticity and assembles as
before."""
import math

import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

import chamber_mp as cm
from test_scene_aero import AT, BAR, Recorder, run, scene_text, write_obj


@pytest.fixture()
def folder(tmp_path):
    write_obj(tmp_path / "cube.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI)
    (tmp_path / "chain.seg").write_text("v 0 0 0\nv 0.1 0 0\ns 1 2\n")
    return str(tmp_path)


def test_keyword_parses_with_its_defaults():
    cfg = ss.SceneConfig.parse(scene_text(f"bar.msh {AT} plastic 0.05", f"bar.msh {AT} plastic 0 creep 2.5", f"bar.msh {AT} material 800 1e5 0.3 plastic 1e-2 harden 0.5 creep 10",
                                          f"bar.msh {AT}", f"bar.msh {AT} plastic 0.02 harden 3 contactGroup 2"), ".")
    assert [s.plastic for s in cfg.shapes] == [(0.05, math.inf, 0.0), (0.0, 2.5, 0.0), (0.01, 10.0, 0.5), None, (0.02, math.inf, 3.0)]
    assert cfg.shapes[2].material == (800.0, 1e5, 0.3) and cfg.shapes[4].contact_group == 2  # the keywords of a shape line come in any order


def test_malformed_and_misplaced_tokens_are_value_errors():
    for bad in (f"bar.msh {AT} plastic", f"bar.msh {AT} plastic -0.1", f"bar.msh {AT} plastic nan", f"bar.msh {AT} plastic 0.05 creep", f"bar.msh {AT} plastic 0.05 creep 0",
                f"bar.msh {AT} plastic 0.05 creep -1", f"bar.msh {AT} plastic 0.05 harden", f"bar.msh {AT} plastic 0.05 harden -2", f"bar.msh {AT} plastic 0.05 harden inf",
                f"bar.msh {AT} plastic 0.05 harden nan", f"bar.msh {AT} plastic creep 2",  # no yield strain
                f"bar.msh {AT} creep 2",  # a parameter without plastic in front of it
                f"cube.obj {AT} shell 0.001 plastic 0.05",  # a shell
                f"cube.obj {AT} plastic 0.05",  # a surface-only shape
                f"chain.seg {AT} rod 0.002 plastic 0.05"):  # a rod
        with pytest.raises(ValueError) as e:
            ss.SceneConfig.parse(scene_text(bad), ".")
        assert not isinstance(e.value, ss.UnsupportedKeyword) or "creep" in str(e.value), bad


def test_plastic_shapes_reach_set_plasticity_per_component_behind_the_materials(folder):
    cfg, sc, calls = run(scene_text("bar.msh 0 0 0  0 0 0  1 1 1 plastic 0.05 creep 4", "bar.msh 3 0 0  0 0 0  1 1 1 material 800 1e5 0.3",
                                    "bar.msh 6 0 0  0 0 0  1 1 1 material 900 2e5 0.3 plastic 0.01 harden 0.5"), folder)
    names = [c[0] for c in calls]
    nT = len(BAR[1])
    got = [a for nm, a, _ in calls if nm == "set_plasticity"]
    assert got == [((0, nT), 0.05, 4.0, 0.0), ((2 * nT, 3 * nT), 0.01, math.inf, 0.5)]
    last_material = max(i for i, nm in enumerate(names) if nm == "set_component_material")
    assert names.index("set_mesh") < last_material < names.index("set_plasticity") < names.index("opt_init")


def test_a_scene_without_the_keyword_is_what_it_was(folder):
    lines = ("bar.msh 0 0 0  0 0 0  1 1 1", "bar.msh 3 0 0  0 0 0  1 1 1 material 800 1e5 0.3")
    _, sc0, calls0 = run(scene_text(*lines), folder)
    assert "set_plasticity" not in [c[0] for c in calls0]
    _, sc1, calls1 = run(scene_text(lines[0] + " plastic 0.05", lines[1]), folder)
    rest = [c for c in calls1 if c[0] != "set_plasticity"]
    assert [c[0] for c in rest] == [c[0] for c in calls0] and len(calls1) == len(calls0) + 1
    for (_, a0, k0), (_, a1, k1) in zip(calls0, rest):  # every other call carries the same arguments
        assert len(a0) == len(a1) and k0.keys() == k1.keys()
        for x, y in zip(list(a0) + list(k0.values()), list(a1) + list(k1.values())):
            assert np.array_equal(np.asarray(x, dtype=object), np.asarray(y, dtype=object)) if not isinstance(x, np.ndarray) else np.array_equal(x, y)
    assert np.array_equal(sc0.V, sc1.V) and np.array_equal(sc0.T, sc1.T)
