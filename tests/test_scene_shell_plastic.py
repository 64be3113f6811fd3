"""The keyword `yield <y> [bendyield <yb>] [creep <rate>] [harden <K>]` inside the `shell` clause of a shape line (this project's keyword, not the reference's):
what it parses to, the defaults, where it is refused, and what the backend receives (a recording stub: no GPU).  A scene without it never calls
shell_set_plasticity."""
import math

import numpy as np
import pytest

from ipc_amd import scene_script as ss

import chamber_mp as cm
from test_scene_aero import AT, Recorder, run, scene_text, write_obj  # noqa: F401


@pytest.fixture()
def folder(tmp_path):
    write_obj(tmp_path / "cube.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI)
    write_obj(tmp_path / "open.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI[:-3])
    return str(tmp_path)


def test_keyword_parses_with_its_defaults():
    cfg = ss.SceneConfig.parse(scene_text(f"cube.obj {AT} shell 0.001 yield 0.01", f"cube.obj {AT} shell 0.002 bend 0.5 yield 0 bendyield 0.003 creep 2.5 harden 0.5",
                                          f"cube.obj {AT} shell 0.001 limit 1.2 onset 1.05 yield 0.02 harden 3 contactGroup 2", f"cube.obj {AT} shell 0.001",
                                          f"cube.obj {AT} material 800 1e5 0.3 shell 0.001 yield inf bendyield 0.004"), ".")
    assert [s.shell_plastic for s in cfg.shapes] == [(0.01, 0.01, math.inf, 0.0), (0.0, 0.003, 2.5, 0.5), (0.02, 0.02, math.inf, 3.0), None, (math.inf, 0.004, math.inf, 0.0)]
    assert cfg.shapes[1].shell_bend == 0.5 and cfg.shapes[2].shell_limit == 1.2 and cfg.shapes[2].shell_onset == 1.05 and cfg.shapes[2].contact_group == 2
    assert cfg.shapes[4].material == (800.0, 1e5, 0.3)


def test_malformed_and_misplaced_tokens_are_value_errors():
    for bad in (f"cube.obj {AT} shell 0.001 yield", f"cube.obj {AT} shell 0.001 yield -0.1", f"cube.obj {AT} shell 0.001 yield nan", f"cube.obj {AT} shell 0.001 yield 0.01 bendyield",
                f"cube.obj {AT} shell 0.001 yield 0.01 bendyield -1", f"cube.obj {AT} shell 0.001 yield 0.01 creep 0", f"cube.obj {AT} shell 0.001 yield 0.01 creep -1",
                f"cube.obj {AT} shell 0.001 yield 0.01 harden -2", f"cube.obj {AT} shell 0.001 yield 0.01 harden inf", f"cube.obj {AT} shell 0.001 yield 0.01 harden nan",
                f"cube.obj {AT} shell 0.001 bendyield 0.01",  # a parameter without yield in front of it
                f"cube.obj {AT} shell 0.001 creep 2",
                f"cube.obj {AT} shell 0.001 yield 0.01 creep 2 bendyield 0.02",  # the parameters come in their order
                f"cube.obj {AT} shell 0.001 yield 0.01 limit 1.2",  # yield comes behind the limit group
                f"cube.obj {AT} shell 0.001 yield 0.01 bend 0.5",
                f"cube.obj {AT} shell 0.001 rubber yield 0.01",  # a rubber membrane has no plastic flow
                f"cube.obj {AT} shell 0.001 rubber mr 0.2 limit 1.5 yield 0.01",
                f"cube.obj {AT} yield 0.01",  # no shell clause in front of it
                f"bar.msh {AT} yield 0.01",
                f"cube.obj {AT} shell 0.001 plastic 0.05"):  # the tetrahedra's keyword stays refused on a shell
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), ".")


def test_plastic_shell_shapes_reach_shell_set_plasticity_with_their_triangle_range(folder):
    cfg, sc, calls = run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 yield 0.01 creep 4", "open.obj 3 0 0  0 0 0  1 1 1 shell 0.001",
                                    "cube.obj 6 0 0  0 0 0  1 1 1 shell 0.001 limit 1.3 yield 0.02 bendyield 0.005 harden 0.5", "bar.msh 9 0 0  0 0 0  1 1 1"), folder)
    names = [c[0] for c in calls]
    n0, n1 = len(cm.CUBE_TRI), len(cm.CUBE_TRI) - 3
    got = [a for nm, a, _ in calls if nm == "shell_set_plasticity"]
    assert got == [((0, n0), 0.01, 0.01, 4.0, 0.0), ((n0 + n1, 2 * n0 + n1), 0.02, 0.005, math.inf, 0.5)]
    assert len(next(a for nm, a, _ in calls if nm == "set_shell")[0]) == 2 * n0 + n1
    assert names.index("set_shell") < names.index("set_shell_strain_limit") < names.index("shell_set_plasticity") < names.index("opt_init")
    assert "set_plasticity" not in names


def test_a_scene_without_the_keyword_is_what_it_was(folder):
    lines = ("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001", "bar.msh 3 0 0  0 0 0  1 1 1")
    _, sc0, calls0 = run(scene_text(*lines), folder)
    assert "shell_set_plasticity" not in [c[0] for c in calls0]
    _, sc1, calls1 = run(scene_text(lines[0] + " yield 0.01", lines[1]), folder)
    rest = [c for c in calls1 if c[0] != "shell_set_plasticity"]
    assert [c[0] for c in rest] == [c[0] for c in calls0] and len(calls1) == len(calls0) + 1
    assert np.array_equal(sc0.V, sc1.V) and np.array_equal(sc0.shell["tri"], sc1.shell["tri"])
