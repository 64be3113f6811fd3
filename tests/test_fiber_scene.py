"""The shape-line keyword `fiber <k> dir <x> <y> <z> [exp <k2>] [tensiononly] [activate <act> [ramp <seconds>]]` of a scene (this project's keyword, not the
reference's): what it parses to, where it is refused, how `dir` turns with the shape line's rotation, the ramp schedule tools/run_scene.py follows, and what
the backend receives (a recording stub: no GPU).  A scene without it never calls set_fibers."""
import numpy as np
import pytest

from ipc_amd import scene_script as ss

import chamber_mp as cm
from test_scene_aero import AT, BAR, run, scene_text, write_obj


@pytest.fixture()
def folder(tmp_path):
    write_obj(tmp_path / "cube.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI)
    (tmp_path / "chain.seg").write_text("v 0 0 0\nv 0.1 0 0\ns 1 2\n")
    return str(tmp_path)


def test_keyword_parses_with_its_defaults():
    cfg = ss.SceneConfig.parse(scene_text(f"bar.msh {AT} fiber 5e4 dir 1 0 0", f"bar.msh {AT} fiber 2e4 dir 0 1 1 exp 3.5", f"bar.msh {AT} fiber 1e4 dir 0 0 2 tensiononly activate 0.3 ramp 0.5",
                                          f"bar.msh {AT}", f"bar.msh {AT} material 800 1e5 0.3 fiber 1e3 dir 1 1 0 activate -0.2 contactGroup 2"), ".")
    f = [s.fiber for s in cfg.shapes]
    assert f[0] == {"k": 5e4, "dir": (1.0, 0.0, 0.0), "law": "spring", "k2": 0.0, "tension_only": False, "act": 0.0, "ramp": 0.0}
    assert f[1]["law"] == "exp" and f[1]["k2"] == 3.5 and f[1]["dir"] == (0.0, 1.0, 1.0)
    assert f[2]["tension_only"] and f[2]["act"] == 0.3 and f[2]["ramp"] == 0.5 and f[3] is None
    assert f[4]["act"] == -0.2 and f[4]["ramp"] == 0.0 and cfg.shapes[4].contact_group == 2 and cfg.shapes[4].material == (800.0, 1e5, 0.3)


def test_malformed_and_misplaced_tokens_are_value_errors():
    """each refusal by its own message (an unknown keyword raises a ValueError too: the message tells the new refusals from that)"""
    B = f"bar.msh {AT} fiber"
    for bad, msg in ((B, "fiber needs <k> dir"), (f"{B} 5e4", "fiber needs <k> dir"), (f"{B} 5e4 dir 1 0", "fiber needs <k> dir"), (f"{B} 5e4 1 0 0 0", "fiber needs <k> dir"),
                     (f"{B} 0 dir 1 0 0", "positive, finite stiffness"), (f"{B} -1 dir 1 0 0", "positive, finite stiffness"), (f"{B} nan dir 1 0 0", "positive, finite stiffness"),
                     (f"{B} 5e4 dir 0 0 0", "direction that is not zero"), (f"{B} 5e4 dir inf 0 0", "finite direction"),
                     (f"{B} 5e4 dir 1 0 0 exp", "exp needs a number"), (f"{B} 5e4 dir 1 0 0 exp 0", "exp needs a positive, finite k2"), (f"{B} 5e4 dir 1 0 0 exp -1", "exp needs a positive, finite k2"),
                     (f"{B} 5e4 dir 1 0 0 activate", "activate needs a number"), (f"{B} 5e4 dir 1 0 0 activate 1", "activation below 1"), (f"{B} 5e4 dir 1 0 0 activate 1.5", "activation below 1"),
                     (f"{B} 5e4 dir 1 0 0 activate 0.3 ramp", "ramp needs a time"), (f"{B} 5e4 dir 1 0 0 activate 0.3 ramp 0", "ramp needs a positive, finite time"),
                     (f"{B} 5e4 dir 1 0 0 activate 0.3 ramp -1", "ramp needs a positive, finite time"),
                     (f"{B} 5e4 dir 1 0 0 exp 2 activate 0.3", "activate is not defined for exp fibres"),
                     (f"{B} 5e4 dir 1 0 0 plastic 0.05", "fiber and plastic exclude each other"),
                     (f"cube.obj {AT} shell 0.001 fiber 5e4 dir 1 0 0", "fiber is valid on a tetrahedral shape only"),
                     (f"cube.obj {AT} fiber 5e4 dir 1 0 0", "fiber is valid on a tetrahedral shape only"),
                     (f"chain.seg {AT} rod 0.002 fiber 5e4 dir 1 0 0", "fiber is valid on a tetrahedral shape only")):
        with pytest.raises(ValueError, match=msg):
            ss.SceneConfig.parse(scene_text(bad), ".")
    with pytest.raises(ValueError, match="fiber needs <k> dir"):
        ss.SceneConfig.parse(scene_text(f"{B} 5e4 1 0 0"), ".")
    with pytest.raises(ss.UnsupportedKeyword):
        ss.SceneConfig.parse(scene_text(f"{B} 5e4 dir 1 0 0 ramp 2"), ".")  # a ramp without activate in front of it is no keyword of a shape


def test_dir_turns_with_the_shape_and_every_fibred_shape_gets_its_group(folder):
    cfg, sc, calls = run(scene_text("bar.msh 0 0 0  0 0 90  1 1 1 fiber 5e4 dir 1 0 0 activate 0.25", "bar.msh 3 0 0  0 0 0  1 1 1 material 800 1e5 0.3",
                                    "bar.msh 6 0 0  30 -40 70  1 2 1 fiber 2e4 dir 0.3 -0.5 0.8 exp 2 ", "bar.msh 9 0 0  0 0 0  1 1 1 fiber 1e4 dir 0 1 0 tensiononly activate 0.3 ramp 0.4"), folder)
    nT = len(BAR[1])
    got = [(a, k) for nm, a, k in calls if nm == "set_fibers"]
    assert [a[0] for a, _ in got] == [(0, nT), (2 * nT, 3 * nT), (3 * nT, 4 * nT)] and [k["group"] for _, k in got] == [0, 1, 2]
    assert np.allclose(got[0][0][1], ss._rot((0, 0, 90)) @ [1.0, 0.0, 0.0], atol=1e-15) and np.allclose(got[0][0][1], [0.0, 1.0, 0.0], atol=1e-15)
    # a material line of the mesh file: the image of p + t dir under p -> R (p * scale) + translate runs along R (dir * scale)
    d = ss._rot((30, -40, 70)) @ (np.array([0.3, -0.5, 0.8]) * [1, 2, 1])
    assert np.allclose(got[1][0][1], d / np.linalg.norm(d), atol=1e-15) and got[1][1]["law"] == "exp" and got[1][1]["k2"] == 2.0
    assert got[2][1]["tension_only"] and not got[0][1]["tension_only"] and [a[2] for a, _ in got] == [5e4, 2e4, 1e4]
    names = [c[0] for c in calls]
    last_material = max(i for i, nm in enumerate(names) if nm == "set_component_material")
    assert names.index("set_mesh") < last_material < names.index("set_fibers") < names.index("opt_init")
    # an activation without a ramp is set once by apply(); a ramped one starts at 0 and is left to the run
    assert [a for nm, a, _ in calls if nm == "fiber_set_activation"] == [(0, 0.25)]
    # the ramp schedule: act min(1, t / ramp) for the time at which the step ends
    assert sc.fiber_activations(0.1) == [(2, 0.3 * 0.25)] and sc.fiber_activations(0.4) == [(2, 0.3)] and sc.fiber_activations(7.0) == [(2, 0.3)]
    assert sc.fiber_activations(0.2)[0][1] == 0.3 * min(1.0, 0.2 / 0.4)


def test_a_scene_without_the_keyword_is_what_it_was(folder):
    lines = ("bar.msh 0 0 0  0 0 0  1 1 1", "bar.msh 3 0 0  0 0 0  1 1 1 material 800 1e5 0.3")
    _, sc0, calls0 = run(scene_text(*lines), folder)
    assert "set_fibers" not in [c[0] for c in calls0] and sc0.fibers is None and sc0.fiber_activations(1.0) is None
    _, sc1, calls1 = run(scene_text(lines[0] + " fiber 5e4 dir 1 0 0", lines[1]), folder)
    rest = [c for c in calls1 if c[0] != "set_fibers"]
    assert [c[0] for c in rest] == [c[0] for c in calls0] and len(calls1) == len(calls0) + 1 and sc1.fiber_activations(1.0) is None
    assert np.array_equal(sc0.V, sc1.V) and np.array_equal(sc0.T, sc1.T)
