"""The top-level line `wind <wx> <wy> <wz> [density <rho>]` and the shape-line keyword `aero [cn <C>] [ct <C>] [onesided]` of a scene (this project's
keywords, not the reference's): what they parse to on shell and tetrahedral shapes, the defaults, where they are refused, the outward faces of a solid, and
what the backend receives (a recording stub: no GPU).  A scene without them never calls set_aero."""
import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

import chamber_mp as cm


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


def write_obj(path, V, tri):
    path.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in V) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in tri))


@pytest.fixture()
def folder(tmp_path):
    write_obj(tmp_path / "cube.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI)
    write_obj(tmp_path / "open.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI[:-3])
    (tmp_path / "chain.seg").write_text("v 0 0 0\nv 0.1 0 0\ns 1 2\n")
    return str(tmp_path)


def scene_text(*shape_lines, tail=""):
    return f"shapes input {len(shape_lines)}\n" + "".join(line + "\n" for line in shape_lines) + f"density 500\nstiffness 2e5 0.35\ntime 1 0.05\n{tail}\n"


BAR = scene.make_bar(2, 1, 1, size=(2.0, 1.0, 1.0))
AT = "0 0 0  0 0 0  1 1 1"


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    sc = ss.assemble(cfg, lambda p: (BAR[0].copy(), BAR[1].copy(), scene.surface_tris(BAR[1])))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_keywords_parse_with_their_defaults():
    cfg = ss.SceneConfig.parse(scene_text(f"cube.obj {AT} shell 0.001 aero", f"bar.msh {AT} aero cn 0.9 ct 0.05", f"cube.obj {AT} aero onesided ct 0.3 shell 0.002 bend 0.5",
                                          f"bar.msh {AT}", f"open.obj {AT} shell 0.001 aero cn 2 onesided", tail="wind 1 -2.5 3e-1 density 1.1"), ".")
    assert [(s.aero, s.aero_cn, s.aero_ct, s.aero_onesided) for s in cfg.shapes] == [(True, 1.28, 0.0, False), (True, 0.9, 0.05, True), (True, 1.28, 0.3, True),
                                                                                       (False, 1.28, 0.0, False), (True, 2.0, 0.0, True)]
    assert cfg.shapes[2].shell_thickness == 0.002 and cfg.shapes[2].shell_bend == 0.5  # the keywords of a shape line come in any order
    assert cfg.wind == (1.0, -2.5, 0.3) and cfg.air_density == 1.1
    cfg = ss.SceneConfig.parse(scene_text(f"cube.obj {AT} shell 0.001 aero", tail="wind 0 0 4"), ".")
    assert cfg.wind == (0.0, 0.0, 4.0) and cfg.air_density == 1.225
    cfg = ss.SceneConfig.parse(scene_text(f"cube.obj {AT} shell 0.001 aero"), ".")
    assert cfg.wind == (0.0, 0.0, 0.0) and cfg.air_density == 1.225  # still air


def test_malformed_and_misplaced_tokens_are_value_errors():
    for bad in (f"cube.obj {AT} shell 0.001 aero cn", f"cube.obj {AT} shell 0.001 aero cn -1", f"cube.obj {AT} shell 0.001 aero ct nan", f"cube.obj {AT} shell 0.001 aero cn inf",
                f"cube.obj {AT} shell 0.001 aero ct",
                f"cube.obj {AT} shell 0.001 cn 1.0",  # a coefficient without aero in front of it
                f"cube.obj {AT} shell 0.001 onesided", f"cube.obj {AT} shell 0.001 aero shell 0.002 ct 0.2",  # ... or behind another keyword
                f"cube.obj {AT} aero",  # a kinematic triangle mesh: no shell
                f"chain.seg {AT} rod 0.002 aero"):
        with pytest.raises(ValueError) as e:
            ss.SceneConfig.parse(scene_text(bad), ".")
        assert not isinstance(e.value, ss.UnsupportedKeyword), bad
    for tail in ("wind 1 2", "wind 1 2 3 4", "wind 1 2 3 density", "wind 1 2 3 rho 1.2", "wind 1 2 nan", "wind 1 inf 3", "wind 1 2 3 density 0", "wind 1 2 3 density -1",
                 "wind 1 2 3 density inf"):
        with pytest.raises(ValueError) as e:
            ss.SceneConfig.parse(scene_text(f"cube.obj {AT} shell 0.001 aero", tail=tail), ".")
        assert not isinstance(e.value, ss.UnsupportedKeyword), tail


def test_shell_and_tetrahedral_shape_reach_set_aero_once_and_the_wind_follows(folder):
    cfg, sc, calls = run(scene_text("bar.msh 0 0 0  0 0 0  1 1 1", "cube.obj 3 0 0  0 0 0  1 1 1 shell 0.001 aero ct 0.1", "bar.msh 6 0 0  0 0 0  1 1 1 aero cn 0.8",
                                    "open.obj 9 0 0  0 0 0  1 1 1 shell 0.001 aero onesided", tail="wind 2 0 -1 density 1.3"), folder)
    names = [c[0] for c in calls]
    assert names.count("set_aero") == 1 and names.count("aero_set_wind") == 1
    assert names.index("set_mesh") < names.index("set_shell") < names.index("set_aero") < names.index("aero_set_wind") < names.index("opt_init")
    (lists, cn, ct, one), = [a for nm, a, _ in calls if nm == "set_aero"]
    (wind, rho), = [a for nm, a, _ in calls if nm == "aero_set_wind"]
    assert wind == (2.0, 0.0, -1.0) and rho == 1.3
    assert sc.aero is not None and set(sc.aero) == {"tri_lists", "cn", "ct", "one_sided"} and lists is sc.aero["tri_lists"]
    assert cn.tolist() == [1.28, 0.8, 1.28] and ct.tolist() == [0.1, 0.0, 0.0] and one.tolist() == [False, True, True] and len(lists) == 3
    nBar = len(BAR[0])
    # surface 0: the shell's own triangles, as the shell got them (two-sided: the file's orientation stays)
    shellTri, = [a[0] for nm, a, _ in calls if nm == "set_shell"]
    assert lists[0].dtype == np.int32 and np.array_equal(lists[0], cm.CUBE_TRI + nBar) and np.array_equal(shellTri[:12], lists[0])
    # surface 1: the boundary faces of the second bar's tetrahedra, every one outward
    skin = scene.surface_tris(BAR[1]) + nBar + 8
    assert np.array_equal(np.sort(np.sort(lists[1], axis=1), axis=0), np.sort(np.sort(skin, axis=1), axis=0))
    centre = sc.V[np.unique(lists[1])].mean(axis=0)
    for t in lists[1]:
        assert np.cross(sc.V[t[1]] - sc.V[t[0]], sc.V[t[2]] - sc.V[t[0]]) @ (sc.V[t].mean(axis=0) - centre) > 0
    assert cm.rest_volume(sc.V, lists[1], cm.ref_point(sc.V, lists[1])) > 0
    # surface 2: an open shell is fine
    assert np.array_equal(lists[2], cm.CUBE_TRI[:-3] + nBar + 8 + nBar)


def test_a_mirrored_solid_still_faces_outward(folder):
    _, sc, calls = run(scene_text("bar.msh 0 0 0  0 0 0  -1 1 1 aero"), folder)
    (lists, cn, ct, one), = [a for nm, a, _ in calls if nm == "set_aero"]
    centre = sc.V.mean(axis=0)
    for t in lists[0]:
        assert np.cross(sc.V[t[1]] - sc.V[t[0]], sc.V[t[2]] - sc.V[t[0]]) @ (sc.V[t].mean(axis=0) - centre) > 0
    assert one.tolist() == [True]


def test_a_scene_without_the_keyword_never_calls_set_aero(folder):
    _, sc, calls = run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001", "bar.msh 6 0 0  0 0 0  1 1 1", tail="wind 1 2 3"), folder)
    names = [c[0] for c in calls]
    assert "set_aero" not in names and "aero_set_wind" not in names and sc.aero is None
