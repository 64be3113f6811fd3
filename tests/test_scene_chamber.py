"""The shape-line keyword `pressure <p> [ramp <seconds>]` of a scene (this project's keyword, not the reference's): what it parses to on shell and
tetrahedral shapes, where it is refused, the flip of an inward list, the open surface, the ramp, and what the backend receives (a recording stub: no GPU).
A scene without it never calls set_chambers."""
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
    write_obj(tmp_path / "inward.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI[:, ::-1])
    write_obj(tmp_path / "open.obj", cm.CUBE_X * 0.1, cm.CUBE_TRI[:-1])
    twisted = cm.CUBE_TRI.copy()
    twisted[3] = twisted[3][::-1]
    write_obj(tmp_path / "twisted.obj", cm.CUBE_X * 0.1, twisted)
    (tmp_path / "chain.seg").write_text("v 0 0 0\nv 0.1 0 0\ns 1 2\n")
    return str(tmp_path)


def scene_text(*shape_lines, tail=""):
    return f"shapes input {len(shape_lines)}\n" + "".join(line + "\n" for line in shape_lines) + f"density 500\nstiffness 2e5 0.35\ntime 1 0.05\n{tail}\n"


BAR = scene.make_bar(2, 1, 1, size=(2.0, 1.0, 1.0))


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    sc = ss.assemble(cfg, lambda p: (BAR[0].copy(), BAR[1].copy(), scene.surface_tris(BAR[1])))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def volume(V, tri):
    return cm.rest_volume(V, tri, cm.ref_point(V, tri))


def test_keyword_parses_on_shell_and_tetrahedral_shapes(folder):
    cfg = ss.SceneConfig.parse(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 40", "bar.msh 1 0 0  0 0 0  1 1 1 pressure -2.5e3 ramp 0.2",
                                          "cube.obj 3 0 0  0 0 0  1 1 1 pressure 7 ramp 1 shell 0.002 bend 0.5", "bar.msh 5 0 0  0 0 0  1 1 1"), folder)
    assert [(s.pressure, s.pressure_ramp) for s in cfg.shapes] == [(40.0, 0.0), (-2500.0, 0.2), (7.0, 1.0), (None, 0.0)]
    assert cfg.shapes[2].shell_thickness == 0.002 and cfg.shapes[2].shell_bend == 0.5  # the keywords of a shape line come in any order
    for bad in ("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure", "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure nan",
                "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure inf", "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 5 ramp",
                "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 5 ramp 0", "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 5 ramp -1",
                "cube.obj 0 0 0  0 0 0  1 1 1 pressure 5",  # a kinematic triangle mesh: no shell
                "chain.seg 0 0 0  0 0 0  1 1 1 rod 0.002 pressure 5"):
        with pytest.raises(ValueError) as e:
            ss.SceneConfig.parse(scene_text(bad), folder)
        assert not isinstance(e.value, ss.UnsupportedKeyword), bad


def test_shell_and_tetrahedral_shape_reach_set_chambers_once_behind_set_shell(folder):
    cfg, sc, calls = run(scene_text("bar.msh 0 0 0  0 0 0  1 1 1", "cube.obj 3 0 0  0 0 0  1 1 1 shell 0.001 pressure 40 ramp 0.2",
                                    "bar.msh 6 0 0  0 0 0  1 1 1 pressure -300"), folder)
    names = [c[0] for c in calls]
    assert names.count("set_chambers") == 1
    assert names.index("set_mesh") < names.index("set_shell") < names.index("set_chambers") < names.index("opt_init")
    (lists, p), = [a for nm, a, _ in calls if nm == "set_chambers"]
    nBar = len(BAR[0])
    assert sc.chambers is not None and set(sc.chambers) == {"tri_lists", "pressure", "ramp"}  # the dictionary handed on
    assert lists is sc.chambers["tri_lists"] and p is sc.chambers["pressure"]
    assert p.tolist() == [40.0, -300.0] and sc.chambers["ramp"].tolist() == [0.2, 0.0] and len(lists) == 2
    # chamber 0: the shell's own triangles (shape 1: global ids behind the first bar), as the shell got them
    shellTri, = [a[0] for nm, a, _ in calls if nm == "set_shell"]
    assert lists[0].dtype == np.int32 and np.array_equal(lists[0], cm.CUBE_TRI + nBar) and np.array_equal(shellTri, lists[0])
    # chamber 1: the boundary faces of the second bar's tetrahedra (shape 2)
    skin = scene.surface_tris(BAR[1]) + nBar + 8
    assert np.array_equal(np.sort(np.sort(lists[1], axis=1), axis=0), np.sort(np.sort(skin, axis=1), axis=0))
    for t in lists:  # closed and outward in the assembled mesh
        assert volume(sc.V, t) > 0
        e = np.vstack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        assert sorted(map(tuple, e)) == sorted(map(tuple, e[:, ::-1]))  # every directed edge has its opposite
    assert abs(volume(sc.V, lists[0]) - 1e-3) <= 1e-15 and abs(volume(sc.V, lists[1]) - 2.0) <= 1e-12


def test_inward_list_is_flipped_in_the_chambers_copy_only(folder):
    _, sc, calls = run(scene_text("inward.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 40"), folder)
    (lists, p), = [a for nm, a, _ in calls if nm == "set_chambers"]
    shellTri, = [a[0] for nm, a, _ in calls if nm == "set_shell"]
    assert np.array_equal(shellTri, cm.CUBE_TRI[:, ::-1])  # the shell keeps the file's orientation
    assert np.array_equal(lists[0], cm.CUBE_TRI) and volume(sc.V, lists[0]) > 0 > volume(sc.V, shellTri)
    assert np.array_equal(sc.SF, cm.CUBE_TRI[:, ::-1])  # ... and so does the contact surface
    # a mirroring scale turns an outward file inward: the orientation is judged on the transformed shape
    _, sc, calls = run(scene_text("cube.obj 0 0 0  0 0 0  -1 1 1 shell 0.001 pressure 40"), folder)
    (lists, p), = [a for nm, a, _ in calls if nm == "set_chambers"]
    assert np.array_equal(lists[0], cm.CUBE_TRI[:, ::-1]) and volume(sc.V, lists[0]) > 0


def test_open_or_inconsistent_surface_is_refused_by_name(folder):
    with pytest.raises(ValueError, match=r"shape 1 \(open\.obj\).*open"):
        run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 1", "open.obj 1 0 0  0 0 0  1 1 1 shell 0.001 pressure 40"), folder)
    with pytest.raises(ValueError, match=r"shape 0 \(twisted\.obj\).*same direction"):
        run(scene_text("twisted.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 40"), folder)
    run(scene_text("open.obj 1 0 0  0 0 0  1 1 1 shell 0.001"), folder)  # without the keyword an open shell is fine


def test_ramp_schedule(folder):
    _, sc, _ = run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 40 ramp 0.2", "bar.msh 6 0 0  0 0 0  1 1 1 pressure -300",
                              "cube.obj 3 0 0  0 0 0  1 1 1 shell 0.001 pressure -8 ramp 1"), folder)
    assert sc.chamber_pressures(0.0).tolist() == [0.0, -300.0, 0.0]
    assert sc.chamber_pressures(0.05).tolist() == [40.0 * (0.05 / 0.2), -300.0, -8.0 * 0.05]
    assert sc.chamber_pressures(0.2).tolist() == [40.0, -300.0, -8.0 * 0.2]
    assert sc.chamber_pressures(7.0).tolist() == [40.0, -300.0, -8.0]
    _, sc, _ = run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 pressure 40"), folder)
    assert sc.chamber_pressures(0.1) is None  # no ramp: nothing to set between the steps


def test_a_scene_without_the_keyword_never_calls_set_chambers(folder):
    _, sc, calls = run(scene_text("cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001", "bar.msh 6 0 0  0 0 0  1 1 1"), folder)
    assert "set_chambers" not in [c[0] for c in calls] and sc.chambers is None and sc.chamber_pressures(0.1) is None
