"""The `rod <radius> [bend <scale>]` keyword of a shape line (this project's keyword, not the reference's): what it parses to, where it is refused, and what
the backend receives (a recording stub: no GPU).  A segment shape without the keyword behaves as before."""
import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

import rod_mp as rmp


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


@pytest.fixture()
def rod(tmp_path):
    V, seg = rmp.chain(6)
    p = tmp_path / "rod.seg"
    p.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in V) + "".join(f"s {a + 1} {b + 1}\n" for a, b in seg))
    return str(tmp_path), V, seg


def scene_text(tail):
    return f"shapes input 1\nrod.seg 0 1 0  0 0 0  1 1 1 {tail}\ndensity 500\nstiffness 2e5 0.35\nselfCollisionOn\n"


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    Vb, Tb = scene.make_bar(1, 1, 1, size=(1.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (Vb.copy(), Tb.copy(), scene.surface_tris(Tb)))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_keyword_parses_with_and_without_bend(rod):
    folder = rod[0]
    a = ss.SceneConfig.parse(scene_text("rod 0.002"), folder).shapes[0]
    assert a.rod_radius == 0.002 and a.rod_bend == 1.0
    b = ss.SceneConfig.parse(scene_text("material 900 1e6 0.3 rod 0.001 bend 10 contactGroup 2"), folder).shapes[0]
    assert b.rod_radius == 0.001 and b.rod_bend == 10.0 and b.contact_group == 2 and b.material == (900.0, 1e6, 0.3)
    assert ss.SceneConfig.parse(scene_text("rod 0.001 bend 0"), folder).shapes[0].rod_bend == 0.0  # bending switched off
    for bad in ("rod", "rod 0", "rod -1", "rod 0.01 bend", "rod 0.01 bend -2"):
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), folder)


@pytest.mark.parametrize("path", ["cloth.obj", "bar.msh", "dot.pt"])
def test_keyword_on_another_kind_of_shape_is_a_value_error(path):
    with pytest.raises(ValueError) as e:
        ss.SceneConfig.parse(f"shapes input 1\n{path} 0 0 0  0 0 0  1 1 1 rod 0.01\n", "/x")
    assert not isinstance(e.value, ss.UnsupportedKeyword) and "segment shape" in str(e.value)


def test_shell_on_a_segment_shape_stays_a_value_error():
    with pytest.raises(ValueError, match="triangle-mesh"):
        ss.SceneConfig.parse("shapes input 1\nrod.seg 0 0 0  0 0 0  1 1 1 shell 0.01\n", "/x")


def test_free_rod_assembles_and_reaches_set_rod(rod):
    folder, V, seg = rod
    cfg, sc, calls = run(scene_text("rod 0.002 bend 3"), folder)
    names = [n for n, _, _ in calls]
    assert names.count("set_rod") == 1 and "set_shell" not in names
    assert names.index("set_mesh") < names.index("set_codim_nodes") < names.index("set_rod") < names.index("opt_init") < names.index("set_surface")
    (s, r, E, rho, bend), = [a for n, a, _ in calls if n == "set_rod"]
    assert np.array_equal(s, seg) and bend == 3.0
    assert np.all(r == 0.002) and np.all(E == 2e5) and np.all(rho == 500.0) and len(r) == len(seg)
    assert sc.dirichlet == []  # nobody holds it
    assert sc.T.shape[0] == 0 and np.array_equal(sc.codim_edges, seg)
    (sf, ce), = [a for n, a, _ in calls if n == "set_surface"]  # collision still gets the segments
    assert np.array_equal(ce, seg) and len(sf) == 0
    # the shape's own material wins over the scene's (Poisson's ratio is unused)
    _, _, calls = run(scene_text("material 900 1e6 0.3 rod 0.002"), folder)
    (s, r, E, rho, bend), = [a for n, a, _ in calls if n == "set_rod"]
    assert np.all(E == 1e6) and np.all(rho == 900.0) and bend == 1.0
    # ... and reaches set_rod ONLY: set_component_material would scale the masses set_rod has just set by rho / density once more
    assert "set_component_material" not in [n for n, _, _ in calls]


def test_rod_after_shell_in_the_call_order(rod, tmp_path):
    Vg = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.0]])
    (tmp_path / "tri.obj").write_text("".join(f"v {a} {b} {c}\n" for a, b, c in Vg) + "f 1 2 3\n")
    text = ("shapes input 2\ntri.obj 0 3 0  0 0 0  1 1 1 shell 0.002\nrod.seg 0 1 0  0 0 0  1 1 1 rod 0.002 material 900 1e6 0.3\n"
            "density 500\nstiffness 2e5 0.35\n")
    _, sc, calls = run(text, rod[0])
    names = [n for n, _, _ in calls]
    assert names.index("set_codim_nodes") < names.index("set_shell") < names.index("set_rod") < names.index("opt_init")
    assert sc.rod["seg"].min() == sc.node_ranges[1] and np.all(sc.rod["rho"] == 900.0) and np.all(sc.shell["rho"] == 500.0)


def test_different_bend_scales_are_refused(rod):
    text = "shapes input 2\nrod.seg 0 0 0  0 0 0  1 1 1 rod 0.002 bend 2\nrod.seg 0 2 0  0 0 0  1 1 1 rod 0.002 bend 3\n"
    with pytest.raises(ValueError, match="one bend scale per scene"):
        run(text, rod[0])


def test_partly_held_rod_keeps_its_dirichlet_box(rod):
    folder, V, seg = rod
    _, sc, calls = run(scene_text("rod 0.002 DBC 0 0 0  0.1 1 1  0 0 0  0 0 0"), folder)
    assert len(sc.dirichlet) == 1 and 0 < len(sc.dirichlet[0][0]) < len(V)
    assert [n for n, _, _ in calls].count("set_rod") == 1


def test_the_same_scene_without_the_keyword_is_still_refused(rod):
    with pytest.raises(ss.UnsupportedKeyword, match="codimensional shape that no script fixes or moves"):
        run(scene_text(""), rod[0])


def test_a_held_segment_shape_without_the_keyword_never_calls_set_rod(rod):
    _, sc, calls = run(scene_text("linearVelocity 0 0 0"), rod[0])
    assert "set_rod" not in [n for n, _, _ in calls] and sc.rod is None
