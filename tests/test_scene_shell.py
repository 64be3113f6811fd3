"""The `shell <thickness> [bend <scale>]` keyword of a shape line (this project's keyword, not the reference's): what it parses to, where it is refused, and
what the backend receives (a recording stub: no GPU).  A triangle shape without the keyword behaves as before."""
import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

import shell_mp as smp


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


@pytest.fixture()
def cloth(tmp_path):
    V, tri = smp.grid(4)
    p = tmp_path / "cloth.obj"
    p.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in V) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in tri))
    return str(tmp_path), V, tri


def scene_text(tail):
    return f"shapes input 1\ncloth.obj 0 1 0  0 0 0  1 1 1 {tail}\ndensity 500\nstiffness 2e5 0.35\nselfCollisionOn\n"


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    Vb, Tb = scene.make_bar(1, 1, 1, size=(1.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (Vb.copy(), Tb.copy(), scene.surface_tris(Tb)))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_keyword_parses_with_and_without_bend(cloth):
    folder = cloth[0]
    a = ss.SceneConfig.parse(scene_text("shell 0.002"), folder).shapes[0]
    assert a.shell_thickness == 0.002 and a.shell_bend == 1.0
    b = ss.SceneConfig.parse(scene_text("material 900 1e6 0.3 shell 0.001 bend 10 contactGroup 2"), folder).shapes[0]
    assert b.shell_thickness == 0.001 and b.shell_bend == 10.0 and b.contact_group == 2 and b.material == (900.0, 1e6, 0.3)
    for bad in ("shell", "shell 0", "shell -1", "shell 0.01 bend", "shell 0.01 bend -2"):
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), folder)


@pytest.mark.parametrize("path", ["bar.msh", "rod.seg", "dot.pt"])
def test_keyword_on_another_kind_of_shape_is_a_value_error(path):
    with pytest.raises(ValueError) as e:
        ss.SceneConfig.parse(f"shapes input 1\n{path} 0 0 0  0 0 0  1 1 1 shell 0.01\n", "/x")
    assert not isinstance(e.value, ss.UnsupportedKeyword) and "triangle-mesh" in str(e.value)


def test_free_cloth_assembles_and_reaches_set_shell(cloth):
    folder, V, tri = cloth
    cfg, sc, calls = run(scene_text("shell 0.002 bend 3"), folder)
    names = [n for n, _, _ in calls]
    assert names.count("set_shell") == 1
    assert names.index("set_mesh") < names.index("set_codim_nodes") < names.index("set_shell") < names.index("opt_init") < names.index("set_surface")
    (t, h, E, nu, rho, bend), = [a for n, a, _ in calls if n == "set_shell"]
    assert np.array_equal(t, tri) and bend == 3.0
    assert np.all(h == 0.002) and np.all(E == 2e5) and np.all(nu == 0.35) and np.all(rho == 500.0) and len(h) == len(tri)
    assert sc.dirichlet == []  # nobody holds it
    assert sc.T.shape[0] == 0 and np.array_equal(sc.SF, tri)
    # the shape's own material wins over the scene's
    _, _, calls = run(scene_text("material 900 1e6 0.3 shell 0.002"), folder)
    (t, h, E, nu, rho, bend), = [a for n, a, _ in calls if n == "set_shell"]
    assert np.all(E == 1e6) and np.all(nu == 0.3) and np.all(rho == 900.0) and bend == 1.0
    # ... and reaches set_shell ONLY: set_component_material would scale the masses set_shell has just set by rho / density once more
    assert "set_component_material" not in [n for n, _, _ in calls]


def test_material_of_a_tet_shape_beside_the_cloth_still_reaches_set_component_material(cloth):
    text = ("shapes input 2\nbar.msh 0 0 0  0 0 0  1 1 1 material 2000 1e6 0.3\ncloth.obj 0 2 0  0 0 0  1 1 1 material 900 1e6 0.3 shell 0.002\n"
            "density 500\nstiffness 2e5 0.35\n")
    _, sc, calls = run(text, cloth[0])
    cm = [a for n, a, _ in calls if n == "set_component_material"]
    assert len(cm) == 1 and cm[0][0] == (sc.node_ranges[0], sc.node_ranges[1]) and cm[0][2:] == (2000.0, 1e6, 0.3)
    assert sc.shell is not None and np.all(sc.shell["rho"] == 900.0) and sc.shell["tri"].min() == sc.node_ranges[1]


def test_different_bend_scales_are_refused(cloth):
    text = "shapes input 2\ncloth.obj 0 0 0  0 0 0  1 1 1 shell 0.002 bend 2\ncloth.obj 0 2 0  0 0 0  1 1 1 shell 0.002 bend 3\n"
    with pytest.raises(ValueError, match="one bend scale per scene"):
        run(text, cloth[0])


def test_partly_held_cloth_keeps_its_dirichlet_box(cloth):
    folder, V, tri = cloth
    _, sc, calls = run(scene_text("shell 0.002 DBC 0 0 0  0.1 1 1  0 0 0  0 0 0"), folder)
    assert len(sc.dirichlet) == 1 and 0 < len(sc.dirichlet[0][0]) < len(V)
    assert [n for n, _, _ in calls].count("set_shell") == 1


def test_the_same_scene_without_the_keyword_is_still_refused(cloth):
    with pytest.raises(ss.UnsupportedKeyword, match="codimensional shape that no script fixes or moves"):
        run(scene_text(""), cloth[0])


def test_a_held_triangle_shape_without_the_keyword_never_calls_set_shell(cloth):
    _, sc, calls = run(scene_text("linearVelocity 0 0 0"), cloth[0])
    assert "set_shell" not in [n for n, _, _ in calls] and sc.shell is None
