"""The `limit <s> [onset <sHat>] [stiff <k>]` tail of the `shell` keyword of a shape line (this project's keyword, not the reference's): what it parses to,
where it is refused, and the per-triangle arrays the backend receives per shape (a recording stub: no GPU).  A shell without it behaves as before."""
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


def test_keyword_grammar(cloth):
    folder = cloth[0]
    shape = lambda tail: ss.SceneConfig.parse(scene_text(tail), folder).shapes[0]
    a = shape("shell 0.002")
    assert a.shell_limit is None and a.shell_onset == 1.0 and a.shell_stiff == 1.0
    b = shape("shell 0.002 limit 1.1")
    assert (b.shell_limit, b.shell_onset, b.shell_stiff, b.shell_bend) == (1.1, 1.0, 1.0, 1.0)
    c = shape("material 900 1e6 0.3 shell 0.001 bend 10 limit 1.3 onset 1.05 stiff 2.5 contactGroup 2")
    assert (c.shell_thickness, c.shell_bend, c.shell_limit, c.shell_onset, c.shell_stiff, c.contact_group) == (0.001, 10.0, 1.3, 1.05, 2.5, 2)
    d = shape("shell 0.002 limit 1.2 stiff 4")
    assert (d.shell_limit, d.shell_onset, d.shell_stiff) == (1.2, 1.0, 4.0)
    for bad in ("shell 0.01 limit", "shell 0.01 limit 1.0", "shell 0.01 limit 0.9", "shell 0.01 limit 1.2 onset", "shell 0.01 limit 1.2 onset 1.2",
                "shell 0.01 limit 1.2 onset 0.9", "shell 0.01 limit 1.2 stiff", "shell 0.01 limit 1.2 stiff 0", "shell 0.01 limit 1.2 stiff -1",
                "shell 0.01 limit nan", "shell 0.01 limit inf", "shell 0.01 onset 1.0", "shell 0.01 stiff 2", "shell 0.01 limit 1.2 stiff 2 onset 1.1",
                "shell 0.01 limit 1.2 bend 2"):
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), folder)


def test_limit_reaches_set_shell_strain_limit_after_set_shell(cloth):
    folder, V, tri = cloth
    _, sc, calls = run(scene_text("shell 0.002 limit 1.1 onset 1.02 stiff 3"), folder)
    names = [n for n, _, _ in calls]
    assert names.count("set_shell") == 1 and names.count("set_shell_strain_limit") == 1
    assert names.index("set_shell") < names.index("set_shell_strain_limit") < names.index("opt_init")
    (limit, onset, stiff), = [a for n, a, _ in calls if n == "set_shell_strain_limit"]
    assert np.array_equal(limit, np.full(len(tri), 1.1)) and np.array_equal(onset, np.full(len(tri), 1.02)) and np.array_equal(stiff, np.full(len(tri), 3.0))


def test_shell_without_limit_never_calls_set_shell_strain_limit(cloth):
    _, sc, calls = run(scene_text("shell 0.002 bend 3"), cloth[0])
    assert "set_shell_strain_limit" not in [n for n, _, _ in calls] and "limit" not in sc.shell


def test_shapes_may_differ(cloth):
    """three cloth shapes: limit 1.1, none, limit 1.3 with onset and stiffness -- one call, per triangle, 0 on the triangles of the shape without a limit"""
    folder, V, tri = cloth
    n = len(tri)
    text = ("shapes input 3\ncloth.obj 0 0 0  0 0 0  1 1 1 shell 0.002 limit 1.1\ncloth.obj 0 2 0  0 0 0  1 1 1 shell 0.002\n"
            "cloth.obj 0 4 0  0 0 0  1 1 1 shell 0.003 limit 1.3 onset 1.1 stiff 0.5\nselfCollisionOn\n")
    _, sc, calls = run(text, folder)
    (limit, onset, stiff), = [a for n_, a, _ in calls if n_ == "set_shell_strain_limit"]
    assert len(sc.shell["tri"]) == 3 * n and len(limit) == 3 * n
    assert np.array_equal(limit, np.repeat([1.1, 0.0, 1.3], n)) and np.array_equal(onset, np.repeat([1.0, 1.0, 1.1], n))
    assert np.array_equal(stiff, np.repeat([1.0, 1.0, 0.5], n))
    assert np.array_equal(sc.shell["thickness"], np.repeat([0.002, 0.002, 0.003], n))
