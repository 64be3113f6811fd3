"""The `rubber [mr <alpha>]` part of the `shell` keyword of a shape line (this project's keyword, not the reference's): what it parses to, its defaults, where
it is refused, and the per-triangle arrays the backend receives per shape (a recording stub: no GPU).  A shell without it behaves as before."""
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


def scene_text(*tails):
    lines = "".join(f"cloth.obj {k} 1 0  0 0 0  1 1 1 {tail}\n" for k, tail in enumerate(tails))
    return f"shapes input {len(tails)}\n{lines}density 500\nstiffness 2e5 0.35\nselfCollisionOn\n"


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    Vb, Tb = scene.make_bar(1, 1, 1, size=(1.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (Vb.copy(), Tb.copy(), scene.surface_tris(Tb)))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_keyword_grammar_and_defaults(cloth):
    folder = cloth[0]
    shape = lambda tail: ss.SceneConfig.parse(scene_text(tail), folder).shapes[0]
    a = shape("shell 0.002")
    assert a.shell_rubber is False and a.shell_alpha == 0.0
    b = shape("shell 0.002 rubber")
    assert (b.shell_rubber, b.shell_alpha, b.shell_bend, b.shell_limit) == (True, 0.0, 1.0, None)  # neo-Hookean by default
    c = shape("material 900 1e6 0.3 shell 0.001 bend 0 rubber mr 0.25 limit 1.3 onset 1.05 stiff 2.5 contactGroup 2")
    assert (c.shell_thickness, c.shell_bend, c.shell_rubber, c.shell_alpha, c.shell_limit, c.shell_onset, c.shell_stiff, c.contact_group) \
        == (0.001, 0.0, True, 0.25, 1.3, 1.05, 2.5, 2)
    d = shape("shell 0.002 rubber limit 1.2")
    assert (d.shell_rubber, d.shell_alpha, d.shell_limit) == (True, 0.0, 1.2)
    e = shape("shell 0.002 rubber mr 0 linearVelocity 1 0 0")
    assert (e.shell_rubber, e.shell_alpha, e.lin_vel) == (True, 0.0, (1.0, 0.0, 0.0))
    for bad in ("shell 0.01 rubber mr", "shell 0.01 rubber mr 1", "shell 0.01 rubber mr 1.5", "shell 0.01 rubber mr -0.1", "shell 0.01 rubber mr nan",
                "shell 0.01 rubber mr inf", "shell 0.01 mr 0.2", "shell 0.01 rubber bend 2", "shell 0.01 rubber rubber", "shell 0.01 rubber mr 0.1 mr 0.2",
                "shell 0.01 limit 1.2 rubber", "shell 0.01 limit 1.2 mr 0.1", "shell 0.01 limit 1.2 stiff 2 rubber", "rubber", "shell rubber", "rubber shell 0.01",
                "shell 0.01 rubber mr x"):
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), folder)


def test_backend_receives_the_model_per_triangle_per_shape(cloth):
    folder, V, tri = cloth
    nt = len(tri)
    _, sc, calls = run(scene_text("shell 0.002 rubber mr 0.3", "shell 0.002", "shell 0.002 rubber limit 1.2"), folder)
    names = [c[0] for c in calls]
    assert names.index("set_shell") < names.index("set_shell_membrane") < names.index("set_shell_strain_limit") < names.index("opt_init")
    model, alpha = next(c[1] for c in calls if c[0] == "set_shell_membrane")
    assert model.dtype == np.int32 and np.array_equal(model, np.repeat([1, 0, 1], nt)) and np.array_equal(alpha, np.repeat([0.3, 0.0, 0.0], nt))
    assert np.array_equal(next(c[1] for c in calls if c[0] == "set_shell_strain_limit")[0], np.repeat([0.0, 0.0, 1.2], nt))
    assert np.array_equal(sc.shell["model"], model) and len(sc.shell["tri"]) == 3 * nt


def test_a_scene_without_the_word_makes_no_membrane_call(cloth):
    folder = cloth[0]
    _, sc, calls = run(scene_text("shell 0.002 limit 1.2", "shell 0.002"), folder)
    assert "model" not in sc.shell and "alpha" not in sc.shell
    assert "set_shell_membrane" not in [c[0] for c in calls] and "set_shell" in [c[0] for c in calls]
