"""The `weave <E1> <E2> <G12> dir <x> <y> <z> [nu12 <v>] [bendwarp <s>] [bendweft <s>]` part of the `shell` keyword of a shape line (this project's keyword, not
the reference's): what it parses to, its defaults, where it is refused and why, and the per-triangle arrays the backend receives per shape (a recording stub: no
GPU).  A shell without it behaves as before."""
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


def scene_text(*tails, rotate="0 0 0"):
    lines = "".join(f"cloth.obj {k} 1 0  {rotate}  1 1 1 {tail}\n" for k, tail in enumerate(tails))
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
    assert shape("shell 0.002").shell_weave is None
    b = shape("shell 0.002 weave 1e5 5e4 2e3 dir 1 0 0")
    assert b.shell_weave == {"E1": 1e5, "E2": 5e4, "G12": 2e3, "dir": (1.0, 0.0, 0.0), "nu12": 0.0, "bendwarp": 1.0, "bendweft": 1.0}
    assert (b.shell_rubber, b.shell_bend, b.shell_limit, b.shell_plastic) == (False, 1.0, None, None)
    c = shape("material 900 1e6 0.3 shell 0.001 bend 0.5 weave 2e5 1e5 1e3 dir 0 1 1 nu12 0.3 bendwarp 10 bendweft 2 limit 1.3 onset 1.05 stiff 2.5 contactGroup 2")
    assert c.shell_weave == {"E1": 2e5, "E2": 1e5, "G12": 1e3, "dir": (0.0, 1.0, 1.0), "nu12": 0.3, "bendwarp": 10.0, "bendweft": 2.0}
    assert (c.shell_thickness, c.shell_bend, c.shell_limit, c.shell_onset, c.shell_stiff, c.contact_group) == (0.001, 0.5, 1.3, 1.05, 2.5, 2)
    d = shape("shell 0.002 weave 1e5 5e4 2e3 dir 1 1 0 bendweft 3 linearVelocity 1 0 0")
    assert (d.shell_weave["bendwarp"], d.shell_weave["bendweft"], d.lin_vel) == (1.0, 3.0, (1.0, 0.0, 0.0))
    for bad in ("shell 0.01 weave", "shell 0.01 weave 1e5 5e4 2e3", "shell 0.01 weave 1e5 5e4 2e3 dir 1 0", "shell 0.01 weave 1e5 5e4 dir 1 0 0", "shell 0.01 weave 0 5e4 2e3 dir 1 0 0",
                "shell 0.01 weave 1e5 -1 2e3 dir 1 0 0", "shell 0.01 weave 1e5 5e4 inf dir 1 0 0", "shell 0.01 weave 1e5 5e4 2e3 dir 0 0 0", "shell 0.01 weave 1e5 5e4 2e3 dir nan 0 0",
                "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 nu12", "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 nu12 1.5", "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 bendwarp 0",
                "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 bendweft -1", "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 bendweft 2 bendwarp 3", "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 bend 2",
                "shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 weave 1e5 5e4 2e3 dir 1 0 0", "shell 0.01 limit 1.2 weave 1e5 5e4 2e3 dir 1 0 0", "shell 0.01 nu12 0.2", "shell 0.01 bendwarp 2",
                "weave 1e5 5e4 2e3 dir 1 0 0", "weave 1e5 5e4 2e3 dir 1 0 0 shell 0.01"):
        with pytest.raises(ValueError):
            ss.SceneConfig.parse(scene_text(bad), folder)


def test_weave_excludes_rubber_and_yield_and_says_why(cloth):
    folder = cloth[0]
    for bad, why in (("shell 0.01 rubber weave 1e5 5e4 2e3 dir 1 0 0", "weave is not valid behind rubber: a triangle carries one membrane law"),
                     ("shell 0.01 rubber mr 0.2 weave 1e5 5e4 2e3 dir 1 0 0", "weave is not valid behind rubber"),
                     ("shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 rubber", "rubber is not valid behind weave: a triangle carries one membrane law"),
                     ("shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 yield 0.01", "yield is not valid behind weave: plastic flow rewrites the rest metric"),
                     ("shell 0.01 weave 1e5 5e4 2e3 dir 1 0 0 limit 1.2 yield 0.01", "yield is not valid behind weave")):
        with pytest.raises(ValueError, match=why):
            ss.SceneConfig.parse(scene_text(bad), folder)
    # the texts the keyword's neighbours had stay word for word
    with pytest.raises(ValueError, match="yield is not valid behind rubber: a rubber membrane has no plastic flow"):
        ss.SceneConfig.parse(scene_text("shell 0.01 rubber yield 0.01"), folder)
    with pytest.raises(ValueError, match="mr belongs behind rubber"):
        ss.SceneConfig.parse(scene_text("shell 0.01 mr 0.2"), folder)


def test_backend_receives_the_weave_per_triangle_per_shape(cloth):
    folder, V, tri = cloth
    nt = len(tri)
    _, sc, calls = run(scene_text("shell 0.002 weave 1e5 5e4 2e3 dir 2 0 0 nu12 0.3 bendwarp 10", "shell 0.002", "shell 0.002 weave 3e5 1e5 1e3 dir 0 1 0 bendweft 4 limit 1.2",
                                  "shell 0.002 rubber"), folder)
    names = [c[0] for c in calls]
    assert names.index("set_shell") < names.index("set_shell_membrane") < names.index("set_shell_weave") < names.index("set_shell_strain_limit") < names.index("opt_init")
    woven, d, E1, E2, G12, nu12, bw, bf = next(c[1] for c in calls if c[0] == "set_shell_weave")
    rep = lambda *v: np.repeat(np.array(v, dtype=np.float64), nt)
    assert woven.dtype == np.int32 and np.array_equal(woven, np.repeat([1, 0, 1, 0], nt))
    on = woven == 1
    assert np.array_equal(E1[on], rep(1e5, 3e5)) and np.array_equal(E2[on], rep(5e4, 1e5)) and np.array_equal(G12[on], rep(2e3, 1e3))
    assert np.array_equal(nu12, rep(0.3, 0.0, 0.0, 0.0)) and np.array_equal(bw, rep(10.0, 1.0, 1.0, 1.0)) and np.array_equal(bf, rep(1.0, 1.0, 4.0, 1.0))
    assert d.shape == (4 * nt, 3) and np.array_equal(d[:nt], np.tile([1.0, 0.0, 0.0], (nt, 1))) and np.array_equal(d[2 * nt:3 * nt], np.tile([0.0, 1.0, 0.0], (nt, 1)))  # unit
    assert np.array_equal(next(c[1] for c in calls if c[0] == "set_shell_membrane")[0], np.repeat([0, 0, 0, 1], nt))
    assert np.array_equal(sc.shell["weave"]["woven"], woven) and len(sc.shell["tri"]) == 4 * nt


def test_the_direction_turns_with_the_shape(cloth):
    folder, _, tri = cloth
    _, sc, calls = run(scene_text("shell 0.002 weave 1e5 5e4 2e3 dir 1 0 0", rotate="0 0 90"), folder)
    d = next(c[1] for c in calls if c[0] == "set_shell_weave")[1]
    assert np.allclose(d, np.tile([0.0, 1.0, 0.0], (len(tri), 1)), atol=1e-15)


def test_a_scene_without_the_word_makes_no_weave_call(cloth):
    folder = cloth[0]
    _, sc, calls = run(scene_text("shell 0.002 limit 1.2", "shell 0.002 rubber"), folder)
    assert "weave" not in sc.shell
    assert "set_shell_weave" not in [c[0] for c in calls] and "set_shell" in [c[0] for c in calls]
