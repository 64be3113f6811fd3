"""The `attach` and `stitch` lines of a scene (this project's keywords, not the reference's): what they parse to, where they are refused, and what the
backend receives (a recording stub: no GPU).  A scene without them never calls set_attachments."""
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
def strip(tmp_path):
    """a 4 x 2-node strip in the plane z = 0: x = 0 .. 0.3, y = 0 .. 0.1"""
    V, tri = smp.grid(4, 2, 0.1)
    (tmp_path / "strip.obj").write_text("".join(f"v {a} {b} {c}\n" for a, b, c in V) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in tri))
    return str(tmp_path), V, tri


def scene_text(tail, gap=0.32):
    """two strips, the second `gap` behind the first along x (its first column 0.02 from the first one's last)"""
    return (f"shapes input 2\nstrip.obj 0 0 0  0 0 0  1 1 1 shell 0.001 DBC 0 0 0  0.1 1 1  0 0 0  0 0 0\nstrip.obj {gap} 0 0  0 0 0  1 1 1 shell 0.001\n"
            f"density 500\nstiffness 2e5 0.35\n{tail}\n")


def run(text, folder):
    cfg = ss.SceneConfig.parse(text, folder)
    Vb, Tb = scene.make_bar(1, 1, 1, size=(1.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (Vb.copy(), Tb.copy(), scene.surface_tris(Tb)))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_lines_parse(strip):
    cfg = ss.SceneConfig.parse(scene_text("attach 0 3 1 0 250\nattach 1 7 0 4 10 0.05\nstitch 0 1 0.03 400\nstitch 1 0 0.5 7 rest"), strip[0])
    assert cfg.attach == [(0, 3, 1, 0, 250.0, 0.0), (1, 7, 0, 4, 10.0, 0.05)]
    assert cfg.stitch == [(0, 1, 0.03, 400.0, False), (1, 0, 0.5, 7.0, True)]
    for bad in ("attach 0 3 1 0", "attach 0 3 1 0 0", "attach 0 3 1 0 -5", "attach 0 3 1 0 10 -0.1", "attach 0 3 1 0 10 0.1 2", "attach 0 3 1 0 nan",
                "stitch 0 1 0.03", "stitch 0 1 -0.03 400", "stitch 0 1 0.03 0", "stitch 0 1 0.03 400 resting"):
        with pytest.raises(ValueError) as e:
            ss.SceneConfig.parse(scene_text(bad), strip[0])
        assert not isinstance(e.value, ss.UnsupportedKeyword), bad


def test_two_sewn_strips_reach_set_attachments_once_behind_set_shell(strip):
    folder, V, tri = strip
    n = len(V)
    cfg, sc, calls = run(scene_text("attach 0 0 1 7 50 0.4\nstitch 0 1 0.03 400"), folder)
    names = [c[0] for c in calls]
    assert names.count("set_attachments") == 1
    assert names.index("set_mesh") < names.index("set_shell") < names.index("set_attachments") < names.index("opt_init")
    (A, B, k, L), = [a for nm, a, _ in calls if nm == "set_attachments"]
    # the attach line first, then the seam: the last column of strip 0 (local nodes 3 and 7) to the first of strip 1 (local 0 and 4)
    assert A.tolist() == [0, 3, 7] and B.tolist() == [n + 7, n + 0, n + 4]
    assert k.tolist() == [50.0, 400.0, 400.0] and L.tolist() == [0.4, 0.0, 0.0]
    assert A.dtype == np.int32 and B.dtype == np.int32
    # with `rest` the rest distance of each pair; a larger radius takes more nodes, each to its NEAREST node of the other shape
    _, sc, calls = run(scene_text("stitch 1 0 0.13 400 rest"), folder)
    (A, B, k, L), = [a for nm, a, _ in calls if nm == "set_attachments"]
    assert A.tolist() == [n + 0, n + 1, n + 4, n + 5] and B.tolist() == [3, 3, 7, 7]
    assert np.allclose(L, [0.02, 0.12, 0.02, 0.12], rtol=0, atol=1e-15)
    assert np.allclose(L, np.linalg.norm(sc.V[A] - sc.V[B], axis=1), rtol=0, atol=0)


def test_rest_lengths_follow_the_size_keyword(strip):
    _, sc, calls = run(scene_text("stitch 0 1 0.03 400 rest\nsize 6.2"), strip[0])  # the model is 0.62 long: scaled by 10
    (A, B, k, L), = [a for nm, a, _ in calls if nm == "set_attachments"]
    assert len(A) == 2 and np.allclose(L, 0.2, rtol=1e-13, atol=0)


def test_errors(strip):
    folder = strip[0]
    for tail, word in (("stitch 0 1 0.01 400", "no node of shape 0 lies within 0.01"), ("stitch 0 2 0.03 400", "shape 2 does not exist"),
                       ("stitch 1 1 0.03 400", "must differ"), ("attach 0 8 1 0 10", "node 8 does not exist in shape 0"),
                       ("attach 0 -1 1 0 10", "node -1 does not exist"), ("attach 2 0 1 0 10", "shape 2 does not exist"),
                       ("attach 1 3 1 3 10", "tied to itself")):
        with pytest.raises(ValueError, match=word):
            run(scene_text(tail), folder)


def test_a_scene_without_the_lines_never_calls_set_attachments(strip):
    _, sc, calls = run(scene_text(""), strip[0])
    assert "set_attachments" not in [c[0] for c in calls] and sc.attachments is None
