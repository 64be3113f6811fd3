"""`energy SNH` in a scene script: it parses, and reaches set_energy_type("SNH") of the backend (a recording stub: no GPU); any other unknown energy name still
raises UnsupportedKeyword."""
import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

SCENE = """
energy SNH
shapes input 1
bar.msh 0 0 0  0 0 0  1 1 1
selfCollisionOff
"""


class Recorder:
    """a backend that records every call apply() makes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


def test_energy_snh_parses_and_reaches_the_backend():
    cfg = ss.SceneConfig.parse(SCENE, "/x")
    assert cfg.energy == "SNH"
    V, T = scene.make_bar(2, 1, 1, size=(2.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (V.copy(), T.copy(), scene.surface_tris(T)))
    be = Recorder()
    ss.apply(sc, be)
    energy = [a for n, a, _ in be.calls if n == "set_energy_type"]
    assert energy == [("SNH",)]
    names = [n for n, _, _ in be.calls]
    assert names.index("set_mesh") < names.index("set_energy_type") < names.index("opt_init")


def test_the_binding_maps_snh_to_energy_type_2():
    from ipc_amd import lib as gl

    class L:
        def ipcgpu_set_energy_type(self, h, t):
            self.got = t.value
            return 0
    c = gl.Context.__new__(gl.Context)
    c._L, c.h = L(), None
    for name, code in (("NH", 0), ("FCR", 1), ("SNH", 2)):
        c.set_energy_type(name)
        assert c._L.got == code
    with pytest.raises(KeyError):
        c.set_energy_type("XYZ")


@pytest.mark.parametrize("name", ["XYZ", "snh", "StVK"])
def test_other_energy_names_still_raise(name):
    with pytest.raises(ss.UnsupportedKeyword):
        ss.SceneConfig.parse(f"energy {name}\n")
    assert np.all([ss.SceneConfig.parse(f"energy {e}\n").energy == e for e in ("NH", "FCR", "SNH")])
