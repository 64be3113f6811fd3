"""The shape-line keyword `pressure <p> [ramp <s>] [gas <ambient> [gamma <g>]]`: what `gas` parses to, its errors, `ramp` together with `gas`, and what the
backend receives (the recording stub of test_scene_chamber.py: no GPU).  A scene without `gas` never calls chamber_set_gas."""
import numpy as np
import pytest

from ipc_amd import scene_script as ss

from test_scene_chamber import folder, run, scene_text  # noqa: F401  (folder is a fixture)

CUBE = "cube.obj 0 0 0  0 0 0  1 1 1 shell 0.001 "


def test_gas_parses_with_and_without_gamma_and_ramp(folder):
    cfg = ss.SceneConfig.parse(scene_text(CUBE + "pressure 40 gas 1e5", CUBE + "pressure 40 ramp 0.2 gas 1e5 gamma 1.4", CUBE + "pressure -30 gas 100 gamma 1",
                                          CUBE + "pressure 40"), folder)
    got = [(s.pressure, s.pressure_ramp, s.pressure_gas, s.pressure_ambient, s.pressure_gamma) for s in cfg.shapes]
    assert got == [(40.0, 0.0, True, 1e5, 1.0), (40.0, 0.2, True, 1e5, 1.4), (-30.0, 0.0, True, 100.0, 1.0), (40.0, 0.0, False, 0.0, 1.0)]


@pytest.mark.parametrize("tail", ["pressure 40 gas", "pressure 40 gas nan", "pressure 40 gas -1", "pressure 40 gas inf", "pressure 40 gas 1e5 gamma", "pressure 40 gas 1e5 gamma 0.9",
                                  "pressure 40 gas 1e5 gamma nan", "pressure -30 gas 30", "pressure -30 gas 20", "pressure 40 ramp 1 gas 0", "pressure -40 ramp 1 gas 40"])
def test_gas_errors(folder, tail):
    with pytest.raises(ValueError) as e:
        ss.SceneConfig.parse(scene_text(CUBE + tail), folder)
    assert not isinstance(e.value, ss.UnsupportedKeyword)


def test_backend_receives_set_gas_behind_set_chambers_and_the_ramp_pumps(folder):
    cfg, sc, calls = run(scene_text(CUBE + "pressure 40 ramp 0.2 gas 1e5 gamma 1.4", "cube.obj 3 0 0  0 0 0  1 1 1 shell 0.001 pressure 7"), folder)
    names = [c[0] for c in calls]
    assert names.count("chamber_set_gas") == 1 and names.index("set_chambers") < names.index("chamber_set_gas") < names.index("opt_init")
    (gas, amb, gamma), = [a for nm, a, _ in calls if nm == "chamber_set_gas"]
    assert gas.tolist() == [True, False] and amb.tolist() == [1e5, 0.0] and gamma.tolist() == [1.4, 1.0]
    assert set(sc.chambers) == {"tri_lists", "pressure", "ramp", "gas", "ambient", "gamma"}
    assert np.allclose(sc.chamber_pressures(0.1), [20.0, 7.0]) and np.allclose(sc.chamber_pressures(0.5), [40.0, 7.0])  # the ramp pumps the gas in


def test_a_scene_without_gas_never_calls_set_gas(folder):
    _, sc, calls = run(scene_text(CUBE + "pressure 40 ramp 0.2"), folder)
    assert "chamber_set_gas" not in [c[0] for c in calls] and set(sc.chambers) == {"tri_lists", "pressure", "ramp"}
