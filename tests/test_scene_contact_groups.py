"""The contact-group keywords of a scene script (`contactGroup g` on a shape line, `contactIgnore g h`, `contactFric g h mu`; this project's keywords, not
the reference's): what they parse to, the tables and friction ratios the backend receives (a recording stub: no GPU), scenes without them, error cases."""
import dataclasses

import numpy as np
import pytest

from ipc_amd import scene, scene_script as ss

PLAIN = """
shapes input 3
bar.msh 0 0 0  0 0 0  1 1 1
bar.msh 0 2 0  0 0 0  1 1 1 material 2000 1e6 0.3
bar.msh 0 4 0  0 0 0  1 1 1
selfCollisionOn
selfFric 0.2
"""

GROUPS = """
shapes input 3
bar.msh 0 0 0  0 0 0  1 1 1 contactGroup 2
bar.msh 0 2 0  0 0 0  1 1 1 material 2000 1e6 0.3 contactGroup 1
bar.msh 0 4 0  0 0 0  1 1 1
selfCollisionOn
selfFric 0.2
contactIgnore 2 1
contactFric 0 1 0.8
contactFric 2 2 0.1
"""


class Recorder:
    """a backend that records every call apply() makes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


def run(text):
    cfg = ss.SceneConfig.parse(text, "/x")
    V, T = scene.make_bar(2, 1, 1, size=(2.0, 1.0, 1.0))
    sc = ss.assemble(cfg, lambda p: (V.copy(), T.copy(), scene.surface_tris(T)))
    be = Recorder()
    ss.apply(sc, be)
    return cfg, sc, be.calls


def test_keywords_parse_to_groups_matrix_self_fric_and_ratios():
    cfg, sc, calls = run(GROUPS)
    assert [sh.contact_group for sh in cfg.shapes] == [2, 1, 0]
    assert cfg.shapes[1].material == (2000.0, 1e6, 0.3)  # the keyword behind another one on the line
    assert cfg.contact_ignore == [(2, 1)] and cfg.contact_fric == [(0, 1, 0.8), (2, 2, 0.1)]
    assert cfg.self_fric == 0.2 and cfg.effective_self_fric() == 0.8
    groups, collide, scale, mu = cfg.contact_group_tables()
    assert groups.tolist() == [2, 1, 0] and mu == 0.8
    assert collide.tolist() == [[1, 1, 1], [1, 1, 0], [1, 0, 1]]
    want = np.full((3, 3), 0.2 / 0.8)  # pairs without a line carry selfFric
    want[0, 1] = want[1, 0] = 1.0
    want[2, 2] = 0.1 / 0.8
    assert np.array_equal(scale, want)
    assert np.array_equal(scale, scale.T) and np.array_equal(collide, collide.T)
    names = [n for n, _, _ in calls]
    assert names.count("set_contact_groups") == 1
    assert names.index("set_components") < names.index("set_contact_groups") < names.index("opt_init")
    (g, c, s), = [a for n, a, _ in calls if n == "set_contact_groups"]
    assert g.tolist() == [2, 1, 0] and np.array_equal(c, collide) and np.array_equal(s, want)
    assert len(g) == len([a for n, a, _ in calls if n == "set_components"][0][0])
    assert [a[0] for n, a, _ in calls if n == "set_friction"] == [0.8]  # the largest coefficient


def test_ignore_alone_sends_no_scales_and_keeps_self_fric():
    cfg, _, calls = run(PLAIN + "contactIgnore 0 0\n")
    groups, collide, scale, mu = cfg.contact_group_tables()
    assert groups.tolist() == [0, 0, 0] and collide.tolist() == [[0]] and scale is None and mu == 0.2
    (g, c, s), = [a for n, a, _ in calls if n == "set_contact_groups"]
    assert s is None and c.tolist() == [[0]]
    assert [a[0] for n, a, _ in calls if n == "set_friction"] == [0.2]


def test_fric_lines_without_any_friction_send_no_scales():
    cfg = ss.SceneConfig.parse("contactFric 0 1 0\n")
    groups, collide, scale, mu = cfg.contact_group_tables(2)
    assert groups.tolist() == [0, 0] and collide.tolist() == [[1, 1], [1, 1]] and scale is None and mu == 0.0


def test_a_later_line_replaces_an_earlier_one_and_smaller_coefficients_keep_self_fric_on_top():
    cfg = ss.SceneConfig.parse("selfFric 0.5\ncontactFric 0 1 0.3\ncontactFric 1 0 0.1\n")
    _, _, scale, mu = cfg.contact_group_tables(1)
    assert mu == 0.5 and scale.tolist() == [[1.0, 0.2], [0.2, 1.0]]


def test_mesh_collision_objects_behind_the_shapes_are_in_group_zero():
    cfg = ss.SceneConfig.parse(GROUPS, "/x")
    groups, *_ = cfg.contact_group_tables(5)
    assert groups.tolist() == [2, 1, 0, 0, 0]
    with pytest.raises(ValueError):
        cfg.contact_group_tables(2)


def test_a_scene_without_the_keywords_is_what_it_was():
    cfg, _, calls = run(PLAIN)
    assert not cfg.uses_contact_groups() and cfg.contact_group_tables() is None and cfg.effective_self_fric() == cfg.self_fric
    assert cfg.contact_ignore == [] and cfg.contact_fric == [] and all(sh.contact_group == 0 for sh in cfg.shapes)
    names = [n for n, _, _ in calls]
    assert "set_contact_groups" not in names
    assert names == ["set_mesh", "set_components", "set_energy_type", "set_component_material", "opt_init", "set_surface", "enable_self_collision",
                     "set_friction", "set_rel_tol", "precompute"]
    assert [a for n, a, _ in calls if n == "set_friction"] == [(0.2, 1, 1e-3)]
    # `contactGroup 0` everywhere says nothing: the same configuration, field by field, and the same calls
    cfg0, _, calls0 = run(PLAIN.replace("1 1 1\n", "1 1 1 contactGroup 0\n"))
    for f in dataclasses.fields(cfg):
        if f.name != "shapes":
            assert getattr(cfg, f.name) == getattr(cfg0, f.name), f.name
    assert [n for n, _, _ in calls0] == names


@pytest.mark.parametrize("text", ["contactIgnore 0 16\n", "contactIgnore -1 0\n", "contactIgnore 3\n", "contactFric 0 1\n", "contactFric 0 1 -0.1\n",
                                  "contactFric 0 1 nan\n", "contactFric 0 1 inf\n", "contactFric 0 99 0.5\n", "contactIgnore a b\n",
                                  "shapes input 1\nbar.msh 0 0 0  0 0 0  1 1 1 contactGroup 16\n", "shapes input 1\nbar.msh 0 0 0  0 0 0  1 1 1 contactGroup\n",
                                  "shapes input 1\nbar.msh 0 0 0  0 0 0  1 1 1 contactGroup -2\n"])
def test_error_cases(text):
    with pytest.raises(ValueError):
        ss.SceneConfig.parse(text, "/x")


def test_other_unknown_keywords_still_raise():
    with pytest.raises(ss.UnsupportedKeyword):
        ss.SceneConfig.parse("contactGroups 1\n")
    with pytest.raises(ss.UnsupportedKeyword):
        ss.SceneConfig.parse("shapes input 1\nbar.msh 0 0 0  0 0 0  1 1 1 contactgroup 1\n", "/x")


def test_the_binding_passes_tables_and_the_reset_through():
    from ipc_amd import lib as gl

    class L:
        def ipcgpu_set_contact_groups(self, h, nComp, group, nGroups, collide, scale):
            self.got = (nComp.value, None if not group else [group[i] for i in range(nComp.value)], nGroups.value,
                        None if not collide else [collide[i] for i in range(nGroups.value ** 2)],
                        None if not scale else [scale[i] for i in range(nGroups.value ** 2)])
            return 0
    c = gl.Context.__new__(gl.Context)
    c._L, c.h = L(), None
    c.set_contact_groups([1, 0, 1], [[1, 0], [0, 1]], [[1.0, 0.5], [0.5, 0.0]])
    assert c._L.got == (3, [1, 0, 1], 2, [1, 0, 0, 1], [1.0, 0.5, 0.5, 0.0])
    c.set_contact_groups([0], [[1]])
    assert c._L.got == (1, [0], 1, [1], None)
    c.set_contact_groups(None, None)
    assert c._L.got == (0, None, 0, None, None)
    with pytest.raises(ValueError):
        c.set_contact_groups([0, 1], [[1, 1]])
    with pytest.raises(ValueError):
        c.set_contact_groups([0, 1], [[1, 1], [1, 1]], [[1.0]])
    c.h = None  # nothing to destroy
