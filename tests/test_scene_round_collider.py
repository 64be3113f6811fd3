"""The `sphereCollider` and `capsuleCollider` lines of a scene script: parsing, the defaults, every malformed line refused with its message, a scene
without them parsing as before, and what apply() and the per-step move hand to a backend.  No GPU."""
import dataclasses

import numpy as np
import pytest

from ipc_amd import scene_script as ss

BASE = "energy NH\ntime 1 0.01\n"


def parse(extra):
    return ss.SceneConfig.parse(BASE + extra, ".")


def test_defaults_and_every_option():
    cfg = parse("sphereCollider 0.5 -1 0.25 0.75\ncapsuleCollider 0 0 0 1 0 0 0.5\n"
                "sphereCollider 0 0 0 2 hollow friction 0.3 velocity 0 -0.5 0\ncapsuleCollider 0 1 0 0 1 2 0.1 velocity 1 0 0 friction 0.2\n")
    a, b, c, d = cfg.round_colliders
    assert np.array_equal(a["p0"], [0.5, -1, 0.25]) and np.array_equal(a["p1"], a["p0"]) and a["R"] == 0.75
    assert a["hollow"] is False and a["friction"] == 0.0 and a["velocity"] is None
    assert np.array_equal(b["p0"], [0, 0, 0]) and np.array_equal(b["p1"], [1, 0, 0]) and b["R"] == 0.5 and b["velocity"] is None and not b["hollow"]
    assert c["hollow"] is True and c["friction"] == 0.3 and np.array_equal(c["velocity"], [0, -0.5, 0]) and c["R"] == 2.0
    assert d["friction"] == 0.2 and np.array_equal(d["velocity"], [1, 0, 0]) and np.array_equal(d["p1"], [0, 1, 2])


BAD = [("sphereCollider 0 0 0", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 x 1", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 0 1 solid", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 0 1 friction", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 0 1 velocity 1 2", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 0 1 friction mu", "sphereCollider needs <cx> <cy> <cz> <R>"),
       ("sphereCollider 0 0 0 1 hollow hollow", "hollow is given twice"),
       ("sphereCollider 0 0 0 0", "the radius must be positive"),
       ("sphereCollider 0 0 0 -1", "the radius must be positive"),
       ("sphereCollider 0 nan 0 1", "must be finite"),
       ("sphereCollider 0 0 0 inf", "must be finite"),
       ("sphereCollider 0 0 0 1 friction -0.1", "friction coefficient must be finite and not negative"),
       ("sphereCollider 0 0 0 1 velocity 0 inf 0", "the velocity must be finite"),
       ("capsuleCollider 0 0 0 1 0 0", "capsuleCollider needs <ax> <ay> <az> <bx> <by> <bz> <R>"),
       ("capsuleCollider 0 0 0 1 0 0 0.5 hollow", "only a sphere may be hollow"),
       ("capsuleCollider 0 0 0 0 0 0 0.5", "the two end points coincide"),
       ("capsuleCollider 0 0 0 1 0 0 0", "the radius must be positive"),
       ("capsuleCollider 0 0 0 1 0 0 0.5 friction 0.1 friction 0.2", "friction is given twice")]


@pytest.mark.parametrize("line,message", BAD)
def test_malformed_lines_are_refused_with_their_message(line, message):
    with pytest.raises(ValueError) as e:
        parse(line + "\n")
    assert message in str(e.value) and str(e.value).startswith(line.split()[0])


def test_a_scene_without_the_lines_parses_as_before():
    cfg = parse("ground 0.1 -1\n")
    assert cfg.round_colliders == () and len(cfg.half_spaces) == 1
    assert "round_colliders" not in {f.name for f in dataclasses.fields(ss.SceneConfig)}
    assert "round_colliders" not in dataclasses.asdict(cfg)
    with pytest.raises(ss.UnsupportedKeyword):
        parse("torusCollider 0 0 0 1 0.2\n")
    # two configurations do not share a list
    parse("sphereCollider 0 0 0 1\n")
    assert parse("").round_colliders == ()


class Recorder:
    def __init__(self, left):
        self.calls, self.left = [], list(left)

    def round_move(self, idx, delta, slackness):
        self.calls.append((idx, np.array(delta), slackness))
        return self.left.pop(0)


def test_the_move_before_a_step_carries_what_was_left_over():
    cfg = parse("sphereCollider 0 0 0 1\nsphereCollider 0 5 0 1 velocity 0 -2 0\n")
    sc = ss.AssembledScene(cfg, np.zeros((0, 3)), np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32), [], [], [], np.zeros((0, 3)))
    be = Recorder([0.25, 0.0, 0.5])
    assert sc.move_round_colliders(be) == [0.25]
    assert sc.move_round_colliders(be) == [0.0]
    assert sc.move_round_colliders(be) == [0.5]
    step = np.array([0.0, -0.02, 0.0])
    assert [q[0] for q in be.calls] == [1, 1, 1] and all(q[2] == 0.5 for q in be.calls)  # the collider at rest is never moved
    assert np.array_equal(be.calls[0][1], step) and np.array_equal(be.calls[1][1], step + 0.25 * step) and np.array_equal(be.calls[2][1], step)
