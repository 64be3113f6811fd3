#!/usr/bin/env python3
"""Writes tests/golden/scene_assembly.json: what ipc_amd/scene_script.py makes of a set of small scenes, in the exact form of tests/scene_dump.py -- the
assembled scene, the backend calls of apply(), and for the scripts with a per-step rule six driven calls of before_step().  One scene per script name the
parser accepts, the scripts that read start positions once more under `rotateModel` and under `size`, the shape keywords under `script null`, and every
refusal of assemble() as exception type and message.  Data only; it uses SceneConfig.parse, assemble, apply and before_step and nothing else of the module,
so the same file records any commit.  tests/test_scene_assembly_golden.py rebuilds every case and compares by equality.

Meshes are boxes of ipc_amd.scene.make_box named by their cells: `b2_2_2.msh` is handed in through read_mesh, `b1_1_1.obj` / `.seg` / `.pt` are written
into a temporary folder (the surface triangles, their edges, the nodes), `sq_1_1_1_obj` is a folder with files 0 .. 7 of a mesh sequence.  --list prints the
cases with the sizes of their Dirichlet groups."""
import contextlib
import inspect
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ipc_amd import scene, scene_script as ss  # noqa: E402
import scene_dump as sd  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_assembly.json")
STEPS = 6
PUSH = (False, True, True, False, True, False)  # the steps that start with the deciding nodes beyond the rule's threshold


def script_literals():
    """the script names `parse` spells out itself, read from its `script` branch (the families are the module's tuples)"""
    src = inspect.getsource(ss.SceneConfig.parse)
    line = src[src.index('k == "script"'):].splitlines()[1]
    return tuple(re.findall(r'"(\w+)"', line.split("+")[0]))


def script_names():
    names = script_literals() + ss.HANDLE_SCRIPTS + ss.HOLD_SCRIPTS + ss.PULL_SCRIPTS + ss.INITVEL_SCRIPTS + ss.RULE_SCRIPTS + tuple(ss.DCO_SCRIPTS)
    return tuple(dict.fromkeys(names))


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------------------------
def _box(name):
    n = [int(x) for x in re.match(r"b(\d+)_(\d+)_(\d+)", name).groups()]
    V, F = scene.make_box(*n)
    return V, F, scene.surface_tris(F)


def read_mesh(path):
    name = os.path.basename(path)
    V, F, SF = _box(name[2:] if name.startswith("n_") else name)
    return V, F, (np.zeros((0, 3), dtype=np.int32) if name.startswith("n_") else SF)  # `n_b1_1_1.msh`: a mesh that comes without surface triangles


def _write_obj(path, V, SF=()):
    with open(path, "w") as f:
        f.writelines("v %r %r %r\n" % tuple(float(c) for c in v) for v in V)
        f.writelines("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in SF)


def _write_seg(path, V, SF):
    edges = sorted({(min(a, b), max(a, b)) for t in np.asarray(SF).tolist() for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))})
    with open(path, "w") as f:
        f.writelines("v %r %r %r\n" % tuple(float(c) for c in v) for v in V)
        f.writelines("s %d %d\n" % (a + 1, b + 1) for a, b in edges)


def write_files(text, folder):
    """every mesh file and sequence folder the scene text names"""
    for name, ext in set(re.findall(r"\b((?:open_|flip_)?b\d+_\d+_\d+)\.(obj|seg|pt)\b", text)):
        V, _F, SF = _box(name.split("_", 1)[1] if name[0] != "b" else name)
        path = os.path.join(folder, f"{name}.{ext}")
        if name.startswith("open_"):
            SF = SF[1:]  # one triangle missing
        elif name.startswith("flip_"):
            SF = np.vstack([SF[:1, ::-1], SF[1:]])  # one triangle walks the other way
        if ext == "obj":
            _write_obj(path, V, SF)
        elif ext == "seg":
            _write_seg(path, V, SF)
        else:
            _write_obj(path, V)
    for name, dims, ext in set(re.findall(r"\b(sq_(\d+_\d+_\d+)_(obj|seg|pt))\b", text)):
        V, _F, SF = _box("b" + dims)
        os.makedirs(os.path.join(folder, name), exist_ok=True)
        for i in range(STEPS + 2):
            W = V + np.array([0.0, 0.03125 * i, 0.0])
            path = os.path.join(folder, name, f"{i}.{ext}")
            if ext == "seg":
                _write_seg(path, W, SF)
            else:
                _write_obj(path, W, SF if ext == "obj" else ())


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------
def _shapes(*lines):
    return f"shapes input {len(lines)}\n" + "".join(l + "\n" for l in lines)


BODY = "b2_2_2.msh 0 0 0  0 0 0  1 1 1"
WIDE = "b4_2_2.msh 0 0 0  0 0 0  1 1 1"


def _plate(x, y=0.0, z=0.0, ext="obj"):
    return f"b1_1_1.{ext} {x} {y} {z}  0 0 0  1 1 1"


PLATES6 = [_plate(-2), _plate(2), _plate(0, -2), _plate(0, 2), _plate(0, 0, -2), _plate(0, 0, 2)]
FAR6 = "halfSpace -1 0 0  1 0 0  1 0\nhalfSpace 2 0 0  -1 0 0  1 0\n" \
       "halfSpace 0 0.46875 0  0 1 0  1 0.5\nhalfSpace 0 0.5 0  0 -1 0  1 0\nhalfSpace 0 0 -1  0 0 1  1 0\nhalfSpace 0 0 2  0 0 -1  1 0\n"
# what a script needs beside `script <name>` and one default box
SCENES = {
    "dragright": "meshCO b1_1_1.obj 0.5 -1 0.5  0.5 0 0\n" + _shapes(BODY),
    "ACOSquash": "halfSpace -1 0 0  1 0 0  1 0\nhalfSpace 2 0 0  -1 0 0  1 0.25\n" + _shapes(BODY),
    "ACOSquash6": FAR6 + _shapes(BODY),
    "meshSeqFromFile": _shapes(_plate(0, -2), BODY, _plate(0, 3)),
    "DCOFix": _shapes(_plate(0, -2), BODY),
    "DCOBallHitWall": _shapes(_plate(3), BODY),
    "DCOHammerWalnut": _shapes(BODY, "b1_1_1.msh 1 2 0  0 0 0  1 1 1"),
    "DCOCut": _shapes(BODY, _plate(0, 2)),
    "DCOSquash": _shapes(_plate(-2), _plate(2), BODY),
    "DCOSquash6": _shapes(*PLATES6, BODY),
    "DCORotCylinders": _shapes(_plate(-2), _plate(2), _plate(0, -2), _plate(0, 2), BODY),
    "DCOVerschoorRoller": _shapes(*PLATES6, BODY),
    "DCOSqueezeOut": _shapes(_plate(0, 2), BODY, _plate(0, -2)),
    "DCOSegBedSquash": _shapes(_plate(0, -2, ext="seg"), BODY, _plate(0, 2, ext="seg"), _plate(0, 4, ext="pt")),
    "curtain": _shapes("b14_2_1.msh 0 0 0  0 0 0  1 1 1"),
}
for _s in ("hang", "stampBoth", "stretch", "squash", "upndown", "stretchnsquash", "bend", "twistnstretch", "twistnsns", "twistnsns_old", "stretchAndPause"):
    SCENES[_s] = _shapes(WIDE)  # two different border sets
START_SCRIPTS = ("fall", "dragdown", "dragright", "stamp", "swing", "scaleF", "stampInv", "standInv", "twistnsns", "leftHitRight", "XYRotate", "DCOCut")
ROTATE = {"dragdown": "0 0 1 -3"}  # (at 30 degrees no node lies in the middle of the bottom tenth)

SHELL = "b1_1_1.obj 0 0 0  0 0 0  1 1 1 shell 0.01"
KEYWORDS = {
    "DBC and NBC boxes on a transformed shape": _shapes("b2_2_2.msh 1 2 3  10 20 30  2 1 0.5 DBC 0 0 0 1 0.1 1  0 -1 0  0 0 90  0.5 2.0 "
                                                        "DBC 0.9 0 0 1 1 1  1 0 0  0 0 0 NBC 0 0.9 0 1 1 1  0 0 5 NBC 0 0 0 1 1 0.1  1 0 0  0.25 0.75"),
    "DBC boxes that select nothing": _shapes(BODY + " DBC 2 2 2 3 3 3  0 0 0  0 0 0 NBC 2 2 2 3 3 3  0 0 1"),
    "linearVelocity and angularVelocity": _shapes(_plate(0, -2) + " linearVelocity 0 -1 0 angularVelocity 0 0 10", BODY, _plate(0, 3) + " angularVelocity 5 0 0",
                                                  "b1_1_1.msh 3 0 0  0 0 0  1 1 1 linearVelocity 1 0 0"),
    "initVel": _shapes(BODY + " initVel 1 0 0  0 0 90 DBC 0 0 0 1 0.1 1  0 0 0  0 0 0", "b1_1_1.msh 3 0 0  0 45 0  1 2 1 initVel 0 -1 0  10 0 0",
                       _plate(0, 3) + " linearVelocity 0 1 0 initVel 1 1 1  0 0 0"),
    "initVel under a script": "script drop\n" + _shapes(BODY + " initVel 1 0 0  0 0 90"),
    "material": _shapes(BODY + " material 500 2e5 0.3", "b1_1_1.msh 3 0 0  0 0 0  1 1 1 material 800 nan 0.3", "b1_1_1.msh 6 0 0  0 0 0  1 1 1"),
    "meshSeq on obj, seg and pt": _shapes("b1_1_1.obj 0 -2 0  0 0 0  1 1 1 meshSeq sq_1_1_1_obj", BODY, "b1_1_1.seg 0 3 0  0 0 0  1 1 1 meshSeq sq_1_1_1_seg",
                                          "b1_1_1.pt 3 0 0  0 0 0  1 1 1 meshSeq sq_1_1_1_pt linearVelocity 0 1 0"),
    "shell": _shapes(SHELL),
    "shell bend": _shapes(SHELL + " bend 0.5 material 900 3e5 0.35 DBC 0 0.9 0 1 1 1  0 0 0  0 0 0"),
    "shell limit": _shapes(SHELL + " limit 1.25 onset 1.0625 stiff 2"),
    "shell rubber": _shapes(SHELL + " rubber"),
    "shell rubber mr": _shapes(SHELL + " bend 2 rubber mr 0.25 limit 1.5"),
    "two shells, one limited": _shapes(SHELL + " limit 1.5", "b2_2_2.obj 3 0 0  0 0 0  1 1 1 shell 0.02 material 700 1e6 0.45"),
    "two shells, one rubber": _shapes(SHELL, "b2_2_2.obj 3 0 0  0 0 0  1 1 1 shell 0.02 rubber mr 0.5", BODY.replace("0 0 0", "0 3 0", 1)),
    "rod": _shapes("b1_1_1.seg 0 0 0  0 0 0  1 1 1 rod 0.01"),
    "two rods with bend, material and a DBC box": _shapes("b1_1_1.seg 0 0 0  0 0 0  1 1 1 rod 0.01 bend 0.5 material 900 3e5 0.35 DBC 0 0.9 0 1 1 1  0 0 0  0 0 0",
                                                          "b2_2_2.seg 3 0 0  0 0 30  1 1 1 rod 0.02 bend 0.5", BODY.replace("0 0 0", "0 3 0", 1)),
    "pressure on a shell": _shapes(SHELL + " pressure 100"),
    "pressure with ramp and gas on a shell": _shapes(SHELL + " pressure 100 ramp 0.5 gas 1000 gamma 1.4", "b2_2_2.obj 3 0 0  0 0 0  1 1 1 shell 0.02 pressure -5"),
    "pressure on a tetrahedral shape": _shapes(BODY + " pressure 50 gas 200", SHELL.replace("0 0 0", "3 0 0", 1) + " pressure 10 ramp 2"),
    "pressure on shapes with a mirroring scale": _shapes(SHELL.replace("1 1 1", "-1 1 2") + " pressure 100", BODY.replace("0 0 0", "3 0 0", 1).replace("1 1 1", "1 -1 1") + " pressure 7"),
    "attach and stitch": "attach 0 3 1 5 100 0.25\nattach 1 0 0 0 50\nstitch 0 1 1.25 10\n" + _shapes(BODY, "b1_1_1.msh 1.5 0 0  0 0 0  1 1 1"),
    "stitch with rest under size": "size 3\nattach 0 3 1 5 100 0.25\nstitch 0 1 1.25 10 rest\nstitch 1 0 0.75 20\n" + _shapes(BODY, "b1_1_1.msh 1.5 0 0  0 0 0  1 1 1"),
    "stitch with rest under size and rotateModel": "size 3\nrotateModel 0 0 1 30\nstitch 0 1 1.25 10 rest\n" + _shapes(BODY, SHELL.replace("0 0 0", "1.5 0 0", 1)),
    "a point shape beside a tetrahedral one": _shapes("b1_1_1.pt 0 3 0  0 0 0  1 1 1 linearVelocity 0 -1 0", BODY, "b1_1_1.msh 3 0 0  0 0 0  2 1 1"),
    "a point and a segment shape alone": "density 500\n" + _shapes("b1_1_1.pt 0 3 0  0 0 0  1 1 1 linearVelocity 0 -1 0", "b1_1_1.seg 0 0 0  0 0 0  1 2 1 angularVelocity 0 0 5",
                                                                  "b1_1_1.obj 3 0 0  0 0 0  1 2 1 linearVelocity 1 0 0"),
    "meshCO with rotate": "meshCO b1_1_1.obj 0.5 -1 0.5  2 0 0.3 rotate 10 20 30\nmeshCO b2_2_2.obj 0.5 -3 0.5  4 0 0\nselfCollisionOff\n" + _shapes(BODY),
    "meshCO under size and rotateModel": "meshCO b1_1_1.obj 0.5 -1 0.5  2 0 0 rotate 0 0 45\nsize 2\nrotateModel 1 0 0 20\nselfFric 0.2\n" + _shapes(BODY),
    "contactGroup and contactFric lines": "selfFric 0.1\ncontactIgnore 0 1\ncontactFric 1 2 0.4\ncontactFric 2 2 0\nmeshCO b1_1_1.obj 0.5 -3 0.5  4 0 0\n"
                                          + _shapes(BODY + " contactGroup 1", "b1_1_1.msh 3 0 0  0 0 0  1 1 1 contactGroup 2", "b1_1_1.msh 6 0 0  0 0 0  1 1 1"),
    "the other lines apply() reads": "energy FCR\ntimeIntegration NM 0.3 0.6\ntime 1 0.01\ndensity 800\nstiffness 2e5 0.3\nturnOffGravity\nground 0.5 -1\nhalfSpace 0 5 0  0 -2 0  1\n"
                                     "tuning 6\n1e4 2e-3 1e-3 1e-8\n2e-3 1e-3\nfricIterAmt 2\nDBCTimeRange 0.5 2\nNBCTimeRange 0.25 3\nuseAbsParameters\nkappaMinMultiplier 1e10\n"
                                     "dampingRatio 0.5\nwarmStart 3\ntol 1\n1e-3\nrestart status7\nscript twist\nhandleRatio 0.1\n"
                                     + _shapes(BODY + " DBC 0 0 0 1 0.1 1  0 0 0  0 0 0  1 1.5 NBC 0 0.9 0 1 1 1  0 0 5"),
}

REFUSALS = {
    "a codimensional shape that nothing moves": _shapes(_plate(0, -2), BODY),
    "a codimensional shape that nothing moves, before the ACO refusal": "script ACOSquash\n" + _shapes(_plate(0, -2), BODY),
    "a codimensional shape that nothing moves, under a hold script": "script stand\n" + _shapes(_plate(0, -2, ext="seg"), BODY),
    "meshSeq under a script": "script fall\n" + _shapes("b1_1_1.obj 0 -2 0  0 0 0  1 1 1 meshSeq sq_1_1_1_obj", BODY),
    "meshSeq on a tetrahedral shape": _shapes(BODY + " meshSeq sq_2_2_2_obj"),
    "ACOSquash with one plane": "script ACOSquash\nground 0 -1\n" + _shapes(BODY),
    "ACOSquash6 with five planes": "script ACOSquash6\n" + "".join(FAR6.splitlines(True)[:5]) + _shapes(BODY),
    "DCOSquash with too few components": "script DCOSquash\n" + _shapes(_plate(-2), _plate(2)),
    "DCOSquash6 with too few components": "script DCOSquash6\n" + _shapes(*PLATES6),
    "DCORotCylinders with too few components": "script DCORotCylinders\n" + _shapes(_plate(-2), BODY),
    "DCOVerschoorRoller with too few components": "script DCOVerschoorRoller\n" + _shapes(BODY),
    "DCOSquash with a surface it does not move": "script DCOSquash\n" + _shapes(_plate(-2), _plate(2), BODY, _plate(0, 3)),
    "DCOCut without a second component": "script DCOCut\n" + _shapes(BODY),
    "DCOHammerWalnut without a second component": "script DCOHammerWalnut\n" + _shapes(BODY),
    "DCOCut with a surface it does not move": "script DCOCut\n" + _shapes(BODY, _plate(0, 2), _plate(0, 4)),
    "meshSeqFromFile without a part": "script meshSeqFromFile sq_1_1_1_obj\n" + _shapes(BODY),
    "DCOSegBedSquash without a part": "script DCOSegBedSquash\n" + _shapes(BODY),
    "differing bend scales of shells": _shapes(SHELL + " bend 0.5", "b2_2_2.obj 3 0 0  0 0 0  1 1 1 shell 0.02"),
    "differing bend scales of rods": _shapes("b1_1_1.seg 0 0 0  0 0 0  1 1 1 rod 0.01 bend 0.5", "b2_2_2.seg 3 0 0  0 0 0  1 1 1 rod 0.02 bend 2"),
    "attach to a shape that does not exist": "attach 0 0 2 0 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "attach from a shape that does not exist": "attach -1 0 1 0 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "attach to a node that does not exist": "attach 0 0 1 27 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "attach from a node that does not exist": "attach 0 -1 1 0 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "attach of a node to itself": "attach 1 4 1 4 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "stitch to a shape that does not exist": "stitch 0 5 1 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "stitch of a shape to itself": "stitch 1 1 1 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "stitch that ties nothing": "stitch 0 1 0.5 10\n" + _shapes(BODY, BODY.replace("0 0 0", "3 0 0", 1)),
    "pressure on a shape without surface triangles": _shapes("n_b1_1_1.msh 0 0 0  0 0 0  1 1 1 pressure 5"),
    "pressure on an open surface": _shapes("open_b1_1_1.obj 0 0 0  0 0 0  1 1 1 shell 0.01 pressure 5"),
    "pressure on a surface that is not oriented": _shapes(BODY, "flip_b1_1_1.obj 3 0 0  0 0 0  1 1 1 shell 0.01 pressure 5"),
}


def cases():
    """{case name: scene text}, in the order of the fixture"""
    out = {}
    for s in script_names():
        head = f"script {s}" + (" sq_1_1_1_obj" if s == "meshSeqFromFile" else "") + "\n"
        out[f"script {s}"] = head + SCENES.get(s, _shapes(BODY))
        if s in START_SCRIPTS:
            out[f"script {s}, rotateModel"] = head + f"rotateModel {ROTATE.get(s, '0 0 1 30')}\n" + SCENES.get(s, _shapes(BODY))
            out[f"script {s}, size"] = head + "size 3\n" + SCENES.get(s, _shapes(BODY))
        if s in ("fall", "dragdown", "dragright", "twistnsns", "stampInv"):
            out[f"script {s}, rotateModel and size"] = head + "size 0.75\nrotateModel 0.6 0 0.8 40\n" + SCENES.get(s, _shapes(BODY))
    out["script ACOSquash, planes that are close"] = "script ACOSquash\nhalfSpace 0.46875 0 0  1 0 0  1 0\nhalfSpace 0.5 0 0  -1 0 0  1 0\n" + _shapes(BODY)
    out["script DCOBallHitWall with a speed"] = "script DCOBallHitWall 1 250\n" + SCENES["DCOBallHitWall"]
    out["script DCOFix with nothing to hold"] = "script DCOFix\n" + _shapes(BODY + " DBC 0 0 0 1 0.1 1  0 0 0  0 0 0")
    out["script fall over DBC and NBC boxes"] = "script fall\n" + _shapes(BODY + " DBC 0 0 0 1 0.1 1  0 0 0  0 0 0 NBC 0 0.9 0 1 1 1  0 0 5")
    out["script NMFixBottomDragLeft over DBC and NBC boxes"] = "script NMFixBottomDragLeft\n" + _shapes(BODY + " DBC 0 0 0 1 0.1 1  0 0 0  0 0 0 NBC 0 0.9 0 1 1 1  0 0 5")
    out["script dragdown beside a moved surface"] = "script dragdown\nrotateModel 0 0 1 -3\n" + _shapes(BODY, "b2_2_2.obj 0 -2 0  0 0 0  1 1 1 linearVelocity 0 1 0")
    out["script dragright beside a moved surface"] = "script dragright\nrotateModel 0 0 1 30\nmeshCO b1_1_1.obj 0.5 -1 0.5  0.5 0 0\n" + _shapes(BODY, _plate(0, -2) + " linearVelocity 0 1 0")
    out["script dragright without an obstacle"] = "script dragright\n" + _shapes(BODY)
    out["script DCOSegBedSquash with lower parts only"] = "script DCOSegBedSquash\n" + _shapes(_plate(0, -2, ext="seg"), BODY, BODY.replace("0 0 0", "3 0 0", 1))
    out.update({f"keyword: {k}": v for k, v in KEYWORDS.items()})
    out.update({f"refusal: {k}": v for k, v in REFUSALS.items()})
    return out


# ---- recording -------------------------------------------------------------------------------------------------------------------------------------------
def positions(sc, r0, k):
    """the positions before_step() finds in step k: the start positions, in the steps of PUSH with the deciding nodes of the rule beyond its threshold"""
    X = np.array(sc.V if sc.V0 is None else sc.V0, dtype=np.float64)
    if r0 is None or not PUSH[k]:
        return X
    kind, nr = r0.get("kind", "dragright"), sc.node_ranges
    if kind == "turn":
        X[r0["turn"], r0["axis"]] = r0["hi"] + 1e-3 if k == 4 and np.isfinite(r0["hi"]) else r0["lo"] - 1e-3
    elif kind == "let_go":
        X[r0["turn"], r0["axis"]] = r0["limit"] + (-1e-3 if r0["below"] else 1e-3)
    elif kind == "pause":
        X[r0["turn"], 0] = r0["x_limit"] - 1e-3
    elif kind == "dragright" and np.isfinite(r0["x_limit"]):
        X[:r0["nSim"], 0] += r0["x_limit"] - X[:r0["nSim"], 0].min() + 1e-3
    elif kind == "dco":
        X[nr[1]:nr[2], 0] += X[nr[0]:nr[1], 0].max() + 0.05 - X[nr[1]:nr[2], 0].min()
    elif kind == "segbed" and len(r0["down"]):
        X[r0["up"], 1] += X[r0["down"], 1].max() + 0.05 - X[r0["up"], 1].min()
    elif kind == "while_above":
        X[r0["ids"], 1] += r0["y"] - 5e-4 - X[r0["ids"], 1].min()
    return X


@contextlib.contextmanager
def _chdir(folder):
    old = os.getcwd()
    os.chdir(folder)
    try:
        yield
    finally:
        os.chdir(old)


def record(text):
    """the fixture entry of one scene text"""
    with tempfile.TemporaryDirectory() as tmp, _chdir(tmp):  # (relative paths: no folder name of this run gets into the record)
        write_files(text, tmp)
        try:
            sc = ss.assemble(ss.SceneConfig.parse(text, "."), read_mesh)
        except (ss.UnsupportedKeyword, ValueError) as e:
            return {"error": [type(e).__name__, str(e)]}
        out = {"scene": sd.dump(sc), "apply": sd.dump_apply(sc)}
        if sc.release is not None or sc.mesh_seqs:
            r0 = None if sc.release is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.release.items()}
            be, out["steps"] = sd.Recorder(), []
            for k in range(STEPS):
                be.V, n = positions(sc, r0, k), len(be.calls)
                ret = sc.before_step(be, k * sc.cfg.dt)
                out["steps"].append({"ret": sd.dump(ret, "ret"), "calls": be.calls[n:], "release": sd.dump(sc.release, "release"), "mesh_i": sc.mesh_i})
        return out


def entry(rec):
    """What the fixture keeps of a record: a refusal as it is; else the digest of the scene, of the calls of apply() and of each driven step -- the dumps
    themselves would be 700 KB -- beside two figures a reader can check by eye, the sizes of the Dirichlet groups and which steps told the backend something.
    Where a digest differs, `--dump CASE` on the two commits prints the records to compare."""
    if "error" in rec:
        return rec
    groups = [int(np.prod(v["shape"])) for k, v in rec["scene"].items() if re.fullmatch(r"dirichlet\[\d+\]\(0\)", k)]
    out = {"groups": groups, "scene": sd.digest(rec["scene"]), "apply": sd.digest(rec["apply"])}
    if "steps" in rec:
        out["fired"] = [s["ret"]["ret"] for s in rec["steps"]]
        out["steps"] = sd.digest(rec["steps"])
    return out


def main():
    if "--dump" in sys.argv:  # the whole record of one case, one name a line
        print(json.dumps(record(cases()[sys.argv[sys.argv.index("--dump") + 1]]), indent=0))
        return
    out = {name: entry(record(text)) for name, text in cases().items()}
    if "--list" in sys.argv:
        for name, e in out.items():
            print(f"{name:70s} {e['error'] if 'error' in e else (e['groups'], e.get('fired'))}")
        return
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in out.items()) + "\n}\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(out), "cases")


if __name__ == "__main__":
    main()
