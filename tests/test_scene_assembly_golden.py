"""ipc_amd/scene_script.py against tests/golden/scene_assembly.json, the record tools/make_scene_assembly_golden.py took of it: for every script name the
parser accepts, for the shape keywords and for every refusal of assemble() the assembled scene, the backend calls of apply() and six driven calls of
before_step() are rebuilt and compared by equality -- floats by their float.hex(), large arrays by their SHA-256 (tests/scene_dump.py), each dump by the
SHA-256 of its JSON spelling.  Where a digest differs, `python tools/make_scene_assembly_golden.py --dump "<case>"` prints the record to compare.  No GPU."""
import importlib.util
import json
import os

import pytest

from ipc_amd import scene_script as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_scene_assembly_golden", os.path.join(ROOT, "tools", "make_scene_assembly_golden.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

CASES = tool.cases()
with open(tool.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_assembled_applied_and_stepped_as_recorded(name):
    got, want = tool.entry(tool.record(CASES[name])), GOLDEN[name]
    assert list(got) == list(want)
    for part in want:
        assert got[part] == want[part], part


def test_every_script_name_has_a_case_and_every_case_a_record():
    names = ss.HOLD_SCRIPTS + ss.PULL_SCRIPTS + ss.INITVEL_SCRIPTS + ss.RULE_SCRIPTS + ss.HANDLE_SCRIPTS + tuple(ss.DCO_SCRIPTS) + tool.script_literals()
    assert {"null", "twist", "fall", "DCOCut", "stretchAndPause"} <= set(tool.script_literals())
    for s in names:
        ss.SceneConfig.parse(f"script {s} folder\n" if s == "meshSeqFromFile" else f"script {s}\n")  # the parser accepts it
        assert f"script {s}" in CASES and "scene" in GOLDEN[f"script {s}"], s
    assert list(GOLDEN) == list(CASES)  # no case without a record, none skipped
    assert sum("error" in v for v in GOLDEN.values()) == len(tool.REFUSALS)
    assert all(len(v["fired"]) == tool.STEPS for v in GOLDEN.values() if "steps" in v)
