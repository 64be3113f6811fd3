"""Host side of the contact groups (`ipcgpu_set_contact_groups`): validation of the tables and the per-node packed words of
`ipc_amd/csrc/contact_groups.cpp`, run as a stand-alone program (`tests/contact_groups/main.cpp`) and compared with words packed by hand; the same
program once more under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ipc_amd", "csrc")
SRCS = [os.path.join(HERE, "contact_groups", "main.cpp"), os.path.join(CSRC, "contact_groups.cpp")]
DEFAULT_WORD = 0xFFFF0000


def _build(name, extra):
    exe = os.path.join(HERE, "contact_groups", "_build", name)
    deps = SRCS + [os.path.join(CSRC, "contact_groups.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}"] + extra + SRCS + ["-o", exe])
    return exe


def case(nV, ends, groups, collide, scale=None, null_tables=False):
    return dict(nV=nV, ends=list(ends), groups=list(groups), collide=np.asarray(collide), scale=None if scale is None else np.asarray(scale, dtype=float),
                null_tables=null_tables)


def _run(exe, cases):
    """per case None-with-reason (rejected: a str) or (words[nV] uint32, scale[16, 16])"""
    text = ""
    for c in cases:
        n = c["collide"].shape[0]
        t = [c["nV"], len(c["ends"])] + c["ends"] + [len(c["groups"])] + c["groups"]
        if c["null_tables"]:
            t += [-n, 0]
        else:
            t += [n] + [int(x) for x in c["collide"].ravel()]
            t += [0] if c["scale"] is None else [1] + [repr(float(x)) for x in c["scale"].ravel()]
        text += " ".join(str(x) for x in t) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    res = []
    for line, c in zip(out, cases):
        if line.startswith("0 "):
            res.append(line[2:])
            continue
        a = line.split()
        assert a[0] == "1" and len(a) == 1 + c["nV"] + 256
        res.append((np.array(a[1:1 + c["nV"]], dtype=np.uint64).astype(np.uint32), np.array(a[1 + c["nV"]:], dtype=float).reshape(16, 16)))
    return res


@pytest.fixture(scope="module")
def packer():
    exe = _build("contact_groups_main", [])
    return lambda cases: _run(exe, cases)


def pack_by_hand(c):
    """the layout of include/ipcgpu.h: bits 4-7 the group, bits 16-31 the group's row of collide, everything else 0"""
    words = np.zeros(c["nV"], dtype=np.uint32)
    v0 = 0
    for end, g in zip(c["ends"], c["groups"]):
        row = sum(int(c["collide"][g, h]) << h for h in range(c["collide"].shape[0]))
        words[v0:end] = (g << 4) | (row << 16)
        v0 = end
    scale = np.ones((16, 16))
    if c["scale"] is not None:
        n = c["collide"].shape[0]
        scale[:n, :n] = c["scale"]
    return words, scale


def good_cases():
    full16 = np.ones((16, 16), dtype=int)
    checker = np.array([[(g + h) % 3 != 0 or g == h for h in range(16)] for g in range(16)], dtype=int)
    checker = checker & checker.T
    rng = np.random.default_rng(3)
    s16 = rng.uniform(0, 2, size=(16, 16))
    s16 = 0.5 * (s16 + s16.T)
    return {
        "one component, one group": case(5, [5], [0], [[1]]),
        "one group that does not collide with itself": case(4, [4], [0], [[0]]),
        "three bodies, A-B off, scales": case(10, [3, 7, 10], [0, 1, 2], [[1, 0, 1], [0, 1, 1], [1, 1, 1]], [[1, 0.25, 0], [0.25, 1, 1], [0, 1, 0.5]]),
        "two components share a group; an empty component": case(9, [2, 2, 6, 9], [1, 0, 1, 0], [[1, 1], [1, 0]]),
        "groups in another order than the components": case(6, [1, 2, 6], [2, 0, 1], [[0, 1, 0], [1, 1, 1], [0, 1, 1]]),
        "sixteen groups, all on": case(32, list(range(2, 34, 2)), list(range(16)), full16),
        "sixteen groups, a pattern, scales": case(48, list(range(3, 51, 3)), list(range(15, -1, -1)), checker, s16),
        "a scale of zero on the diagonal": case(3, [3], [0], [[1]], [[0.0]]),
        "no node": case(0, [0], [0], [[1]]),
    }


def bad_cases():
    ok = dict(nV=6, ends=[2, 6], groups=[0, 1], collide=[[1, 0], [0, 1]], scale=[[1, 0.5], [0.5, 1]])

    def but(**kw):
        d = dict(ok)
        d.update(kw)
        return case(**d)

    return {
        "nComp differs from the component table": but(groups=[0, 1, 1]),
        "one group for a table of two": but(groups=[0]),
        "no component table": but(ends=[]),
        "table that does not end at nV": but(ends=[2, 5]),
        "table that decreases": but(ends=[7, 6]),
        "group 16": case(6, [2, 6], [0, 16], np.ones((16, 16), dtype=int)),
        "group == nGroups": but(groups=[0, 2]),
        "negative group": but(groups=[-1, 1]),
        "seventeen groups": case(6, [2, 6], [0, 1], np.ones((17, 17), dtype=int)),
        "collide not symmetric": but(collide=[[1, 1], [0, 1]]),
        "collide entry 2": but(collide=[[1, 2], [2, 1]]),
        "scale not symmetric": but(scale=[[1, 0.5], [0.25, 1]]),
        "negative scale": but(scale=[[1, -0.5], [-0.5, 1]]),
        "infinite scale": but(scale=[[float("inf"), 0.5], [0.5, 1]]),
        "NaN scale": but(scale=[[1, 0.5], [0.5, float("nan")]]),
        "null tables": but(null_tables=True),
    }


def check_good(c, got):
    assert not isinstance(got, str), got
    words, scale = got
    want_w, want_s = pack_by_hand(c)
    assert np.array_equal(words, want_w) and np.array_equal(scale, want_s)
    assert np.all(words & 0xFF0F == 0)  # bits 0-3 and 8-15 belong to the kernel's own flags / stay clear
    n = c["collide"].shape[0]
    # what pair_filtered reads: bit 16 + group(b) of a's word, for every pair of nodes
    grp = (words >> 4) & 15
    for a in range(c["nV"]):
        for b in range(c["nV"]):
            assert (int(words[a]) >> (16 + int(grp[b]))) & 1 == c["collide"][grp[a], grp[b]]
    assert np.all(grp < n)


def test_packed_words_for_hand_written_tables(packer):
    G = good_cases()
    for (name, c), got in zip(G.items(), packer(list(G.values()))):
        check_good(c, got)
    w, s = packer([G["three bodies, A-B off, scales"]])[0]
    assert [hex(x) for x in w[[0, 3, 7]]] == ["0x50000", "0x60010", "0x70020"]
    assert s[0, 1] == 0.25 and s[1, 0] == 0.25 and s[0, 2] == 0.0 and s[2, 2] == 0.5 and s[3, 3] == 1.0 and s[0, 3] == 1.0


def test_default_word_is_group_zero_colliding_with_every_group(packer):
    """A table of one group that collides with itself differs from the default word only in the rows of groups that do not exist; the default (the
    word of a context without a table, `CONTACT_GROUP_DEFAULT_WORD`) is group 0 with an all-ones row, so no pair is ever filtered by it."""
    w, s = packer([case(7, [7], [0], [[1]])])[0]
    assert np.all(w == 0x00010000) and np.all(s == 1.0)
    w16, _ = packer([case(7, [7], [0], np.ones((16, 16), dtype=int))])[0]
    assert np.all(w16 == DEFAULT_WORD)
    hdr = open(os.path.join(CSRC, "contact_groups.h")).read()
    assert "CONTACT_GROUP_DEFAULT_WORD = 0xFFFF0000u" in hdr
    assert (DEFAULT_WORD >> 4) & 15 == 0 and all((DEFAULT_WORD >> (16 + h)) & 1 for h in range(16))


def test_every_validation_error_is_reported(packer):
    B = bad_cases()
    res = packer(list(B.values()))
    for name, got in zip(B, res):
        assert isinstance(got, str) and got.startswith("contact groups:"), (name, got)
    assert "symmetric" in res[list(B).index("collide not symmetric")] and "symmetric" in res[list(B).index("scale not symmetric")]
    assert "component" in res[list(B).index("nComp differs from the component table")]
    assert "16" in res[list(B).index("seventeen groups")]


def test_same_program_under_address_and_undefined_behaviour_sanitizers():
    exe = _build("contact_groups_main_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    G, B = good_cases(), bad_cases()
    res = _run(exe, list(G.values()) + list(B.values()))
    for c, got in zip(G.values(), res):
        check_good(c, got)
    assert all(isinstance(r, str) for r in res[len(G):])
