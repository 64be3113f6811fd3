"""The launch plan of the multifrontal solver (`ipc_amd/csrc/mf_plan.cpp`: which front takes which kernel, and every descriptor record the factorisation and the
sweeps read), run on the host through `tests/mf_symbolic/shim.cpp` and read here the way the kernels read it: every front, tile, panel and block must be covered
exactly once.  No GPU.

The case: `stacked_pattern(13)`, two 13 x 13 sheets with contact pairs, 676 nodes -- the smallest n for which the default tuning gives a level with two or more
fronts of the multi-workgroup path (n = 13: 11, 7, 4, 3, 2, 1 of them on levels 2 .. 7) AND a front with nc >= 192 (n = 13: one, nc = 195; n = 12 has none, 144).
The dissection tree is binary, so no front has more than FUSED_MAX_KIDS children: the chained records are walked for what there is (chains of one)."""
import ctypes as C

import numpy as np
import pytest

from test_mf_symbolic import analyze, shim, stacked_pattern  # noqa: F401  (shim: the module's fixture, it builds the library)

N_CASE = 13
NB, TS, ROWS_B, MV_ROWS, FD, MAX_KIDS = 32, 64, 96, 32, 64, 8  # geometry of mf_plan.h
TUNE = ("fusedLds", "ntBigN", "xinvMin", "borderMaxNc", "schur64Min", "bulkMinMB", "bulkBlock")
XINV_MIN = 192
LEVEL_FIELDS = ("small", "bigFronts", "ea", "schur", "fwdRect", "bwdInit", "bigTri", "xinvFwd", "xinvBwd")


@pytest.fixture(scope="module")
def sym(shim):  # noqa: F811
    V, G, ia, ja = stacked_pattern(N_CASE)
    o = analyze(shim, ia, ja, V, leaf=8)
    o["N"] = 3 * np.diff(o["idxPtr"])
    o["nc"] = 3 * np.diff(o["firstNode"])
    o["kids"] = [o["child"][o["childPtr"][s]:o["childPtr"][s + 1]].tolist() for s in range(o["ns"])]
    return o


def make_plan(shim, sym, world=1, rank=0, **tune):  # noqa: F811
    """both planner steps on the shim's analysis; the arrays come back as int64, records as rows of four"""
    shim.shim_plan_fetch.restype = C.c_longlong
    t = np.array([float(tune.pop(k)) if k in tune else np.nan for k in TUNE])
    assert not tune
    err = C.create_string_buffer(256)
    assert shim.shim_plan(C.c_int(world), C.c_int(rank), t.ctypes.data_as(C.c_void_p), err, C.c_int(256)) == 0, err.value

    def fetch(name):
        n = shim.shim_plan_fetch(name.encode(), None)
        assert n >= 0, name
        a = np.zeros(max(n, 1), np.int64)
        shim.shim_plan_fetch(name.encode(), a.ctypes.data_as(C.c_void_p))
        return a[:n]
    p = {k: fetch(k) for k in ("symLevel", "symInvPtr", "bucketStart", "fused", "smallList", "bigList", "eaTileBase", "eaColTiles", "nodeFront", "dinvOff", "owner",
                               "exec", "aPtr", "eaAPtr", "bigFd", "fdesc", "xinvOff", "triList", "scalars")}
    for k in ("frontInfo", "xchgDesc", "ea", "desc", "xinvDesc"):
        p[k] = fetch(k).reshape(-1, 4)
    lv = fetch("levels").reshape(-1, 30)
    steps, bulks = fetch("steps").reshape(-1, 2), fetch("bulks").reshape(-1, 2)
    p["levels"], at = [], 0
    for row in lv:
        L = {k: (int(row[2 * i]), int(row[2 * i + 1])) for i, k in enumerate(LEVEL_FIELDS)}
        L.update(smallLds=int(row[18]), solveLds=int(row[19]), triLds=int(row[20]), bwdLds=int(row[21]), smallThreads=int(row[22]), schur64=bool(row[23]),
                 stepTop=bool(row[24]), fuseEA=bool(row[25]))
        n = int(row[26])
        L["step"], L["bulk"] = steps[at:at + n].tolist(), bulks[at:at + n].tolist()
        at += n
        p["levels"].append(L)
    xl, at = fetch("xinvLevels"), 0
    p["xinvLevels"] = []
    for _ in lv:
        n = int(xl[at + 4])
        p["xinvLevels"].append(dict(blocks=tuple(xl[at:at + 2]), init=tuple(xl[at + 2:at + 4]), rounds=xl[at + 5:at + 5 + 4 * n].reshape(-1, 4).tolist()))
        at += 5 + 4 * n
    assert at == len(xl)
    p["xchg"] = []
    if world > 1:
        xc, at = fetch("xchgLevels"), 0
        for _ in lv:
            X = dict(pack=tuple(xc[at:at + 2]), unpack=tuple(xc[at + 2:at + 4]), count=int(xc[at + 4]), countW=int(xc[at + 5]))
            at += 6
            for k in ("opsM", "opsW", "opsX"):
                n = int(xc[at])
                X[k] = xc[at + 1:at + 1 + 4 * n].reshape(-1, 4).tolist()
                at += 1 + 4 * n
            p["xchg"].append(X)
        assert at == len(xc)
    p["world"], p["rank"] = world, rank
    p["xinvMin"] = int(t[2]) if not np.isnan(t[2]) else XINV_MIN
    p["borderMaxNc"] = int(t[3]) if not np.isnan(t[3]) else 1536
    p["bulkBlock"] = int(t[6]) if not np.isnan(t[6]) else 256
    return p


def span(p, rng):
    return range(rng[0], rng[0] + rng[1])


def big_of(p, L):
    return [int(p["bigList"][i]) for i in span(p, L["bigFronts"])]


def off64(lo, hi):
    return (int(hi) << 32) | (int(lo) & 0xffffffff)


def front_of_geometry(sym, rec):
    """the front a (N, nc-or-E, offset lo, offset hi) record belongs to"""
    s = int(np.searchsorted(sym["frontOff"], off64(rec[2], rec[3])))
    assert sym["frontOff"][s] == off64(rec[2], rec[3]) and sym["N"][s] == rec[0]
    return s


def check_front_placement(sym, p):
    """every front this rank executes: exactly once, in smallList or bigList, inside its level's range; returns the executed fronts"""
    seen = []
    atS = atB = 0
    for l, L in enumerate(p["levels"]):
        assert L["small"][0] == atS and L["bigFronts"][0] == atB  # the ranges tile the lists
        atS, atB = atS + L["small"][1], atB + L["bigFronts"][1]
        small, big = [int(p["smallList"][i]) for i in span(p, L["small"])], big_of(p, L)
        for s in small + big:
            assert p["symLevel"][s] == l and p["exec"][s] == p["rank"]
        assert all(p["fused"][s] for s in small) and not any(p["fused"][s] for s in big)
        assert L["smallThreads"] in (256, 512)
        seen += small + big
    mine = [s for s in range(sym["ns"]) if p["world"] == 1 or p["exec"][s] == p["rank"]]
    assert sorted(seen) == mine
    for s in range(sym["ns"]):
        assert p["frontInfo"][s][0] == (-1 if s not in set(mine) else (0 if p["fused"][s] else 1))
    return mine


def first_records(sym, p):
    """front -> its first packed record, from the extend-add descriptors (every big front has tile (0, 0))"""
    rec = {}
    for L in p["levels"]:
        for i in span(p, L["ea"]):
            r, ti, tj, _ = p["ea"][i]
            if ti == 0 and tj == 0:
                d = p["bigFd"][FD * r:FD * r + FD]
                rec[front_of_geometry(sym, (d[2], d[3], d[0], d[1]))] = int(r)
    return rec


def check_extend_add_and_records(sym, p):
    recOf = first_records(sym, p)
    at, nFused = 0, 0
    for L in p["levels"]:
        assert L["ea"][0] == at
        at += L["ea"][1]
        want = []
        for s in big_of(p, L):
            nt = -(-sym["N"][s] // TS)
            want += [(recOf[s], ti, tj) for ti in range(nt) for tj in range(ti + 1) if not (L["fuseEA"] and TS * tj >= sym["nc"][s])]
            if L["fuseEA"]:
                nFused += sum(1 for ti in range(nt) for tj in range(ti + 1) if TS * tj >= sym["nc"][s])
        got = [tuple(int(x) for x in p["ea"][i][:3]) for i in span(p, L["ea"])]
        assert sorted(got) == sorted(want) and len(set(got)) == len(got)  # each lower-triangle tile once; on a fused level exactly the update-only tiles are absent
        for i in span(p, L["ea"]):
            assert p["ea"][i][3] == i  # record i carries tile number i
    assert at == p["scalars"][0] and len(p["eaAPtr"]) == at + 1
    assert np.array_equal(p["eaAPtr"], p["bucketStart"][sym["ns"]:] - p["bucketStart"][sym["ns"]])
    # chained records: every child once, the chain ends with -1
    for s, r in recOf.items():
        kids, hops = [], 0
        while r >= 0:
            d = p["bigFd"][FD * r:FD * r + FD]
            assert off64(d[0], d[1]) == sym["frontOff"][s] and d[2] == sym["N"][s] and d[3] == sym["nc"][s] and 0 <= d[8] <= MAX_KIDS
            for q in range(int(d[8])):
                k = d[16 + 6 * q:22 + 6 * q]
                c = front_of_geometry(sym, (k[2], k[3], k[0], k[1]))
                assert k[3] == sym["nc"][c] and k[4] == p["symInvPtr"][c]
                kids.append(c)
            r, hops = int(d[9]), hops + 1
        assert kids == sym["kids"][s] and hops == max(1, -(-len(kids) // MAX_KIDS))
    assert sorted(recOf) == sorted(s for L in p["levels"] for s in big_of(p, L))
    return recOf, nFused


def check_fused_records(sym, p):
    n = sum(L["small"][1] for L in p["levels"])
    assert len(p["fdesc"]) == FD * max(n, 1)
    assert np.array_equal(p["aPtr"], p["bucketStart"][:sym["ns"] + 1])
    for i in range(n):
        s, d = int(p["smallList"][i]), p["fdesc"][FD * i:FD * i + FD]
        assert off64(d[0], d[1]) == sym["frontOff"][s] and d[2] == sym["N"][s] and d[3] == sym["nc"][s]
        assert off64(d[4], d[5]) == p["dinvOff"][s] == sum(-(-int(c) // NB) for c in sym["nc"][:s])
        assert d[6] == p["bucketStart"][s] and d[7] == p["bucketStart"][s + 1]
        assert d[8] == len(sym["kids"][s]) <= MAX_KIDS
        for q, c in enumerate(sym["kids"][s]):
            k = d[16 + 6 * q:22 + 6 * q]
            assert off64(k[0], k[1]) == sym["frontOff"][c] and k[2] == sym["N"][c] and k[3] == sym["nc"][c] and k[4] == p["symInvPtr"][c]
    return n


def check_step_launches(sym, p):
    """per big front: cover[q][r, c] = how often the update of panel q reaches entry (r, c) of the own columns -- 1 on the lower triangle behind the panel"""
    nBulk = nRoleC = 0
    for L in p["levels"]:
        big = big_of(p, L)
        if not big:
            assert L["step"] == [] and L["bulk"] == []
            continue
        assert len(L["step"]) == max(-(-sym["nc"][s] // NB) for s in big) + 1 == len(L["bulk"])
        cover = {s: np.zeros((-(-sym["nc"][s] // NB), sym["N"][s], sym["nc"][s]), np.int8) for s in big}
        for launch, (R, U) in enumerate(zip(L["step"], L["bulk"])):
            j = launch - 1
            kb, kb1 = NB * j, NB * (j + 1)  # the panel this launch applies, the panel it factors
            rows = {s: [] for s in big}
            roleC = {s: [] for s in big}
            for w in range(R[1]):
                a, b = p["desc"][R[0] + 2 * w], p["desc"][R[0] + 2 * w + 1]
                s = front_of_geometry(sym, b)
                N, nc = sym["N"][s], sym["nc"][s]
                assert s in cover and kb1 < nc + NB
                if a[3] == -2:  # role B: rows [kb1 + r0, + ROWS_B) of panel kb1, updated by panel kb unless the bulk launch has done that
                    assert a[0] == p["dinvOff"][s] and b[1] == nc and kb1 < nc
                    rows[s].append(int(a[2]))
                    assert a[1] in ((-1,) if j < 0 else (kb, -2 - kb1))
                    if a[1] == kb:
                        cover[s][j, kb1 + a[2]:min(kb1 + a[2] + ROWS_B, N), kb1:min(kb1 + NB, nc)] += 1
                elif a[3] == -6:  # role C: panel kb of the inverse, 16-column tile c0
                    assert a[0] == s and a[1] == kb and j >= 0 and b[1] == nc and L["stepTop"]
                    roleC[s].append(int(a[2]))
                else:  # role A: panel kb onto trailing tile (ti, tj) behind the next panel, columns below E = b[1]
                    assert a[0] == p["dinvOff"][s] and a[1] == kb and j >= 0 and b[1] <= nc
                    M0 = min(kb1 + NB, nc)
                    r0, c0 = M0 + TS * a[2], M0 + TS * a[3]
                    assert a[3] <= a[2] and r0 < N and c0 < b[1]
                    cover[s][j, r0:min(r0 + TS, N), c0:min(c0 + TS, b[1])] += 1
            for s in big:
                N, nc = sym["N"][s], sym["nc"][s]
                assert rows[s] == (list(range(0, N - kb1, ROWS_B)) if kb1 < nc else [])  # rows [kb1, N) once, in pieces of ROWS_B
                bordered = XINV_MIN <= nc and p["xinvMin"] <= nc <= p["borderMaxNc"]
                assert roleC[s] == (list(range(0, kb + 1, 16)) if bordered and 0 <= kb < nc else [])
                nRoleC += len(roleC[s])
            for w in range(U[1]):  # bulk: the panels of outer block [a[1], a[1] + a[0]) onto tile (ti, tj) behind the block
                a, b = p["desc"][U[0] + 2 * w], p["desc"][U[0] + 2 * w + 1]
                s = front_of_geometry(sym, b)
                N, nc = sym["N"][s], sym["nc"][s]
                Eb = int(a[0] + a[1])
                assert a[0] == p["bulkBlock"] and Eb == kb1 + NB and Eb % a[0] == 0 and Eb < nc and b[1] == nc and a[3] <= a[2]
                r0, c0 = Eb + 64 * a[2], Eb + 64 * a[3]
                assert r0 < N and c0 < nc
                cover[s][a[1] // NB:Eb // NB, r0:min(r0 + 64, N), c0:min(c0 + 64, nc)] += 1
                nBulk += 1
        for s in big:
            N, nc = sym["N"][s], sym["nc"][s]
            r, c = np.arange(N)[:, None], np.arange(nc)[None, :]
            for q in range(cover[s].shape[0]):
                behind = (c >= min(NB * (q + 1), nc)) & (r >= c)
                assert np.array_equal(cover[s][q][behind], np.ones(int(behind.sum()), np.int8)), (s, q)
                assert not cover[s][q][(c < NB * (q + 1)) & (r >= c)].any()
    return nBulk, nRoleC


def check_schur(sym, p, recOf):
    n = 0
    for L in p["levels"]:
        T = 64 if L["schur64"] else 32
        want = []
        for s in big_of(p, L):
            nt = -(-(sym["N"][s] - sym["nc"][s]) // T)
            want += [(s, ti, tj, recOf[s] if L["fuseEA"] else 0) for ti in range(nt) for tj in range(ti + 1)]  # front after front
        got = []
        for w in range(L["schur"][1]):
            a, b = p["desc"][L["schur"][0] + 2 * w], p["desc"][L["schur"][0] + 2 * w + 1]
            assert front_of_geometry(sym, b) == a[0] and b[1] == sym["nc"][a[0]]
            got.append(tuple(int(x) for x in a))
        assert sorted(got) == sorted(want) and len(set(got)) == len(got)  # a permutation of the front-after-front enumeration
        n += len(got)
        # the rectangle below the triangle in the sweeps
        assert [tuple(p["desc"][i][:2]) for i in span(p, L["fwdRect"])] == [(s, r0) for s in big_of(p, L) for r0 in range(0, sym["N"][s] - sym["nc"][s], MV_ROWS)]
        assert [tuple(p["desc"][i][:2]) for i in span(p, L["bwdInit"])] == [(s, c0) for s in big_of(p, L) if sym["N"][s] > sym["nc"][s] for c0 in range(0, sym["nc"][s], 16)]
    return n


def check_inverses(sym, p):
    """returns (fronts with an inverse, doubling GEMM records)"""
    xd, nc = p["xinvDesc"], sym["nc"]
    inv, nGemm, at = [], 0, 0
    for L, X in zip(p["levels"], p["xinvLevels"]):
        big = big_of(p, L)
        withInv = [s for s in big if nc[s] >= p["xinvMin"]]
        for s in withInv:  # a range of nc^2 in X, one after the other
            assert p["xinvOff"][s] == at
            at += int(nc[s]) ** 2
        assert all(p["xinvOff"][s] == -1 for s in big if s not in withInv)
        assert [int(p["triList"][i]) for i in span(p, L["bigTri"])] == [s for s in big if s not in withInv]  # everybody else: one workgroup sweeps the triangle
        assert L["triLds"] == 8 * max([1] + [nc[s] for s in big if s not in withInv])
        doubling = [s for s in withInv if nc[s] > p["borderMaxNc"]]  # (the bordered ones: role C of the step launches, check_step_launches)
        assert L["stepTop"] == any(nc[s] <= p["borderMaxNc"] for s in withInv)
        assert [tuple(xd[i][:2]) for i in span(p, X["init"])] == [(s, b) for s in doubling for b in range(-(-nc[s] // NB))]  # the diagonal blocks
        assert X["blocks"][1] == X["init"][1]
        sz, lvlMax = NB, max([0] + [nc[s] for s in doubling])
        for g1, g2 in [(r[:2], r[2:]) for r in X["rounds"]]:
            assert sz < lvlMax
            for mode, g in ((1, g1), (2, g2)):
                got = [(tuple(xd[2 * w]), tuple(xd[2 * w + 1])) for w in span(p, g)]
                want = []
                for s in doubling:
                    edges = []
                    for a0 in range(0, nc[s], 2 * sz):  # pairs A = [a0, a0 + sz), C = [a0 + sz, cEnd): together with a last lone A they tile [0, nc)
                        cEnd = min(a0 + 2 * sz, nc[s])
                        edges.append((a0, min(a0 + sz, nc[s]), cEnd))
                        if a0 + sz < nc[s]:
                            want += [((s, r, c, mode), (cEnd, a0 + sz, a0, a0 + sz) if mode == 1 else (cEnd, a0 + sz, a0 + sz, cEnd))
                                     for r in range(a0 + sz, cEnd, 32) for c in range(a0, a0 + sz, 32)]
                    assert edges[0][0] == 0 and edges[-1][2] == nc[s] and all(e[2] == f[0] for e, f in zip(edges, edges[1:]))
                assert got == want
                nGemm += len(got)
            sz *= 2
        assert sz >= lvlMax  # doubled until one block spans the widest front
        assert L["xinvFwd"][0] % 2 == 0  # (the sweep lists start on a pair boundary: the GEMM records in front of them are pairs)
        assert [tuple(xd[i][:2]) for i in span(p, L["xinvFwd"])] == [(s, r0) for s in withInv for r0 in range(0, nc[s], MV_ROWS)]
        assert [tuple(xd[i][:2]) for i in span(p, L["xinvBwd"])] == [(s, c0) for s in withInv for c0 in range(0, nc[s], 16)]
        inv += withInv
    assert at == p["scalars"][1]
    assert p["scalars"][8] == 8 * max([1] + [nc[s] for s in inv])
    return inv, nGemm


def check_all(sym, p):
    mine = check_front_placement(sym, p)
    recOf, nUpdateOnlyTiles = check_extend_add_and_records(sym, p)
    out = dict(mine=mine, fusedFronts=check_fused_records(sym, p), updateOnlyTiles=nUpdateOnlyTiles)
    out["bulk"], out["roleC"] = check_step_launches(sym, p)
    out["schur"] = check_schur(sym, p, recOf)
    out["inverses"], out["gemm"] = check_inverses(sym, p)
    return out


def test_default_tuning(shim, sym):  # noqa: F811
    p = make_plan(shim, sym)
    got = check_all(sym, p)
    assert [L["bigFronts"][1] for L in p["levels"]] == [0, 0, 11, 7, 4, 3, 2, 1]  # the case has not degenerated
    assert sorted(sym["nc"][sym["nc"] >= XINV_MIN].tolist()) == [195]
    assert got["mine"] == list(range(sym["ns"])) and got["fusedFronts"] == sym["ns"] - 28 > 0
    assert len(got["inverses"]) == 1 and got["roleC"] > 0 and got["gemm"] == 0  # the inverse is bordered
    assert got["bulk"] == 0 and got["schur"] > 0 and got["updateOnlyTiles"] == 0 and not any(L["fuseEA"] or L["schur64"] for L in p["levels"])


def test_two_level_blocking_forced(shim, sym):  # noqa: F811
    got = check_all(sym, make_plan(shim, sym, bulkMinMB=0, bulkBlock=64))
    assert got["bulk"] > 0


def test_every_inverse_through_doubling(shim, sym):  # noqa: F811
    p = make_plan(shim, sym, borderMaxNc=0)
    got = check_all(sym, p)
    assert len(got["inverses"]) == 1 and got["roleC"] == 0 and got["gemm"] > 0 and not any(L["stepTop"] for L in p["levels"])
    assert max(len(X["rounds"]) for X in p["xinvLevels"]) == 3  # 32 -> 64 -> 128 -> 256 >= 195


@pytest.mark.parametrize("schur64Min,fusedEA", [(1, True), (10 ** 9, False)])
def test_both_schur_tilings(shim, sym, schur64Min, fusedEA):  # noqa: F811
    p = make_plan(shim, sym, schur64Min=schur64Min)
    got = check_all(sym, p)
    for L in p["levels"]:  # the rule: a level with at least schur64Min Schur tiles of 32 x 32 (the root's front has no update block: none)
        tiles32 = sum(nt * (nt + 1) // 2 for nt in (-(-(sym["N"][s] - sym["nc"][s]) // 32) for s in big_of(p, L)))
        assert L["fuseEA"] == L["schur64"] == (tiles32 >= schur64Min)
    assert any(L["fuseEA"] for L in p["levels"]) == fusedEA
    assert got["schur"] > 0 and (got["updateOnlyTiles"] > 0) == fusedEA


def test_four_ranks(shim, sym):  # noqa: F811
    plans = [make_plan(shim, sym, world=4, rank=r) for r in range(4)]
    got = [check_all(sym, p) for p in plans]
    executed = [s for g in got for s in g["mine"]]
    assert sorted(executed) == list(range(sym["ns"]))  # disjoint, and together all fronts
    assert all(len(g["mine"]) > 0 for g in got)
    frontAt = {3 * int(sym["firstNode"][s]): s for s in range(sym["ns"])}
    m = sym["N"] - sym["nc"]
    nOps = 0
    lists = []
    for p in plans:
        per = []
        for X in p["xchg"]:
            fronts = [int(p["xchgDesc"][i][0]) for i in span(p, X["pack"])] + [int(p["xchgDesc"][i][0]) for i in span(p, X["unpack"])]
            assert len(fronts) == len(X["opsM"]) == len(X["opsW"])
            for i, s in enumerate(fronts):
                d = p["xchgDesc"][(list(span(p, X["pack"])) + list(span(p, X["unpack"])))[i]]
                assert X["opsM"][i][0] == off64(d[1], d[2]) and X["opsW"][i][0] == d[3]
                assert X["opsM"][i][1] == m[s] * (m[s] + 1) // 2 and X["opsW"][i][1] == m[s]
                assert X["opsM"][i][2:] == X["opsW"][i][2:] == [X["opsM"][i][2], 1 if i < X["pack"][1] else 0]
            for off, cnt, peer, send in X["opsM"]:  # inside the level's staging counts ...
                assert 0 <= off and off + cnt <= X["count"] and 0 <= peer < 4 and peer != p["rank"]
            for off, cnt, peer, send in X["opsW"]:
                assert X["count"] <= off and off + cnt <= X["count"] + X["countW"] <= p["scalars"][9]
            for off, cnt, peer, send in X["opsX"]:  # ... or inside the solution vector
                assert cnt == sym["nc"][frontAt[off]] and off + cnt <= 3 * sym["nn"]
            per.append(dict(M=[(s, o[1], o[2], o[3]) for s, o in zip(fronts, X["opsM"])], W=[(s, o[1], o[2], o[3]) for s, o in zip(fronts, X["opsW"])],
                            X=[(frontAt[o[0]], o[1], o[2], o[3]) for o in X["opsX"]]))
            nOps += len(X["opsM"]) + len(X["opsX"])
        lists.append(per)
    assert nOps > 0
    for r in range(4):  # what r sends to q at a level is what q receives from r: front, count, order
        for q in range(4):
            for l in range(len(plans[0]["levels"])):
                for k in "MWX":
                    assert [o[:2] for o in lists[r][l][k] if o[2] == q and o[3] == 1] == [o[:2] for o in lists[q][l][k] if o[2] == r and o[3] == 0]
