"""The shared device helpers of ipc_amd/csrc/device_prims.h, each checked on its own through tests/device_prims/prims_shim.hip.

Bit-reproducible energies, gradients and CSR values rest on every unit running the same reduction tree.  The expected values here replay that tree in numpy --
offsets 32, 16, ..., 1 inside each 64-lane wave (a lane whose partner lies past the wave keeps its own value), the waves of a workgroup in index order, the
partial sums strided by 256 and summed by the same tree -- and are compared for equal bits, never within a tolerance.  The inputs span 30 orders of magnitude
with mixed signs, so that any other summation order changes bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000]
PARTIAL_COUNTS = [0, 1, 255, 256, 257]


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "device_prims", "prims_shim.hip")
    hdr = os.path.join(ROOT, "ipc_amd", "csrc", "device_prims.h")
    so = os.path.join(HERE, "device_prims", "_build", "libprims_shim.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-x", "hip",
                               "-I" + os.path.dirname(hdr), src, "-o", so])
    lib = C.CDLL(so)
    lib.prims_wave_f64.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    lib.prims_wave_i32.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.prims_block_partials.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.prims_reduce.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]
    lib.prims_block_row_off.argtypes = [C.c_int, C.c_void_p]
    lib.prims_find_block.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.prims_nblk.argtypes = [C.c_longlong, C.c_int]
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def wild(n, seed):
    """n doubles, magnitudes 1e-15 .. 1e15, mixed signs"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15.0, 15.0, n)).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the replay ---------------------------------------------------------------------------------------------------------------------------------------------
def wave_down(x, op):
    """all 64 lanes after the __shfl_down tree; lane 0 holds the result"""
    x = np.array(x)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        src = np.where(lanes + off < 64, lanes + off, lanes)
        x = op(x, x[src])
    return x


def wave_xor(x):
    x = np.array(x)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[lanes ^ off]
    return x


def padded(v, mult, pad):
    out = np.full(-(-len(v) // mult) * mult, pad, dtype=v.dtype)
    out[:len(v)] = v
    return out


def block_sum_replay(x256):
    """block_sum<256>: the wave tree, then the four waves in index order starting from +0.0"""
    r = np.float64(0.0)
    for w in range(4):
        r = r + wave_down(x256[64 * w:64 * w + 64], np.add)[0]
    return r


def partials_replay(v):
    p = padded(v, 256, 0.0)
    return np.array([block_sum_replay(p[256 * b:256 * b + 256]) for b in range(len(p) // 256)], dtype=np.float64)


def reduce_replay(partial, scale, accumulate, out0):
    x = np.zeros(256)
    for i in range(len(partial)):  # lane l takes partials l, l + 256, ... in index order
        x[i % 256] = x[i % 256] + partial[i]
    r = np.float64(scale) * block_sum_replay(x)
    return np.float64(out0) + r if accumulate else r


# ---- wave reductions ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_wave_reductions_f64(shim, n):
    v = wild(n, 100 + n)
    nw = (n + 63) // 64
    for op, fn, pad in ((0, np.add, 0.0), (1, np.fmin, np.inf), (2, np.fmax, -np.inf)):
        got = np.full(nw, np.nan)
        assert shim.prims_wave_f64(op, ptr(v), n, pad, ptr(got)) == 0
        p = padded(v, 64, pad)
        want = np.array([wave_down(p[64 * w:64 * w + 64], fn)[0] for w in range(nw)])
        assert np.array_equal(bits(got), bits(want)), (op, n)
    got = np.full(64 * nw, np.nan)
    assert shim.prims_wave_f64(3, ptr(v), n, 0.0, ptr(got)) == 0
    p = padded(v, 64, 0.0)
    want = np.concatenate([wave_xor(p[64 * w:64 * w + 64]) for w in range(nw)])
    assert np.array_equal(bits(got), bits(want)), n


@pytest.mark.parametrize("n", LENGTHS)
def test_wave_reductions_i32(shim, n):
    v = np.random.default_rng(200 + n).integers(-(1 << 20), 1 << 20, n).astype(np.int32)
    nw = (n + 63) // 64
    big = np.iinfo(np.int32).max
    for op, fn, pad in ((0, np.add, 0), (1, np.minimum, big), (2, np.maximum, -big)):
        got = np.full(nw, -1, dtype=np.int32)
        assert shim.prims_wave_i32(op, ptr(v), n, pad, ptr(got)) == 0
        p = padded(v, 64, pad)
        want = np.array([wave_down(p[64 * w:64 * w + 64], fn)[0] for w in range(nw)], dtype=np.int32)
        assert np.array_equal(got, want), (op, n)
    got = np.full(64 * nw, -1, dtype=np.int32)
    assert shim.prims_wave_i32(3, ptr(v), n, 0, ptr(got)) == 0
    p = padded(v, 64, 0)
    assert np.array_equal(got, np.concatenate([wave_xor(p[64 * w:64 * w + 64]) for w in range(nw)])), n


# ---- workgroup sum and the reduce kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_block_sum_then_reduce(shim, n):
    v = wild(n, 300 + n)
    nb = shim.prims_nblk(n, 256)
    assert nb == (n + 255) // 256
    part = np.full(nb, np.nan)
    assert shim.prims_block_partials(ptr(v), n, ptr(part)) == 0
    want = partials_replay(v)
    assert np.array_equal(bits(part), bits(want)), n
    for scale, acc, out0 in ((1.0, 0, 7.0), (0.3, 0, 7.0), (1.0, 1, -2.5e3), (0.3, 1, -2.5e3)):
        out = np.array([out0])
        assert shim.prims_reduce(ptr(part), nb, scale, acc, ptr(out)) == 0
        assert bits(out)[0] == bits(reduce_replay(want, scale, acc, out0))[0], (n, scale, acc)


@pytest.mark.parametrize("n", PARTIAL_COUNTS)
def test_reduce_partial_counts(shim, n):
    part = wild(n, 400 + n)
    for scale, acc, out0 in ((1.0, 0, 7.0), (-1.7e-3, 0, 7.0), (1.0, 1, 1.0e-4), (-1.7e-3, 1, 1.0e-4)):
        out = np.array([out0])
        assert shim.prims_reduce(ptr(part), n, scale, acc, ptr(out)) == 0
        assert bits(out)[0] == bits(reduce_replay(part, scale, acc, out0))[0], (n, scale, acc)


def test_plain_store_keeps_negative_zero(shim):
    """-0.0 partials under scale -1: the sum is +0.0, the product -0.0, and a plain store must publish that -0.0 (0.0 + r would give +0.0)"""
    part = np.full(257, -0.0)
    out = np.array([7.0])
    assert shim.prims_reduce(ptr(part), len(part), -1.0, 0, ptr(out)) == 0
    want = reduce_replay(part, -1.0, 0, 7.0)
    assert bits(want)[0] == 0x8000000000000000 and bits(out)[0] == bits(want)[0]


# ---- blocks of the upper CSR ---------------------------------------------------------------------------------------------------------------------------------
NBRS = {0: [1, 3, 4], 1: [2, 4], 2: [3], 3: [], 4: []}  # upper neighbours of five nodes: row lengths 3 + 3 * len = 12, 9, 6, 3, 3


def pattern():
    ia, ja = [0], []
    for v in range(5):
        for r in range(3):
            ja += [3 * v + c for c in range(r, 3)] + [3 * w + c for w in NBRS[v] for c in range(3)]
            ia.append(len(ja))
    ia, ja = np.array(ia, dtype=np.int32), np.array(ja, dtype=np.int32)
    assert [ia[3 * v + 1] - ia[3 * v] for v in range(5)] == [12, 9, 6, 3, 3]
    return ia, ja


def test_find_block_every_pair(shim):
    """All ten pairs rn < cn: the six present ones at the position enumerated from ia / ja (the last block of rows 0, 1 and 2 among them), the four absent
    ones -1 -- a column between two neighbours (0, 2), one past the last neighbour (2, 4), and rows without any neighbour (1, 3) and (3, 4)."""
    ia, ja = pattern()
    pairs = [(v, w) for v in range(5) for w in range(v + 1, 5)]
    rn, cn = (np.array(x, dtype=np.int32) for x in zip(*pairs))
    got = np.full(len(pairs), -7, dtype=np.int32)
    assert shim.prims_find_block(len(ia) - 1, ptr(ia), ptr(ja), len(pairs), ptr(rn), ptr(cn), ptr(got)) == 0
    want = []
    for v, w in pairs:
        row = ja[ia[3 * v]:ia[3 * v + 1]]
        hit = np.flatnonzero(row == 3 * w)
        want.append(int(ia[3 * v] + hit[0]) if len(hit) else -1)
    assert sum(p < 0 for p in want) == 4 and [want[pairs.index(p)] for p in ((0, 2), (1, 3), (2, 4), (3, 4))] == [-1] * 4
    assert want[pairs.index((0, 4))] == ia[1] - 3 and want[pairs.index((2, 3))] == ia[7] - 3  # the last block of a row
    assert list(got) == want


def test_block_row_off_against_enumerated_positions(shim):
    """Positions enumerated from ia / ja of the scalar upper CSR, every block of every row, the last block of a row included."""
    nbrs = NBRS
    ia, ja = pattern()
    checked = 0
    for v in range(5):
        L = int(ia[3 * v + 1] - ia[3 * v])
        off = np.full(3, -1, dtype=np.int32)
        assert shim.prims_block_row_off(L, ptr(off)) == 0
        for w in nbrs[v]:
            p0 = int(ia[3 * v] + np.flatnonzero(ja[ia[3 * v]:ia[3 * v + 1]] == 3 * w)[0])
            for r in range(3):
                row = ja[ia[3 * v + r]:ia[3 * v + r + 1]]
                want = int(ia[3 * v + r] + np.flatnonzero(row == 3 * w)[0])
                assert p0 + off[r] == want, (v, w, r)
                assert list(ja[want:want + 3]) == [3 * w, 3 * w + 1, 3 * w + 2]
                checked += 1
    assert checked == 18
