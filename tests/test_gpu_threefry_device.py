"""The device Threefry routines for wave-uniform keys (csrc/rng.h: threefry2x32_uh / threefry2x32_uh2) against the numpy Threefry-2x32-20 of
the oracle, word for word.  The routines fold the key injections into neighbouring instructions (v_add3_u32, v_xad_u32) and add the
wave-uniform parts of the counters -- offset, half, key word -- on the scalar unit before the lane's part: identities mod 2^32, which
this file checks where the sums wrap.  One block of 256 threads through dibs_debug_threefry (include/dibs_hip.h); no workload shapes."""
import ctypes as C

import numpy as np
import pytest

from oracle import prng

pytestmark = pytest.mark.gpu

U32 = np.uint32
M32 = 0xFFFFFFFF
# Random123 known-answer vectors (tests/test_prng.py): key, counter, output
KAT = [((0, 0), (0, 0), (0x6B200159, 0x99BA4EFE)),
       ((M32, M32), (M32, M32), (0x1CB996FC, 0xBB002BE7)),
       ((0x13198A2E, 0x03707344), (0x243F6A88, 0x85A308D3), (0xC4923A9C, 0x483DF7A0))]


def _device(k0, k1, half, off_b, c0):
    from dibs_amd import _lib
    lib = _lib.load()
    c0 = np.ascontiguousarray(c0, dtype=U32)
    out = np.zeros((c0.size, 6), dtype=U32)
    _lib.check(lib.dibs_debug_threefry(int(k0), int(k1), int(half), int(off_b), c0.ctypes.data_as(C.c_void_p), c0.size,
                                      out.ctypes.data_as(C.c_void_p)))
    return out


def _expected(k0, k1, half, off_b, c0):
    c0 = np.asarray(c0, dtype=np.uint64)
    a = (c0 & M32).astype(U32)
    b = ((c0 + off_b) & M32).astype(U32)
    ya = prng.threefry2x32(k0, k1, a, ((c0 + half) & M32).astype(U32))
    yb = prng.threefry2x32(k0, k1, b, ((c0 + off_b + half) & M32).astype(U32))
    return np.stack([ya[0], ya[1], ya[0], ya[1], yb[0], yb[1]], axis=1)


def _check(k0, k1, half, off_b, c0):
    got, want = _device(k0, k1, half, off_b, c0), _expected(k0, k1, half, off_b, c0)
    assert np.array_equal(got, want), (hex(k0), hex(k1), hex(half), hex(off_b), np.argwhere(got != want)[:4].tolist())


def test_random123_vectors():
    for (k0, k1), (c0, c1), y in KAT:
        half = (c1 - c0) & M32
        for off_b in (0, 1, 0x9E3779B9):
            # entry 0: the vector is the single call and call a of the pair; entry 1: it is call b of the pair
            got = _device(k0, k1, half, off_b, [c0, (c0 - off_b) & M32])
            assert got[0, :4].tolist() == [y[0], y[1], y[0], y[1]]
            assert got[1, 4:].tolist() == [y[0], y[1]]
            _check(k0, k1, half, off_b, [c0, (c0 - off_b) & M32])


def test_extreme_keys_and_wrapping_sums():
    c0 = np.arange(0xFFFFFF00, 0x100000000, dtype=np.uint64)  # 256 lanes: c0 + half, c0 + off_b (and their sum) wrap for every one of them
    for k0 in (0, M32):
        for k1 in (0, M32):
            for half, off_b in ((0x180, 0x200), (0x100, 0x100), (M32, M32), (0x80000000, 0x80000100), (0, 0)):
                # (k1 = 0xFFFFFFFF: half + k1 wraps for every half > 0; k0 = 0xFFFFFFFF: off_b + k0 wraps for every off_b > 0)
                _check(k0, k1, half, off_b, c0)
    # keys and scalars that wrap only in the three-term sums off_b + half + k1
    _check(0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, 0x00000003, c0)
    _check(0x80000000, 0x00000001, 0xFFFFFFFE, 0x00000001, c0)


def test_random_arguments():
    rng = np.random.default_rng(20)
    for _ in range(64):  # 64 keys x 64 counters = 4 096 random (key, half, c0)
        k0, k1, half, off_b = (int(v) for v in rng.integers(0, 1 << 32, size=4, dtype=np.uint64))
        _check(k0, k1, half, off_b, rng.integers(0, 1 << 32, size=64, dtype=np.uint64))


def test_more_counters_than_threads():
    rng = np.random.default_rng(21)
    _check(0xDEADBEEF, 0x01234567, 0x00271000, 50, rng.integers(0, 1 << 32, size=1000, dtype=np.uint64))  # (the block strides over n)
