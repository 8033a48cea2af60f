"""The fused PPO entry points' host side (no kernel launch): argument validation, the hyper-parameter struct's layout, and the numpy
mirror of ewn_ppo_shuffle's keyed bijection (tests/test_gpu_ppo_fused.py checks the device against this mirror)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ewn_gym_amd import _lib
from ewn_gym_amd._lib import EwnConfig, EwnPpoHyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def shuffle_mirror(n, key, counter, epoch):
    """ewn_ppo_shuffle's row `epoch`: a four-round Feistel network on 2 * half bits with cycle walking into [0, n)"""
    bits = max(0, int(n - 1).bit_length())
    half = 1 if bits < 2 else (bits + 1) // 2
    ke = splitmix64(key ^ splitmix64(((counter & 0xFFFFFFFF) << 32) | (epoch & 0xFFFFFFFF)))
    rk = [np.uint64(splitmix64((ke + r) & M64) & 0xFFFFFFFF) for r in range(4)]
    mask = np.uint64((1 << half) - 1)
    sh = np.uint64(half)

    def feistel(x):
        L, R = x >> sh, x & mask
        for r in range(4):
            L, R = R, L ^ (_fmix32(R ^ rk[r]) & mask)
        return (L << sh) | R

    x = feistel(np.arange(n, dtype=np.uint64))
    out = x >= np.uint64(n)
    while out.any():
        x[out] = feistel(x[out])
        out = x >= np.uint64(n)
    return x.astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 4095, 327680, 327681])
def test_shuffle_mirror_is_a_permutation(n):
    p = shuffle_mirror(n, 17, 0, 0)
    assert np.array_equal(np.sort(p), np.arange(n, dtype=np.int32))
    if n >= 32:
        assert not np.array_equal(p, np.arange(n)), "the identity is no shuffle"
        assert not np.array_equal(p, shuffle_mirror(n, 17, 0, 1)), "another epoch, another order"
        assert not np.array_equal(p, shuffle_mirror(n, 17, 40, 0)), "another update (step count), another order"
        assert not np.array_equal(p, shuffle_mirror(n, 18, 0, 0)), "another seed, another order"


def test_hyper_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    body = re.search(r"typedef struct ewn_ppo_hyper \{(.*?)\} ewn_ppo_hyper;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in EwnPpoHyper._fields_]
    assert C.sizeof(EwnPpoHyper) == 4 * len(fields) == 48


def _cfg(S=5, L=3, N=64):
    return EwnConfig(board_size=S, cube_layer=L, n_lanes=N, opponent_kind=0, max_depth=3, rng_kind=1, shaped=1, autoreset=1)


def test_host_validation_without_a_launch():
    lib = _lib.load()
    EINVAL, ENULL, EUNS = -1, -2, -4
    hp = EwnPpoHyper(0.99, 0.95, 0.2, 0.5, 0.0, 0.5, 3e-4, 0.9, 0.999, 1e-5, 1, 1)
    cfg = _cfg()
    one = C.c_void_p(16)     # never dereferenced: every call below fails validation before anything is launched
    # geometry: what ewn_a2c_* serves (cube_layer 3, 5x5 / 7x7)
    for S, L in ((6, 3), (8, 3), (7, 4)):
        c = _cfg(S, L)
        assert lib.ewn_ppo_scratch_bytes(C.byref(c), 5, 64) == EUNS
        assert lib.ewn_ppo_prepare(C.byref(c), 5, one, one, one, C.byref(hp), one, None) == EUNS
        assert lib.ewn_ppo_grad(C.byref(c), 5, one, one, one, C.byref(hp), one, 64, one, one, None) == EUNS
        assert lib.ewn_ppo_apply(C.byref(c), one, one, one, one, one, C.byref(hp), None, None) == EUNS
    assert lib.ewn_ppo_scratch_bytes(C.byref(cfg), 5, 64) > 0
    # K < 1, batch_size outside [1, K * N]
    for K, B in ((0, 1), (-1, 1), (5, 0), (5, 5 * 64 + 1), (1, 65)):
        assert lib.ewn_ppo_scratch_bytes(C.byref(cfg), K, B) == EINVAL
        assert lib.ewn_ppo_grad(C.byref(cfg), K, one, one, one, C.byref(hp), one, B, one, one, None) == EINVAL
    assert lib.ewn_ppo_prepare(C.byref(cfg), 0, one, one, one, C.byref(hp), one, None) == EINVAL
    assert lib.ewn_ppo_scratch_bytes(C.byref(cfg), 5, 5 * 64) > 0 and lib.ewn_ppo_scratch_bytes(C.byref(cfg), 1, 1) > 0
    # null pointers
    assert lib.ewn_ppo_scratch_bytes(None, 5, 64) == ENULL
    for i in range(5):
        a = [one] * 5
        a[i] = None
        assert lib.ewn_ppo_prepare(C.byref(cfg), 5, a[0], a[1], a[2], C.byref(hp) if i != 3 else None, a[4], None) == ENULL
    for i in range(7):
        a = [one] * 7
        a[i] = None
        assert lib.ewn_ppo_grad(C.byref(cfg), 5, a[0], a[1], a[2], C.byref(hp) if i != 3 else None, a[4], 64, a[5], a[6], None) == ENULL
    for i in range(6):
        a = [one] * 6
        a[i] = None
        assert lib.ewn_ppo_apply(C.byref(cfg), a[0], a[1], a[2], a[3], a[4], C.byref(hp) if i != 5 else None, None, None) == ENULL
    bad_world = EwnPpoHyper(0.99, 0.95, 0.2, 0.5, 0.0, 0.5, 3e-4, 0.9, 0.999, 1e-5, 1, 0)
    assert lib.ewn_ppo_apply(C.byref(cfg), one, one, one, one, one, C.byref(bad_world), None, None) == EINVAL
    # shuffle: n in [1, 2^31 - 1], epochs >= 1, perm required
    assert lib.ewn_ppo_shuffle(0, 1, 0, None, one, None) == EINVAL
    assert lib.ewn_ppo_shuffle(1 << 31, 1, 0, None, one, None) == EINVAL
    assert lib.ewn_ppo_shuffle(10, 0, 0, None, one, None) == EINVAL
    assert lib.ewn_ppo_shuffle(10, 1, 0, None, None, None) == ENULL
