"""The two reply exceptions of the slot-task depth-3 search as table entries (ewn_gym_amd/csrc/ewn_movetab.hpp): on 5x5
and 6x6 a reply that does not exist and a reply onto the origin are ONE cell above the board in the reply entry's mask, lvl[0] /
lvl[1] answer the spare levels 7 / 6 for it, and columns 56..63 / 48..55 of every row of rank[] hold "no such reply" / -10.  The
block writes those entries into its LDS copy of the image (slot_tabs_build); the image itself is what it was.

All on the host: tests/phantom_tables_host.hip calls slot_tabs_build in both forms over every image of a board size (compiled here
for the host alone, a second or two); the images of 7x7 and 8x8, which keep the address steering, come from the library and are
pinned by the hashes of the last build before this form (tests/golden/r12_fast_images_sha256.json)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = 8
FAST_NONE8 = 1023 * 8
LVL_NONE, LVL_HOME = 7, 6    # PH_LVL_NONE / PH_LVL_HOME


@pytest.fixture(scope="module")
def lib():
    from ewn_gym_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("phantom")
    exe = str(d / "phantom_tables_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ewn_gym_amd", "csrc"),
                           os.path.join(ROOT, "tests", "phantom_tables_host.hip"), "-o", exe])
    return exe, d


class Built:
    """what the host program wrote for one board size"""

    def __init__(self, exe, d, S):
        out = str(d / ("s%d.bin" % S))
        subprocess.check_call([exe, str(S), out])
        raw = np.fromfile(out, np.uint8)
        hdr = raw[:40].view(np.int32)
        assert hdr[0] == S and hdr[1] == IMAGES
        self.S, self.nbytes, self.ent_new, self.ent_old, self.off_lvl, self.off_m10, self.mb, self.struct_bytes = (int(x) for x in (hdr[0], *hdr[2:9]))
        self.W = 8 * self.mb
        mdt = np.uint32 if self.mb == 4 else np.uint64
        self.image, self.copy, self.rset_new, self.rset_old, self.rkf = [], [], [], [], []
        p = 40
        for _ in range(IMAGES):
            self.image.append(raw[p:p + self.nbytes]); p += self.nbytes
            self.copy.append(raw[p:p + self.nbytes]); p += self.nbytes
            new = raw[p:p + 128 * self.ent_new].reshape(128, self.ent_new); p += 128 * self.ent_new
            old = raw[p:p + 128 * self.ent_old].reshape(128, self.ent_old); p += 128 * self.ent_old
            self.rset_new.append(np.ascontiguousarray(new[:, :3 * self.mb]).view(mdt).astype(np.uint64))       # [position byte][direction]
            assert not new[:, 3 * self.mb:].any()
            self.rset_old.append(np.ascontiguousarray(old[:, :3 * self.mb]).view(mdt).astype(np.uint64))
            self.rkf.append(np.ascontiguousarray(old[:, 3 * self.mb:3 * self.mb + 12]).view(np.uint32))
        assert p == len(raw)
        self.NONE, self.HOME = np.uint64(1 << (self.W - 1)), np.uint64(1 << (self.W - 2))

    def lvl(self, img):
        return img[self.off_lvl - 8:self.off_lvl + 72]   # index z + 8: lvl[-1] (the guard byte) is index 7

    def m10(self, img):
        return int(img[self.off_m10:self.off_m10 + 4].view(np.int32)[0])


@pytest.fixture(scope="module", params=[5, 6])
def built(request, prog):
    return Built(prog[0], prog[1], request.param)


@pytest.fixture(scope="module")
def rank_off(lib):
    return {S: np.array([[lib.ewn_tables_rank_offset(S, ix, iy) for iy in range(64)] for ix in range(64)], np.int64) for S in (5, 6)}


def rank_at(img, off):
    return img[off].astype(np.uint16) | (img[off + 1].astype(np.uint16) << 8)


def side(b, img, masks):
    """a side's 6-bit (level, count) index as ft_side computes it: lvl[clz(mask)] + popcount(mask) (an empty mask reads the guard byte)"""
    masks = np.asarray(masks, np.uint64)
    bl = np.array([int(m).bit_length() for m in masks.ravel()]).reshape(masks.shape)
    pc = np.array([bin(int(m)).count("1") for m in masks.ravel()]).reshape(masks.shape)
    z = np.where(bl == 0, -1 if b.mb == 4 else b.W, b.W - bl)
    return b.lvl(img)[z + 8].astype(np.int64) + pc


def test_the_program_built_the_library_s_images(lib, built):
    n = lib.ewn_tables_bytes(built.S, 3)
    buf = np.zeros(n, np.uint8)
    assert lib.ewn_build_tables(built.S, 3, buf.ctypes.data_as(C.c_void_p)) == 0
    for im, img in enumerate(buf.reshape(IMAGES, -1)):
        assert np.array_equal(img, built.image[im]), im


def test_spare_levels_and_constant_columns_in_every_row(built, rank_off):
    b, off = built, rank_off[built.S]
    for im in range(IMAGES):
        img, cp = b.image[im], b.copy[im]
        assert b.lvl(cp)[8 + 0] == LVL_NONE << 3 and b.lvl(cp)[8 + 1] == LVL_HOME << 3, im
        r = rank_at(cp, off)
        assert (r[:, 56:64] == FAST_NONE8).all() and (r[:, 48:56] == 8 * b.m10(img)).all(), im
        # ... and nothing else of the struct differs from the image (behind it: the image's padding, where the 5x5 move table goes)
        diff = np.flatnonzero(cp[:b.struct_bytes] != img[:b.struct_bytes])
        allowed = set((off[:, 48:64].ravel()[:, None] + np.arange(2)).ravel().tolist()) | {b.off_lvl, b.off_lvl + 1}
        assert set(diff.tolist()) <= allowed, (im, diff[:8])
        assert not img[b.struct_bytes:].any()


def test_no_real_level_and_count_reaches_the_constant_columns(built):
    b, S = built, built.S
    for im in range(IMAGES):
        lv = b.lvl(b.copy[im]).astype(np.int64)
        # lvl[clz] of every real cell h (clz = W - 1 - h), of an empty 64-bit mask (clz = W) and the guard byte, plus the largest count
        real = [lv[8 + b.W - 1 - h] for h in range(S * S)] + [lv[7], lv[8 + b.W] if b.W == 64 else 0]
        assert max(real) + 6 < 8 * LVL_HOME, (im, max(real))
        assert b.W - 1 - (S * S - 1) > 1          # clz of the highest real cell: lvl[0] and lvl[1] belong to no real cell


def test_a_phantom_cell_with_any_real_cells_indexes_the_constant_columns(built):
    b, S = built, built.S
    rng = np.random.default_rng(12)
    masks = [0]
    for k in range(1, 7):
        masks += [sum(1 << int(c) for c in rng.choice(S * S, k, replace=False)) for _ in range(40)]
        masks += [sum(1 << c for c in range(S * S - k, S * S)), sum(1 << c for c in range(k))]
    masks = np.array(masks, np.uint64)
    for im in range(IMAGES):
        iy = side(b, b.copy[im], masks | b.NONE)
        assert iy.min() >= 8 * LVL_NONE + 1 and iy.max() <= 8 * LVL_NONE + 7, im
        iy = side(b, b.copy[im], masks | b.HOME)
        assert iy.min() >= 8 * LVL_HOME + 1 and iy.max() <= 8 * LVL_HOME + 7, im


def test_old_steered_address_and_new_address_read_the_same_rank(built, rank_off):
    """every position byte and direction, every row ix, the replier's other cubes Nk with 0..5 cells:
    old: rank[(ft_addr(ix, side(Nk | rset)) & keep) | fixed] in the image; new: rank[ft_addr(ix, side(Nk | rset'))] in the block's copy"""
    b, S, off = built, built.S, rank_off[built.S]
    rng = np.random.default_rng(7)
    nk = [0] + [sum(1 << int(c) for c in rng.choice(S * S, k, replace=False)) for k in range(1, 6) for _ in range(3)]
    nk = np.array(nk, np.uint64)
    ix = np.arange(64)
    seen = {"none": 0, "home": 0, "real": 0}
    for im in range(IMAGES):
        img, cp = b.image[im], b.copy[im]
        kf, ro, rn = b.rkf[im], b.rset_old[im], b.rset_new[im]
        keep, fixed = (kf & 0xFFFF).astype(np.int64), (kf >> 16).astype(np.int64)
        # the entries themselves
        none, home = (keep == 0) & (fixed == 0), fixed == 2
        assert ((keep == 0xFFFF) | (keep == 0)).all() and (none | home | ((keep == 0xFFFF) & (fixed == 0))).all()
        assert none[64:].all(), "position bytes 64..127: no such cube, no reply"
        assert (rn[none] == b.NONE).all() and (rn[home] == b.HOME).all() and np.array_equal(rn[~none & ~home], ro[~none & ~home])
        seen["none"] += int(none.sum()); seen["home"] += int(home.sum()); seen["real"] += int((~none & ~home).sum())
        iy_old = side(b, img, nk[None, None, :] | ro[:, :, None])                 # [pb][d][Nk]
        iy_new = side(b, cp, nk[None, None, :] | rn[:, :, None])
        assert iy_old.max() < 64 and iy_new.max() < 64
        a_old = (off[ix[:, None, None, None], iy_old[None]] & keep[None, :, :, None]) | fixed[None, :, :, None]   # [ix][pb][d][Nk]
        a_new = off[ix[:, None, None, None], iy_new[None]]
        assert np.array_equal(rank_at(img, a_old), rank_at(cp, a_new)), im
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("S", [7, 8])
def test_images_of_7x7_and_8x8_are_byte_identical_to_the_parent_s(lib, S):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "r12_fast_images_sha256.json")))
    n = lib.ewn_tables_bytes(S, 3)
    buf = np.zeros(n, np.uint8)
    assert lib.ewn_build_tables(S, 3, buf.ctypes.data_as(C.c_void_p)) == 0
    assert hashlib.sha256(buf.tobytes()).hexdigest() == want["S%d" % S]
