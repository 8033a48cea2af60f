"""The leaf-rank table of the specialised searches (FastTab::rank, ewn_gym_amd/csrc/ewn_fast.hpp) is laid out for the LDS banks, not
as rank[(ix << 6) | iy]; only ft_index / ft_addr know the layout.  These tests pin what the layout may not change:

 * CPU: for every board size and every heuristic image, the entry the address helper finds for (ix, iy) is the rank the
   row-major definition rank[(ix << 6) | iy] gave (tests/golden/g14_fast_rank.npz: the tables of the last build with that
   definition), and everything behind rank[] in the image -- val, val6, the small tables -- is unchanged byte for byte;
 * GPU: root values and actions of the max_depth 1-5 searches against the reference's vectors (tests/golden/g5_minimax.json).
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = 8   # four heuristic images x two variants (max_depth 1-3 and 5; max_depth 4 and 6)


def _images(lib, S):
    n = lib.ewn_tables_bytes(S, 3)
    assert n > 0 and n % IMAGES == 0
    buf = np.zeros(n, np.uint8)
    assert lib.ewn_build_tables(S, 3, buf.ctypes.data_as(C.c_void_p)) == 0
    return buf.reshape(IMAGES, n // IMAGES)


@pytest.fixture(scope="module")
def lib():
    from ewn_gym_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def old():
    return np.load(os.path.join(ROOT, "tests", "golden", "g14_fast_rank.npz"))


@pytest.mark.parametrize("S", [5, 6, 7, 8])
def test_every_pair_reads_the_rank_of_the_row_major_table(lib, old, S):
    img = _images(lib, S)
    off = np.array([[lib.ewn_tables_rank_offset(S, ix, iy) for iy in range(64)] for ix in range(64)], np.int64)
    assert off.min() >= 0 and (off % 2 == 0).all()
    assert len(np.unique(off)) == 64 * 64, "two pairs share an entry"
    # the two entries d3_search's address steering reads at fixed byte addresses 0 and 2: "no such reply" and -10
    assert off[0, 0] == 0 and off[0, 1] == 2
    want = old["rank_S%d" % S]          # [image][ix][iy]
    for im in range(IMAGES):
        got = img[im][off].astype(np.uint16) | (img[im][off + 1].astype(np.uint16) << 8)
        assert np.array_equal(got, want[im]), (S, im, np.argwhere(got != want[im])[:4].tolist())


@pytest.mark.parametrize("S", [5, 6, 7, 8])
def test_the_rest_of_the_image_is_unchanged(lib, old, S):
    img = _images(lib, S)
    off = np.array([[lib.ewn_tables_rank_offset(S, ix, iy) for iy in range(64)] for ix in range(64)], np.int64)
    # rank[] is the image's first member; val[] (64-bit LDS reads) follows it at the next 8-byte boundary behind its last entry
    end = (int(off.max()) + 2 + 7) // 8 * 8
    assert end - 8192 <= 256, "the padding of rank[] may cost 256 B at most"
    assert img.shape[1] == 32768, "the image size is part of every kernel's LDS budget"
    for im in range(IMAGES):
        tail = np.trim_zeros(img[im][end:], "b")
        assert hashlib.sha256(tail.tobytes()).digest() == old["tail_S%d" % S][im].tobytes(), (S, im)


def test_rank_offset_rejects_what_has_no_entry(lib):
    for args in ((4, 0, 0), (9, 0, 0), (5, -1, 0), (5, 64, 0), (5, 0, -1), (5, 0, 64)):
        assert lib.ewn_tables_rank_offset(*args) < 0, args


@pytest.mark.gpu
def test_depth_1_to_5_searches_against_the_reference_vectors(golden):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd as ea
    g = golden("g5_minimax.json")
    n, depths = 0, set()
    for (S, L) in sorted({(r["S"], r["L"]) for r in g}):
        recs = [r for r in g if (r["S"], r["L"]) == (S, L)]
        for key in sorted({k for r in recs for k in r["res"]}):
            d, h = key.split("/")
            if not 1 <= int(d) <= 5:
                continue
            sub = [r for r in recs if key in r["res"]]
            boards = np.array([r["board"] for r in sub], np.int8).reshape(-1, S, S)
            acts, vals = ea.predict_minimax(boards, [r["dice"] for r in sub], int(d), h, cube_layer=L)
            acts, vals = acts.cpu().numpy(), vals.cpu().numpy()
            for i, r in enumerate(sub):
                a0, a1, v = r["res"][key]
                assert acts[i].tolist() == [a0, a1], (S, L, key, i)
                assert float(vals[i]).hex() == float.fromhex(v).hex(), (S, L, key, i)
                n += 1
            depths.add(int(d))
    assert depths >= {1, 2, 3, 4, 5} and n > 2000, (sorted(depths), n)
