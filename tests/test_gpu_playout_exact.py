"""The playout tree search with exact endgame values at covered leaves (ewn_playout_search_eg, playout_search_exact,
predict_playout_search_exact) against its definition driven through the public stage calls: puct_begin, then per
round EndgameTable.lookup(leaf rows, leaf dice, return_q=True) and playout_wins on the leaf rows (tree m's row at index obs_id0 + m,
key + r * 0x9E3779B97F4A7C15); where the lookup says covered and the tree has a pending leaf the value is q at the action the lookup
returns, elsewhere (2 w - n) / n as one correctly rounded fp32 division; puct_advance with zero logits.  The tree code, the playout
code, the coverage test and the table's gather are the same on both paths, so there is no tolerance anywhere in this file: every
comparison is of all bytes of all trees, and any difference is a bug.
Tables: the session's (5, 2, 4) and (7, 2, 3), built once by tests/test_gpu_endgame.py's table() and left unchanged.
1. lock step by rounds.  2. covered roots.  3. rows where no leaf is covered.  4. the grid.  5. sims = 0 and rounds = 0.  6. leaf
counts.  7. prior contents.  8. guard zones.  9. dice outside 1..6 and malformed roots.  10. chunks and shards.  11. the stream
contract (the entry is declared outside ewn_hip.h: its two cases live here).  12. the agent, the spec and one tournament row."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_endgame import board_of, table  # noqa: E402
from tests.test_gpu_lookahead_endgame import sample_counts  # noqa: E402
from tests.test_gpu_playout_search import gpu_wins, same, views  # noqa: E402
from tests.test_playout_search_cpu import KEY_STEP, MASK64  # noqa: E402

SHAPES = [(5, 9, 6, 64), (5, 5, 17, 7), (7, 9, 6, 64), (7, 1, 12, 1)]        # (S, M, sims, playouts)
TABLE = {5: (2, 4), 7: (2, 3)}
KEY, OBS0 = 2 ** 64 - 5 * KEY_STEP + 12345, 5                                # the key wraps within the rounds; a first id that is not 0
COVERED = {5: [(2, 2), (2, 2), (2, 2)], 7: [(1, 2), (2, 1), (1, 2)]}         # (own, opposing) cubes of the roots the table covers ...
OUTSIDE = {5: [(3, 2), (2, 3), (3, 2)], 7: [(2, 2), (2, 2), (2, 2)]}         # ... and of the roots just outside it
PICK = {9: list(range(9)), 5: [0, 2, 3, 6, 7], 1: [6]}                       # the rows of a smaller batch, out of the nine
SEED = {5: 1, 7: 5}                                                          # of the sampled roots: chosen so that the mix below holds


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_ROWS, _STAGED = {}, {}


def fresh(ea, S, n):
    env = ea.VecEWN(n, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=n, philox_key=77 + S)
    b, d = env.reset(seeds=(np.arange(n, dtype=np.uint64) * 5 + 3).astype(np.uint32))
    return b.clone().reshape(n, S, S), d.clone()


def rows(ea, S, M, seed=None):
    """M observations, computed once and left unchanged -> (boards int8 [M, S, S], dice int8 [M]).  The nine: row 0 a fresh reset (no
    leaf is covered), row 1 a finished position, row 2 a board with one side empty (4t's degenerate rows), rows 3 .. 5 sampled roots
    that the table covers, rows 6 .. 8 sampled roots just outside it; five and one: PICK's rows of the nine"""
    seed = SEED[S] if seed is None else seed
    if (S, M, seed) not in _ROWS:
        rng = random.Random(1000 * S + seed)
        b0, d0 = fresh(ea, S, 3)
        b0[1], b0[2] = 0, 0
        b0[1, S - 1, S - 1], b0[1, 0, 1], d0[1] = 2, -1, 4     # already won
        b0[2, 1, 1], d0[2] = 2, 3                              # no opposing cube
        sampled = np.stack([board_of(sample_counts(rng, S, ka, ko), S) for ka, ko in COVERED[S] + OUTSIDE[S]])
        dice = torch.tensor([rng.randint(1, 6) for _ in range(6)], dtype=torch.int8, device="cuda")
        b, d = torch.cat([b0, torch.as_tensor(sampled).cuda()]), torch.cat([d0, dice])
        pick = torch.tensor(PICK[M], device="cuda")
        _ROWS[(S, M, seed)] = (b[pick].contiguous(), d[pick].contiguous())
    return _ROWS[(S, M, seed)]


def other_rows(ea, S, M):
    """a second valid set of M observations: the nine in reverse, or another row of them"""
    b9, d9 = rows(ea, S, 9)
    return (b9.flip(0).contiguous(), d9.flip(0).contiguous()) if M == 9 else (b9[7:7 + M].contiguous(), d9[7:7 + M].contiguous())


def exact_of(t, lb, ld):
    """the definition's value of covered rows: lookup's q at the action it returns -> (covered bool [M], value float32 [M]), on the host"""
    acts, covered, q = t.lookup(lb, ld, return_q=True)
    a = (3 * acts[:, 0].long() + acts[:, 1].long())[:, None]
    return covered.cpu().numpy(), q.reshape(-1, 6).gather(1, a).reshape(-1).cpu().numpy()


def staged(ea, t, b, d, sims, n, key=KEY, obs_id0=OBS0, c_puct=1.5):
    """the yardstick -> (the trees after begin and after every round, the leaf counts int32 [M, 2] after as many rounds), clones"""
    wins = gpu_wins(ea)
    M, S = b.shape[0], b.shape[1]
    tree, lb, ld = ea.puct_begin(b, d, sims)
    zeros = torch.zeros((M, 5), dtype=torch.float32, device="cuda")
    spare = fresh(ea, S, 1)[0][0]                              # a live position stands in the playout call where a tree has no leaf
    counts = np.zeros((M, 2), np.int32)
    snaps, csnaps = [tree.clone()], [counts.copy()]
    for r in range(sims + 1):
        pending = ea.puct_tree_views(tree, S, sims)["pending"] >= 0
        covered, exact = exact_of(t, lb, ld)
        batch = torch.cat([spare[None].repeat(obs_id0, 1, 1), torch.where(pending[:, None, None], lb, spare[None])]).contiguous()
        w = wins(batch, n, (key + r * KEY_STEP) & MASK64)[obs_id0:].astype(np.int32)
        value = (2 * w - n).astype(np.float32) / np.float32(n)                 # one correctly rounded division
        pend = pending.cpu().numpy()
        by_table = covered & pend                              # a tree without a pending leaf is not looked up
        value = np.where(by_table, exact, value).astype(np.float32)
        assert np.isfinite(value).all()
        counts[:, 0] += by_table
        counts[:, 1] += pend & ~covered
        ea.puct_advance(tree, zeros, torch.as_tensor(value).cuda(), lb, ld, sims, c_puct=c_puct, terminal_value=1.0)
        snaps.append(tree.clone())
        csnaps.append(counts.copy())
    return snaps, csnaps


def reference(ea, S, M, sims, n):
    """the staged trees and counts of a shape at KEY and OBS0, computed once, shared and left unchanged"""
    if (S, M, sims, n) not in _STAGED:
        b, d = rows(ea, S, M)
        _STAGED[(S, M, sims, n)] = staged(ea, table(ea, S, *TABLE[S]), b, d, sims, n)
    return _STAGED[(S, M, sims, n)]


def counts_equal(got, want, where):
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape, where
    assert np.array_equal(got.cpu().numpy(), want), "%s: leaf counts %s, the yardstick's %s" % (where, got.tolist(), want.tolist())


# ---------------------------------------------------------------- 1. lock step by rounds

@pytest.mark.parametrize("S,M,sims,n", SHAPES)
def test_lock_step_by_rounds(ea, S, M, sims, n):
    """fails without the feature: the entry does not exist"""
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, M)
    want, cwant = reference(ea, S, M, sims, n)
    assert len(want) == sims + 2
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    for r in range(sims + 2):
        got, c = ea.playout_search_exact(b, d, sims, t, rounds=r, **kw)
        same(got, want[r], "%d rounds" % r)
        counts_equal(c, cwant[r], "%d rounds" % r)
    got, c = ea.playout_search_exact(b, d, sims, t, **kw)
    same(got, want[-1], "all rounds")
    counts_equal(c, cwant[-1], "all rounds")
    same(ea.playout_search_exact(b, d, sims, t, rounds=sims + 9, playouts=n, key=KEY, obs_id0=OBS0), want[-1], "more rounds than there are")
    cw = cwant[-1]
    print("S=%d M=%d sims=%d playouts=%d: leaves by table / by playouts per tree %s" % (S, M, sims, n, cw.tolist()))
    assert cw[:, 0].sum() > 0 and cw[:, 1].sum() > 0           # on the yardstick: leaves of both kinds occur across the batch
    v = views(ea, want[-1], S, sims)
    live = v["degenerate"] == 0
    assert (v["done"][live] == sims).all() and (v["pending"] == -1).all()


def test_the_rows_just_outside_hold_both_kinds_in_one_tree(ea):
    """counted on the yardstick at sims 17: at least a quarter of the just-outside rows"""
    S, M, sims, n = SHAPES[1]
    cw = reference(ea, S, M, sims, n)[1][-1]
    outside = [i for i, r in enumerate(PICK[M]) if r >= 6]
    both = [i for i in outside if cw[i, 0] > 0 and cw[i, 1] > 0]
    print("just outside: rows %s, leaf counts %s, both kinds in rows %s" % (outside, cw[outside].tolist(), both))
    assert 4 * len(both) >= len(outside) > 0


# ---------------------------------------------------------------- 2. covered roots

@pytest.mark.parametrize("S", [5, 7])
def test_covered_roots_run_no_playouts(ea, S):
    """every leaf below a covered root is covered (a move never adds a cube), so no playout runs: the trees depend on neither the
    key, nor the first observation id, nor the number of playouts"""
    t = table(ea, S, *TABLE[S])
    rng = random.Random(40 + S)
    b = torch.as_tensor(np.stack([board_of(sample_counts(rng, S, ka, ko), S) for ka, ko in COVERED[S] * 3])).cuda().contiguous()
    d = torch.tensor([1 + i % 6 for i in range(9)], dtype=torch.int8, device="cuda")
    sims = 9
    base, c = ea.playout_search_exact(b, d, sims, t, playouts=64, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    assert int(c[:, 1].sum()) == 0 and int(c[:, 0].min()) >= 1
    same(base, staged(ea, t, b, d, sims, 64)[0][-1], "covered roots against the yardstick")
    for kw in (dict(playouts=64, key=KEY + 1, obs_id0=OBS0), dict(playouts=64, key=KEY, obs_id0=OBS0 + 1), dict(playouts=3, key=KEY, obs_id0=OBS0)):
        got, c2 = ea.playout_search_exact(b, d, sims, t, return_leaf_counts=True, **kw)
        same(got, base, str(kw))
        assert torch.equal(c2, c)


# ---------------------------------------------------------------- 3. rows where no leaf is covered

@pytest.mark.parametrize("S", [5, 7])
def test_without_a_covered_leaf_the_trees_are_playout_searchs(ea, S):
    t = table(ea, S, *TABLE[S])
    b, d = fresh(ea, S, 9)
    for sims, n in ((4, 16), (0, 5)):
        got, c = ea.playout_search_exact(b, d, sims, t, playouts=n, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
        same(got, ea.playout_search(b, d, sims, playouts=n, key=KEY, obs_id0=OBS0), "fresh resets, sims %d" % sims)
        assert int(c[:, 0].sum()) == 0 and (c[:, 1] == sims + 1).all()


# ---------------------------------------------------------------- 4. the grid

@pytest.mark.parametrize("S,sims,n", [(5, 17, 7), (7, 6, 64)])
def test_the_grid(ea, S, sims, n):
    """five trees on one block: two trips, three waves of the second without a tree reach every barrier; nine on one block and on
    the default grid; one tree.  Each tree's bytes are its row's of the nine-tree yardstick (a tree's playouts are keyed by its row)"""
    t = table(ea, S, *TABLE[S])
    b9, d9 = rows(ea, S, 9)
    want, cwant = (x[-1] for x in staged(ea, t, b9, d9, sims, n, obs_id0=0))
    for M, blocks in ((5, 1), (9, 1), (9, None), (1, None), (1, 1)):
        for m0 in ((0, 4) if M < 9 else (0,)):
            got, c = ea.playout_search_exact(b9[m0:m0 + M], d9[m0:m0 + M], sims, t, playouts=n, key=KEY, obs_id0=m0, blocks=blocks,
                                             return_leaf_counts=True)
            same(got, want[m0:m0 + M], "M %d from row %d, blocks %s" % (M, m0, blocks))
            counts_equal(c, cwant[m0:m0 + M], "M %d from row %d, blocks %s" % (M, m0, blocks))


# ---------------------------------------------------------------- 5. sims = 0 and rounds = 0

@pytest.mark.parametrize("S", [5, 7])
def test_no_simulations_and_no_rounds(ea, S):
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, 9)
    for sims in (0, 6):
        got, c = ea.playout_search_exact(b, d, sims, t, rounds=0, return_leaf_counts=True)
        same(got, ea.puct_begin(b, d, sims)[0], "rounds 0, sims %d" % sims)
        assert int(c.abs().sum()) == 0
    snaps, csnaps = staged(ea, t, b, d, 0, 64)
    got, c = ea.playout_search_exact(b, d, 0, t, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    same(got, snaps[-1], "sims 0")
    counts_equal(c, csnaps[-1], "sims 0")
    assert csnaps[-1].sum(1).tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 1]           # the root's own round, where there is a root to search


# ---------------------------------------------------------------- 6. leaf counts

@pytest.mark.parametrize("S,M,sims,n", SHAPES)
def test_leaf_counts(ea, S, M, sims, n):
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, M)
    snaps, csnaps = reference(ea, S, M, sims, n)
    _, c = ea.playout_search_exact(b, d, sims, t, playouts=n, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    counts_equal(c, csnaps[-1], "all rounds")
    with_leaf = sum((views(ea, s, S, sims)["pending"] >= 0).astype(np.int32) for s in snaps[:-1])   # before each round, on the yardstick
    assert np.array_equal(c.cpu().numpy().sum(1), with_leaf)


# ---------------------------------------------------------------- 7. prior contents

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[1], SHAPES[2]])
def test_what_the_buffers_held_does_not_matter(ea, S, M, sims, n):
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, M)
    snaps, csnaps = reference(ea, S, M, sims, n)
    for fill in (0xA5, 0x00):
        tree = torch.full(tuple(snaps[-1].shape), fill, dtype=torch.uint8, device="cuda")
        counts = torch.full((M, 2 * 4), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
        lib_counts = ea.playout_search_exact(b, d, sims, t, playouts=n, key=KEY, obs_id0=OBS0, out=tree, return_leaf_counts=True)
        assert lib_counts[0] is tree
        same(tree, snaps[-1], "fill %#x" % fill)
        from ewn_gym_amd.playout_exact import _launch          # the binding allocates leaf_counts itself: the entry, on a filled buffer
        from ewn_gym_amd._args import _stream
        import ctypes as C
        tree.fill_(fill)
        _launch(ea._lib.load(), S, 3, M, sims, -1, n, C.c_float(1.5), KEY & MASK64, OBS0, 0, t, b, d, tree, counts, _stream())
        same(tree, snaps[-1], "fill %#x, the entry" % fill)
        counts_equal(counts, csnaps[-1], "fill %#x" % fill)


# ---------------------------------------------------------------- 8. guard zones

@pytest.mark.parametrize("S,M,sims,n,blocks", [(5, 5, 17, 7, 1), (7, 9, 6, 64, None)])
def test_guard_zones(ea, S, M, sims, n, blocks):
    import ctypes as C
    from ewn_gym_amd._args import _stream
    from ewn_gym_amd.playout_exact import _launch
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, M)
    snaps, csnaps = reference(ea, S, M, sims, n)
    alloc = GuardedAllocator()
    gb = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards")
    gd = alloc.zeros((M,), dtype=torch.int8, tag="dice")
    gt = alloc.zeros((t.table.numel(),), dtype=torch.float32, tag="table", offset=4)      # 4 bytes past a 16-byte boundary
    gb.copy_(b)
    gd.copy_(d)
    gt.copy_(t.table)
    guarded = ea.EndgameTable(S, *TABLE[S], gt)
    tree = alloc.zeros(tuple(snaps[-1].shape), dtype=torch.uint8, tag="tree", offset=4)
    counts = alloc.zeros((M, 2), dtype=torch.int32, tag="leaf_counts", offset=4)
    assert tree.data_ptr() % 16 == 4 and counts.data_ptr() % 16 == 4 and gt.data_ptr() % 16 == 4
    _launch(ea._lib.load(), S, 3, M, sims, -1, n, C.c_float(1.5), KEY & MASK64, OBS0, 0 if blocks is None else blocks, guarded, gb, gd, tree,
            counts, _stream())
    alloc.check("search, blocks %s" % blocks)
    same(tree, snaps[-1], "in guarded buffers")
    counts_equal(counts, csnaps[-1], "in guarded buffers")
    assert torch.equal(gt.view(torch.int32), t.table.view(torch.int32)), "the table is only read"


# ---------------------------------------------------------------- 9. dice outside 1..6 and malformed roots

@pytest.mark.parametrize("S", [5, 7])
def test_dice_outside_the_range_and_malformed_roots(ea, S):
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, 9)
    sims, n = 6, 64
    odd = torch.tensor([0, -3, 7, 100, -128, 127, 9, 0, 8], dtype=torch.int8, device="cuda")
    got = ea.playout_search_exact(b, odd, sims, t, playouts=n, key=KEY, obs_id0=OBS0)
    same(got, ea.playout_search_exact(b, odd.clamp(1, 6), sims, t, playouts=n, key=KEY, obs_id0=OBS0), "clamped dice")
    same(got, staged(ea, t, b, odd, sims, n)[0][-1], "dice outside 1..6 against the yardstick")
    bad = torch.zeros((2, S, S), dtype=torch.int8, device="cuda")
    bad[0, 1, 1], bad[0, 2, 2], bad[0, S - 2, S - 2] = 3, 3, -2          # a cube number twice
    bad[1, 1, 1], bad[1, S - 2, S - 2] = 7, -2                           # a cell value of 7
    db = torch.tensor([3, 2], dtype=torch.int8, device="cuda")
    assert not bool(t.lookup(bad, db)[1].any())
    snaps, csnaps = staged(ea, t, bad, db, sims, n)
    got, c = ea.playout_search_exact(bad, db, sims, t, playouts=n, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    same(got, snaps[-1], "malformed roots against the yardstick")
    counts_equal(c, csnaps[-1], "malformed roots")
    print("malformed roots: leaf counts %s" % c.tolist())
    by_playouts_alone = torch.as_tensor(csnaps[-1][:, 0] == 0).cuda()          # on the yardstick: no leaf of the tree was covered
    same(got[by_playouts_alone], ea.playout_search(bad, db, sims, playouts=n, key=KEY, obs_id0=OBS0)[by_playouts_alone], "trees that only played out")


# ---------------------------------------------------------------- 10. chunks and shards

@pytest.mark.parametrize("S", [5, 7])
def test_chunks_and_shards(ea, S):
    t = table(ea, S, *TABLE[S])
    b, d = rows(ea, S, 9)
    kw = dict(sims=9, playouts=20, key=KEY, return_visits=True, return_q=True, return_value=True, return_leaf_counts=True)
    whole = ea.predict_playout_search_exact(b, d, t, obs_id0=0, **kw)
    assert len(whole) == 5 and whole[4].dtype == torch.int32 and tuple(whole[4].shape) == (9, 2)
    for x, y in zip(ea.predict_playout_search_exact(b, d, t, obs_id0=0, chunk=4, **kw), whole):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    parts = [ea.predict_playout_search_exact(b[:4], d[:4], t, obs_id0=0, **kw), ea.predict_playout_search_exact(b[4:], d[4:], t, obs_id0=4, **kw)]
    for x0, x1, y in zip(parts[0], parts[1], whole):
        assert torch.equal(torch.cat([x0, x1]).view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(ea.predict_playout_search_exact(b, d, t, sims=9, playouts=20, key=KEY), whole[0])
    tree, c = ea.playout_search_exact(b, d, 9, t, playouts=20, key=KEY, return_leaf_counts=True)
    for x, y in zip(ea.puct_result(tree, S, 9, return_visits=True, return_q=True, return_value=True) + (c,), whole):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---------------------------------------------------------------- 11. the stream contract

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[0], SHAPES[3]])
def test_a_side_stream_is_honoured(ea, S, M, sims, n):
    """on a side stream behind a sleep: the copy of B into the inputs, the fill of the outputs, the call, the copies out.  Only that
    stream is synchronised.  A launch on any other stream reads A behind the sleep's back and is overwritten by the fill."""
    from tests.test_gpu_playout_search import sleep_cycles
    t = table(ea, S, *TABLE[S])
    bB, dB = rows(ea, S, M)
    bA, dA = other_rows(ea, S, M)
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0)
    EA, EB = ea.playout_search_exact(bA, dA, sims, t, **kw), reference(ea, S, M, sims, n)[0][-1]
    assert not torch.equal(EA, EB)
    b, d, tree = bA.clone(), dA.clone(), torch.full_like(EB, 0x3C)
    cycles = sleep_cycles()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        b.copy_(bB)
        d.copy_(dB)
        tree.fill_(0xA5)
        _, c = ea.playout_search_exact(b, d, sims, t, out=tree, return_leaf_counts=True, **kw)
        got, gotc = tree.clone(), c.clone()
    s.synchronize()
    same(got, EB, "on a side stream")
    counts_equal(gotc, reference(ea, S, M, sims, n)[1][-1], "on a side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,M,sims,n", [SHAPES[0], SHAPES[3]])
def test_a_captured_graph_replays_like_eager_calls(ea, S, M, sims, n):
    """the table is built before the capture; captured once, replayed on A, on B and on A again, the tree refilled between, against
    eager calls"""
    import ctypes as C
    from ewn_gym_amd._args import _stream
    from ewn_gym_amd.playout_exact import _launch
    t = table(ea, S, *TABLE[S])
    bB, dB = rows(ea, S, M)
    bA, dA = other_rows(ea, S, M)
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0, return_leaf_counts=True)
    eager = [ea.playout_search_exact(bA, dA, sims, t, **kw), ea.playout_search_exact(bB, dB, sims, t, **kw)]
    eager.append(eager[0])
    same(eager[1][0], reference(ea, S, M, sims, n)[0][-1], "the eager call")
    assert not torch.equal(eager[0][0], eager[1][0])
    b, d, tree = bA.clone(), dA.clone(), torch.full_like(eager[0][0], 0x5A)
    counts = torch.full((M, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        _launch(ea._lib.load(), S, 3, M, sims, -1, n, C.c_float(1.5), KEY & MASK64, OBS0, 0, t, b, d, tree, counts, _stream())
    torch.cuda.synchronize()
    assert bool((tree == 0x5A).all()) and bool((counts == 0x5A5A5A5A).all()), "the captured call ran during the capture"
    for k, (xb, xd) in enumerate(((bA, dA), (bB, dB), (bA, dA))):
        b.copy_(xb)
        d.copy_(xd)
        tree.fill_(0xA5)
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        same(tree, eager[k][0], "replay %d" % (k + 1))
        assert torch.equal(counts, eager[k][1]), "replay %d" % (k + 1)


# ---------------------------------------------------------------- 12. the agent, the spec and one tournament row

def test_the_agent_the_spec_and_one_tournament_row(ea, tmp_path):
    from classical_policies import PlayoutSearchAgent
    from ewn_gym_amd.playout_search import KEY_PLY
    from ewn_gym_amd.tournament import _row, evaluate, tournament
    t = table(ea, 5, *TABLE[5])
    b, d = rows(ea, 5, 9)
    agent = PlayoutSearchAgent(3, 5, sims=8, playouts=16, c_puct=1.25, seed=1, endgame_table=t)
    kw = dict(return_visits=True, return_value=True, return_leaf_counts=True)
    want = ea.predict_playout_search_exact(b, d, t, sims=8, playouts=16, c_puct=1.25, key=99, obs_id0=7, **kw)
    for x, y in zip(agent.predict_batch(b, d, key=99, obs_id0=7, **kw), want):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert int(want[3][:, 0].sum()) > 0                        # the table valued leaves
    assert torch.equal(agent.predict_batch(b.cpu().numpy(), d.cpu().numpy(), key=99, obs_id0=7), want[0])
    plain = PlayoutSearchAgent(3, 5, sims=8, playouts=16, c_puct=1.25, seed=1)
    assert torch.equal(plain.predict_batch(b, d, key=99, obs_id0=7), ea.predict_playout_search(b, d, sims=8, playouts=16, c_puct=1.25, key=99, obs_id0=7))
    with pytest.raises(ValueError, match="return_leaf_counts goes with an endgame_table"):
        plain.predict_batch(b, d, key=99, return_leaf_counts=True)
    with pytest.raises(ValueError, match="PlayoutSearchAgent: the table is for 7x7 boards, the agent plays 5x5"):
        PlayoutSearchAgent(3, 5, endgame_table=table(ea, 7, *TABLE[7]))
    small = ea.EndgameTable.build(5, 1, 2)                     # a saved table by its path, in the agent and in the spec
    small.save(tmp_path / "t.pt")
    loaded = PlayoutSearchAgent(3, 5, sims=8, playouts=16, seed=1, endgame_table=str(tmp_path / "t.pt"))
    assert (loaded.endgame_table.max_cubes, loaded.endgame_table.max_total) == (1, 2) and torch.equal(loaded.endgame_table.table, small.table)
    num, key = 8, 12345                                        # evaluate's own key
    by_hand = lambda bb, dd, step: ea.predict_playout_search_exact(bb, dd, t, sims=8, playouts=16, c_puct=1.5,   # noqa: E731
                                                                   key=(key + KEY_PLY * (step + 1)) & MASK64)
    spec = {"kind": "playout_search", "sims": 8, "playouts": 16, "endgame_table": t}
    r0, r1 = evaluate(spec, {"kind": "random"}, num=num), evaluate(by_hand, {"kind": "random"}, num=num)
    assert (r0["wins"], r0["avg_length"], r0["engine"]) == (r1["wins"], r1["avg_length"], "ewn_step") and r0["episodes"] == num
    assert torch.equal(r0["scores"], r1["scores"]) and torch.equal(r0["lengths"], r1["lengths"])
    row = tournament(("random", "playout_search"), num=num, sims=8, playouts=16, playout_table=t)["playout_search vs random"]
    assert row == _row(r0)
