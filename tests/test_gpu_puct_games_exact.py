"""Whole self-play games in one launch with exact endgame values at covered leaves (ewn_puct_selfplay_eg, selfplay_puct_games_exact,
games_table=) against selfplay_puct(leaf_table=), the lock-step path with one ewn_puct_search_eg and one ewn_puct_play
per ply, and leaf_counts against the per-ply sum of puct_search_exact(return_leaf_counts=True) on the recorded rows.  The tree code,
the move, the network code, the coverage test and the table's gather are the same on both paths, so there is no tolerance anywhere in
this file: every comparison is of all bytes of all records and of leaf_counts, and any difference is a bug.
Tables: the session's (5, 2, 4) and (7, 2, 3), built once by tests/test_gpu_endgame.py's table() and left unchanged.
1. the records.  2. leaf_counts.  3. reset positions.  4. terminal_value, no noise, keys, again.  5. one game and seventy; games that
are not played.  6. guard zones.  7. shards.  8. streams and graphs.  9. the counters' width.  10. the trainer and the command line."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_endgame import table  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct_exact import TABLE, sampled  # noqa: E402
from tests.test_gpu_puct_fused import planted  # noqa: E402
from tests.test_gpu_puct_selfplay import ROWS, reset_positions, row_shapes, same_records, selfplay_trainer  # noqa: E402

GEOMETRIES = ((None, None), (32, 1), (2, 1), (3, 2), (1, 5))   # (tile, blocks); None: the library's choice
# (own, opposing) cubes of the eight few-cube starts: covered ones, ones a cube outside the table, larger ones.  5x5: the mix of
# test_gpu_puct_exact.py::test_selfplay_puct_with_a_leaf_table
MIX = {5: [(2, 2), (3, 2), (2, 3), (1, 2), (3, 3), (2, 1), (3, 2), (2, 2)], 7: [(1, 2), (2, 2), (2, 2), (2, 1), (3, 3), (2, 1), (3, 2), (1, 2)]}
SEED = {5: 70, 7: 70}          # of the sampled starts: chosen so that case 1's counts hold
WIDE_SEED = 21                 # of case 9's reset position: its game lasts long enough
KW = dict(sims=8, max_plies=12, temp_plies=4, key=15, game_offset=2 ** 32 + 5)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_REF = {}


def ten(ea, S):
    """eight few-cube starts and two reset positions"""
    b, d = sampled(S, MIX[S], SEED[S])
    rb, rd = reset_positions(ea, S, 2)
    return torch.cat([b, rb.reshape(2, S, S)]).contiguous(), torch.cat([d, rd]).contiguous()


def seventy(ea, S):
    """70 starts: few-cube starts, reset positions and planted rows (already won, already lost, a side without a cube, an empty board)
    between them"""
    b, d = sampled(S, MIX[S] * 4, SEED[S] + 1)
    rb, rd = reset_positions(ea, S, 24)
    pb, pd, _ = planted(S)
    b, d = torch.cat([b, rb.reshape(24, S, S), pb.cuda()]), torch.cat([d, rd, pd.cuda()])
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(S)).cuda()
    return b[perm].contiguous(), d[perm].contiguous()


def yard_counts(ea, t, rec, params, sims, key, off, eps=0.25, alpha=1.0, c_puct=1.5, tv=1.0):
    """the yardstick of leaf_counts from public calls: per ply puct_search_exact(return_leaf_counts=True) on the recorded live rows
    with that ply's selfplay_noise rows, summed over the plies -> int32 [M, 2]"""
    T, M = rec["live"].shape
    total = torch.zeros((M, 2), dtype=torch.int32, device="cuda")
    for ply in range(T):
        idx = torch.nonzero(rec["live"][ply]).reshape(-1)
        if idx.numel() == 0:
            continue
        noise = ea.selfplay_noise(M, alpha, key, off, ply)[idx].contiguous() if eps > 0 else None
        _, c = ea.puct_search_exact(rec["board"][ply, idx].contiguous(), rec["dice"][ply, idx].contiguous(), params, sims, t, c_puct=c_puct,
                                    terminal_value=tv, root_noise=noise, noise_eps=eps, return_leaf_counts=True)
        total[idx] += c
    return total


def reference(ea, S, what="ten"):
    """computed once per board and left unchanged: the starts, selfplay_puct(leaf_table=)'s records of them and the yardstick's counts"""
    if (S, what) not in _REF:
        t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
        b, d = ten(ea, S) if what == "ten" else seventy(ea, S)
        want = ea.selfplay_puct(b, d, params, leaf_table=t, **KW)
        _REF[(S, what)] = (b, d, want, yard_counts(ea, t, want, params, KW["sims"], KW["key"], KW["game_offset"]))
    return _REF[(S, what)]


def counts_equal(got, want, where=""):
    assert got.dtype == torch.int32 and got.shape == want.shape, where
    assert torch.equal(got, want), "%s: leaf counts %s, the yardstick's %s" % (where, got.tolist(), want.tolist())


def same_with_counts(got, want, cwant, where=""):
    got = dict(got)
    counts_equal(got.pop("leaf_counts"), cwant, where)
    same_records(got, want)


def covered_roots(t, rec):
    T, M, S = rec["board"].shape[:3]
    cov = t.lookup(rec["board"].reshape(T * M, S, S), rec["dice"].reshape(T * M).clamp(min=1))[1].reshape(T, M)
    assert not bool((cov & ~rec["live"]).any())
    return cov


# ---------------------------------------------------------------- 1. the records, 2. leaf_counts

@pytest.mark.parametrize("S", [5, 7])
def test_the_records_and_the_counts_are_the_lock_step_path_s(ea, S):
    """fails without the feature: the entry and the module do not exist"""
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, want, cwant = reference(ea, S)
    cov = covered_roots(t, want)                                   # counted on the yardstick, before anything is compared
    later = ~cov[0] & cov[1:].any(0)
    print("S=%d: %d recorded roots, %d covered at ply 0, %d games covered only later; leaves by table / by the value head per game %s" % (
        S, int(want["live"].sum()), int(cov[0].sum()), int(later.sum()), cwant.tolist()))
    assert int(cov[0].sum()) > 0 and int(later.sum()) > 0
    assert int(cwant[:, 0].sum()) > 0 and int(cwant[:, 1].sum()) > 0 and bool(((cwant[:, 0] > 0) & (cwant[:, 1] > 0)).any())
    assert bool((cwant.sum(1) <= (KW["sims"] + 1) * want["plies"]).all())
    b0, d0 = b.clone(), d.clone()
    for tile, blocks in GEOMETRIES:
        got = ea.selfplay_puct_games_exact(b, d, params, t, tile=tile, blocks=blocks, return_leaf_counts=True, **KW)
        same_with_counts(got, want, cwant, "tile %s blocks %s" % (tile, blocks))
    same_records(ea.selfplay_puct_games_exact(b, d, params, t, **KW), want)       # without the counts: selfplay_puct's keys
    assert torch.equal(b, b0) and torch.equal(d, d0)               # the inputs are not changed
    plain = ea.selfplay_puct_games(b, d, params, **KW)
    assert any(not torch.equal(plain[k], want[k]) for k in ("visits", "value", "action"))          # the table is read: other searches


# ---------------------------------------------------------------- 3. reset positions

@pytest.mark.parametrize("S", [5, 7])
def test_reset_positions_without_a_table_leaf_are_the_plain_games(ea, S):
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d = reset_positions(ea, S, 33)
    kw = dict(sims=8, max_plies=6, key=11, game_offset=5)
    want = ea.selfplay_puct(b, d, params, leaf_table=t, **kw)
    cwant = yard_counts(ea, t, want, params, 8, 11, 5)
    none = cwant[:, 0] == 0                                        # the games without a table leaf, counted on the yardstick
    assert int(none.sum()) > 0 and bool((cwant[none, 1] > 0).all())
    print("S=%d: %d of 33 reset games without a table leaf" % (S, int(none.sum())))
    for tile, blocks in ((None, None), (4, 2)):
        got = ea.selfplay_puct_games_exact(b, d, params, t, tile=tile, blocks=blocks, return_leaf_counts=True, **kw)
        same_with_counts(got, want, cwant)
    plain = ea.selfplay_puct_games(b, d, params, **kw)
    for k in plain:
        dim = 0 if plain[k].dim() == 1 else 1
        x, y = got[k].movedim(dim, 0)[none].contiguous(), plain[k].movedim(dim, 0)[none].contiguous()
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


# ---------------------------------------------------------------- 4. terminal_value, no noise, keys, again

@pytest.mark.parametrize("S", [5, 7])
def test_terminal_value_without_noise_other_keys_and_again(ea, S):
    """10.0 is no power of two: fl(fl(tv * q) * fl(1 / tv)) is not q, and both roundings show"""
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, noisy, _ = reference(ea, S)
    for tv in (0.5, 10.0):
        kw = dict(KW, terminal_value=tv, c_puct=1.25)
        want = ea.selfplay_puct(b, d, params, leaf_table=t, **kw)
        cwant = yard_counts(ea, t, want, params, 8, KW["key"], KW["game_offset"], c_puct=1.25, tv=tv)
        assert int(cwant[:, 0].sum()) > 0 and int(cwant[:, 1].sum()) > 0
        same_with_counts(ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **kw), want, cwant, "terminal_value %g" % tv)
    kw = dict(KW, noise_eps=0.0)                                   # the instances without noise
    want = ea.selfplay_puct(b, d, params, leaf_table=t, **kw)
    cwant = yard_counts(ea, t, want, params, 8, KW["key"], KW["game_offset"], eps=0.0)
    assert not torch.equal(want["visits"], noisy["visits"]) and int(cwant[:, 0].sum()) > 0
    for tile, blocks in ((None, None), (3, 2)):
        got = ea.selfplay_puct_games_exact(b, d, params, t, tile=tile, blocks=blocks, return_leaf_counts=True, **kw)
        same_with_counts(got, want, cwant, "without noise")
    kw = dict(KW, key=16)                                          # a second key: other games, on both paths the same
    other = ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **kw)
    want = ea.selfplay_puct(b, d, params, leaf_table=t, **kw)
    same_with_counts(other, want, yard_counts(ea, t, want, params, 8, 16, KW["game_offset"]), "key 16")
    assert not torch.equal(other["action"], noisy["action"])
    again = ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **kw)          # the same arguments: the same bytes
    same_with_counts(again, {k: v for k, v in other.items() if k != "leaf_counts"}, other["leaf_counts"], "again")


# ---------------------------------------------------------------- 5. one game and seventy; games that are not played

@pytest.mark.parametrize("S", [5, 7])
def test_one_game_and_seventy(ea, S):
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, want, cwant = reference(ea, S, "seventy")
    dead = ~want["live"][0]                                        # the planted rows that are no game: no row, no ply, no count
    cut = want["live"][KW["max_plies"] - 1] & (want["winner"] == 0)
    assert int(dead.sum()) >= 4 and bool((cwant[dead] == 0).all()) and not bool(want["plies"][dead].any())
    assert bool(cut.any()) and bool((want["plies"][cut] == KW["max_plies"]).all()) and bool((want["winner"] != 0).any())
    assert int(cwant[:, 0].sum()) > 0 and int(cwant[:, 1].sum()) > 0
    for tile, blocks in ((None, None), (8, 2)):                    # (8, 2): 16 columns for 70 games, every column is refilled
        got = ea.selfplay_puct_games_exact(b, d, params, t, tile=tile, blocks=blocks, return_leaf_counts=True, **KW)
        same_with_counts(got, want, cwant, "M 70, tile %s blocks %s" % (tile, blocks))
    for m in (0, 3, 9):                                            # one game: the shard of one
        kw = dict(KW, game_offset=KW["game_offset"] + m)
        b1, d1 = b[m:m + 1].contiguous(), d[m:m + 1].contiguous()
        one = ea.selfplay_puct(b1, d1, params, leaf_table=t, **kw)
        c1 = yard_counts(ea, t, one, params, 8, KW["key"], kw["game_offset"])
        for tile, blocks in ((None, None), (8, 2)):
            got = ea.selfplay_puct_games_exact(b1, d1, params, t, tile=tile, blocks=blocks, return_leaf_counts=True, **kw)
            same_with_counts(got, one, c1, "game %d alone" % m)
        counts_equal(c1, cwant[m:m + 1], "game %d alone against the seventy" % m)


def abi_call(ea, S, t, b, d, params, sims, T, tile, blocks, key, off, temp_plies=4, eps=0.25, tv=1.0, fill=None, game=None, skip=None,
             alloc=None, counts=True, buffers=None, launch_only=False):
    """ewn_puct_selfplay_eg through the C ABI on buffers of exactly the needed bytes -> a dict of every buffer.  fill: the byte that the
    scratch, the records and leaf_counts hold before the call; alloc: a GuardedAllocator, every buffer -- a copy of the table among
    them -- then starts 4 bytes past a 16-byte boundary; skip: the record pointer that is NULL; counts False: leaf_counts NULL;
    buffers: an earlier call's, used again; launch_only: nothing but the call (what a graph captures)"""
    from ewn_gym_amd._args import _ptr, _stream
    lib = ea._lib.load()
    if buffers is None:
        M = b.shape[0]
        z = (lambda shape, dtype, tag: alloc.zeros(shape, dtype=dtype, tag=tag, offset=4)) if alloc is not None else (
            lambda shape, dtype, tag: torch.zeros(shape, dtype=dtype, device="cuda"))
        x = {"rec": {k: z((T, M) + s, dt, "rec_" + k) for k, (s, dt) in row_shapes(S).items()}}
        nscr = int(lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, tile, blocks))
        assert nscr > 0 and nscr % lib.ewn_puct_tree_bytes(S, 3, sims) == 0
        x["scratch"] = z((nscr,), torch.uint8, "scratch")
        x["boards"], x["dice"], x["game"] = z((M, S, S), torch.int8, "boards"), z((M,), torch.int8, "dice"), z((M, 4), torch.int32, "game")
        x["params"] = z((params.numel(),), torch.float32, "params")
        x["table"] = z((t.table.numel(),), torch.float32, "table") if alloc is not None else t.table
        x["noise"] = z((T, M, 6), torch.float32, "noise") if eps > 0 else None
        x["counts"] = z((M, 2), torch.int32, "leaf_counts")
        if alloc is not None:
            assert all(v.data_ptr() % 16 == 4 for v in list(x["rec"].values()) + [v for k, v in x.items() if k != "rec" and v is not None])
    else:
        x = buffers
    M = x["boards"].shape[0]
    if not launch_only:
        x["boards"].copy_(b)
        x["dice"].copy_(d)
        x["params"].copy_(params.reshape(-1))
        if x["table"] is not t.table:
            x["table"].copy_(t.table.reshape(-1))
        x["game"].zero_() if game is None else x["game"].copy_(game)
        if x["noise"] is not None:
            x["noise"].copy_(torch.stack([ea.selfplay_noise(M, 1.0, key, off, ply) for ply in range(T)]))
        if fill is not None:
            for v in list(x["rec"].values()) + [x["scratch"], x["counts"]]:
                v.view(torch.uint8).fill_(fill)
    rc = lib.ewn_puct_selfplay_eg(S, 3, M, sims, T, C.c_float(1.5), C.c_float(tv), _ptr(x["params"]), _ptr(x["noise"]), C.c_float(eps), temp_plies,
                                  C.c_uint64(key), C.c_int64(off), tile, blocks, _ptr(x["boards"]), _ptr(x["dice"]), _ptr(x["game"]),
                                  *[_ptr(None if k == skip else x["rec"][k]) for k in ROWS], _ptr(x["scratch"]), t.max_cubes, t.max_total,
                                  _ptr(x["table"]), _ptr(x["counts"] if counts else None), _stream())
    assert rc == 0
    return x


def rows_equal(x, want, cols=None, skip=None):
    for k in ROWS:
        if k == skip:
            continue
        T, M = want["live"].shape
        got, ref = x["rec"][k].view(torch.uint8).reshape(T, M, -1), want[k].contiguous().view(torch.uint8).reshape(T, M, -1)
        if cols is not None:
            got, ref = got[:, cols], ref[:, cols]
        assert torch.equal(got, ref), k


def one_game_by_hand(ea, t, S, b, d, g, m, M, params, sims, T, key, off, temp_plies=4):
    """game m of M from the state (b, d, g) it enters with, in the public calls: per ply puct_search_exact with row m of that ply's noise
    and puct_play with game_offset + m -> (its record rows [T, ...] by name, its counts [2], board, dice, game afterwards)"""
    b, d, g = b.reshape(1, S, S).clone(), d.reshape(1).clone(), g.reshape(1, 4).clone()
    rec = {k: torch.zeros((T, 1) + s, dtype=dt, device="cuda") for k, (s, dt) in row_shapes(S).items()}
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    while True:
        ply, over = int(g[0, 0]), int(g[0, 1])
        if over != 0 or ply < 0 or ply >= T:
            break
        noise = ea.selfplay_noise(M, 1.0, key, off, ply)[m:m + 1].contiguous()
        tree, c = ea.puct_search_exact(b, d, params, sims, t, root_noise=noise, noise_eps=0.25, return_leaf_counts=True)
        counts += c[0]
        ea.puct_play(tree, b, d, g, S, sims, temp_plies=temp_plies, key=key, game_offset=off + m, out={k: rec[k][ply] for k in rec})
    return rec, counts, b, d, g


@pytest.mark.parametrize("S", [5, 7])
def test_games_that_are_not_played_and_games_that_enter_late(ea, S):
    """through the C ABI, where `game` is the caller's: a game that enters over, at ply >= max_plies or at a negative ply has zero
    rows, zero counts and an untouched state; a game that enters at ply 2 or 9 counts the plies played here"""
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, want, cwant = reference(ea, S)
    M, T, sims, key, off = 10, KW["max_plies"], KW["sims"], KW["key"], KW["game_offset"]
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    game[1] = torch.tensor([3, 1, -1, 7])
    game[2] = torch.tensor([0, 1, 0, 0])
    game[4] = torch.tensor([T, 0, 0, 0])
    game[5] = torch.tensor([T + 5, 0, 0, -1])
    game[9] = torch.tensor([-1, 0, 0, 0])
    game[3] = torch.tensor([2, 0, 0, 0])                           # enter late: rows below are zeros, the plies from there on are played
    game[8] = torch.tensor([9, 0, 0, 0])
    game[6, 3] = 0x5A5A                                            # word 3 is nobody's
    idle, late, plain = torch.tensor([1, 2, 4, 5, 9], device="cuda"), (3, 8), torch.tensor([0, 6, 7], device="cuda")
    hand = {m: one_game_by_hand(ea, t, S, b[m], d[m], game[m], m, M, params, sims, T, key, off) for m in late}
    assert all(int(hand[m][1].sum()) >= 1 and int(hand[m][0]["live"][int(game[m, 0])].sum()) == 1 for m in late)   # they are played
    for tile, blocks in ((0, 0), (2, 2)):
        x = abi_call(ea, S, t, b, d, params, sims, T, tile, blocks, key, off, fill=0xFF, game=game)
        torch.cuda.synchronize()
        rows_equal(x, want, cols=plain)
        counts_equal(x["counts"][plain], cwant[plain], "games from ply 0")
        for k in ROWS:
            assert not bool(x["rec"][k][:, idle].view(torch.uint8).any()), k           # every row of a game that is not played: zeros
        assert not bool(x["counts"][idle].any())
        assert torch.equal(x["game"][idle], game[idle]) and torch.equal(x["boards"][idle], b[idle]) and torch.equal(x["dice"][idle], d[idle])
        assert int(x["game"][6, 3]) == 0x5A5A
        for m in late:
            rec, c, b1, d1, g1 = hand[m]
            for k in ROWS:
                assert torch.equal(x["rec"][k][:, m].contiguous().view(torch.uint8), rec[k][:, 0].contiguous().view(torch.uint8)), (m, k)
            counts_equal(x["counts"][m], c, "game %d enters at ply %d" % (m, int(game[m, 0])))
            assert torch.equal(x["boards"][m], b1[0]) and torch.equal(x["dice"][m], d1[0]) and torch.equal(x["game"][m], g1[0])


# ---------------------------------------------------------------- 6. guard zones

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones_and_what_the_buffers_held(ea, S):
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, want, cwant = reference(ea, S)
    T, sims, key, off = KW["max_plies"], KW["sims"], KW["key"], KW["game_offset"]
    noise = torch.stack([ea.selfplay_noise(10, 1.0, key, off, ply) for ply in range(T)])
    alloc, x = GuardedAllocator(), None                            # guard zones round every buffer, allocated once: the table's copy is large
    for fill, skips in ((0xFF, ROWS + (None,)), (0x7F, (None,))):
        for skip in skips:                                         # the record pointers NULL one by one
            x = abi_call(ea, S, t, b, d, params, sims, T, 3, 2, key, off, fill=fill, skip=skip, alloc=alloc, buffers=x)
            torch.cuda.synchronize()
            alloc.check("fill %#x, without %s" % (fill, skip))
            rows_equal(x, want, skip=skip)
            if skip is not None:
                assert bool((x["rec"][skip].view(torch.uint8) == fill).all()), skip     # ... and the buffer behind it is not written
            counts_equal(x["counts"], cwant, "fill %#x, without %s" % (fill, skip))
            assert torch.equal(x["game"][:, 0], want["plies"]) and torch.equal(x["game"][:, 2], want["winner"])
            assert torch.equal(x["table"].view(torch.int32), t.table.reshape(-1).view(torch.int32)), "the table is only read"
            assert torch.equal(x["params"].view(torch.int32), params.reshape(-1).view(torch.int32))
            assert torch.equal(x["noise"].view(torch.int32), noise.view(torch.int32))
    x = abi_call(ea, S, t, b, d, params, sims, T, 3, 2, key, off, fill=0xFF, alloc=alloc, counts=False, buffers=x)   # leaf_counts NULL
    torch.cuda.synchronize()
    alloc.check("without leaf_counts")
    rows_equal(x, want)
    assert bool((x["counts"].view(torch.uint8) == 0xFF).all())


# ---------------------------------------------------------------- 7. shards

@pytest.mark.parametrize("S", [5, 7])
def test_two_shards_are_the_whole(ea, S):
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d, want, cwant = reference(ea, S, "seventy")
    off = KW["game_offset"]
    lo = ea.selfplay_puct_games_exact(b[:33], d[:33], params, t, return_leaf_counts=True, **KW)
    hi = ea.selfplay_puct_games_exact(b[33:], d[33:], params, t, return_leaf_counts=True, **dict(KW, game_offset=off + 33))
    for k in want:
        dim = 0 if want[k].dim() == 1 else 1                       # winner, plies [M]; every other [T, M, ...]
        assert torch.equal(torch.cat([lo[k], hi[k]], dim), want[k]), k
    counts_equal(torch.cat([lo["leaf_counts"], hi["leaf_counts"]]), cwant, "33 + 37")


# ---------------------------------------------------------------- 8. streams and graphs

@pytest.mark.parametrize("S", [5, 7])
def test_a_side_stream_is_honoured(ea, S):
    """on a side stream behind a sleep: the copy of B into the inputs, then the call.  Only that stream is synchronised.  A launch on
    any other stream reads A behind the sleep's back"""
    from tests.test_gpu_playout_search import sleep_cycles
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    bB, dB, want, cwant = reference(ea, S)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    assert not torch.equal(ea.selfplay_puct_games_exact(bA, dA, params, t, **KW)["board"], want["board"])
    b, d = bA.clone(), dA.clone()
    cycles = sleep_cycles()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        b.copy_(bB)
        d.copy_(dB)
        got = ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **KW)
    s.synchronize()
    same_with_counts(got, want, cwant, "on a side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [5, 7])
def test_a_captured_graph_replays_like_eager_calls(ea, S):
    """one chain: the copies of the inputs, then the launch; the table is built before the capture.  Captured once, replayed on A, on
    B and on A again, the outputs refilled between"""
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    bB, dB, wantB, cB = reference(ea, S)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    T, sims, key, off = KW["max_plies"], KW["sims"], KW["key"], KW["game_offset"]
    eager = [ea.selfplay_puct_games_exact(bA, dA, params, t, return_leaf_counts=True, **KW), dict(wantB, leaf_counts=cB)]
    eager.append(eager[0])
    assert not torch.equal(eager[0]["board"], eager[1]["board"])
    x = abi_call(ea, S, t, bA, dA, params, sims, T, 0, 0, key, off)            # an eager call first: the buffers, the noise, the table's copy
    torch.cuda.synchronize()
    rows_equal(x, eager[0])
    src_b, src_d, src_g = bA.clone(), dA.clone(), torch.zeros((10, 4), dtype=torch.int32, device="cuda")
    fills = list(x["rec"].values()) + [x["counts"], x["scratch"]]
    for v in fills:
        v.view(torch.uint8).fill_(0x5A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        x["boards"].copy_(src_b)
        x["dice"].copy_(src_d)
        x["game"].copy_(src_g)
        abi_call(ea, S, t, None, None, None, sims, T, 0, 0, key, off, buffers=x, launch_only=True)
    torch.cuda.synchronize()
    assert all(bool((v.view(torch.uint8) == 0x5A).all()) for v in fills), "the captured call ran during the capture"
    for k, (xb, xd) in enumerate(((bA, dA), (bB, dB), (bA, dA))):
        src_b.copy_(xb)
        src_d.copy_(xd)
        for v in fills:
            v.view(torch.uint8).fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        rows_equal(x, eager[k])
        counts_equal(x["counts"], eager[k]["leaf_counts"], "replay %d" % (k + 1))
        assert torch.equal(x["game"][:, 0], eager[k]["plies"]) and torch.equal(x["game"][:, 2], eager[k]["winner"])


# ---------------------------------------------------------------- 9. the counters' width

def test_a_count_above_65535(ea):
    """one 7x7 game from a reset with 4 096 simulations a ply: 4 097 rounds a ply, so a 16-bit counter wraps within 16 plies"""
    S, sims, T = 7, 4096, 24
    t, params = table(ea, S, *TABLE[S]), pool(ea, S)["params"]
    b, d = reset_positions(ea, S, WIDE_SEED + 1)
    b, d = b.reshape(-1, S, S)[WIDE_SEED:].contiguous(), d[WIDE_SEED:].contiguous()
    kw = dict(sims=sims, max_plies=T, temp_plies=4, key=3, game_offset=9)
    want = ea.selfplay_puct(b, d, params, leaf_table=t, **kw)
    cwant = yard_counts(ea, t, want, params, sims, 3, 9)
    print("plies %d, leaves by table / by the value head %s" % (int(want["plies"][0]), cwant.tolist()))
    assert int(cwant.max()) > 65535                               # counted on the yardstick, before anything is compared
    got = ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **kw)
    same_with_counts(got, want, cwant, "one long game")


# ---------------------------------------------------------------- 10. the trainer and the command line

def test_the_trainer_takes_a_games_table(ea, tmp_path):
    t = table(ea, 5, *TABLE[5])
    tr, ref = selfplay_trainer(ea, games_table=t), selfplay_trainer(ea, leaf_table=t)
    assert tr.games_table is t and tr.leaf_table is None and ref.games_table is None and selfplay_trainer(ea).games_table is None
    for update in range(2):                                        # the second update plays other games, on both paths the same
        tr.collect_and_update()
        ref.collect_and_update()
        same_records(tr.records, ref.records)
        assert torch.equal(bits(tr.grad), bits(ref.grad)) and torch.equal(bits(tr.params), bits(ref.params)), update
    cov = covered_roots(t, ref.records)
    print("the trainer's last update: %d recorded roots, %d covered" % (int(ref.records["live"].sum()), int(cov.sum())))
    path = str(tmp_path / "selfplay.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["games_table_used"] is True and sd["leaf_table_used"] is False and sd["algorithm"] == "SELFPLAY"
    assert not any(isinstance(v, torch.Tensor) and v.numel() == t.table.numel() for v in sd.values())   # that one was used, not its bytes
    ref.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["games_table_used"] is False and sd["leaf_table_used"] is True
    small = ea.EndgameTable.build(5, 1, 2)                         # a saved table by its path: loaded once, on the env's device
    small.save(str(tmp_path / "t.pt"))
    by_path = selfplay_trainer(ea, games_table=str(tmp_path / "t.pt"))
    assert torch.equal(by_path.games_table.table, small.table) and by_path.games_table.table.device == by_path.params.device
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: the games table is for 7x7 boards, the env plays 5x5"):
        selfplay_trainer(ea, games_table=table(ea, 7, *TABLE[7]))


def test_train_a2c_selfplay_games_table_end_to_end(ea, tmp_path):
    """two epochs of one update each with tiny numbers, in a fresh child process: the command line is what this test is about"""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ea.EndgameTable.build(5, 1, 2).save(str(tmp_path / "t.pt"))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SELFPLAY", "--games_table", str(tmp_path / "t.pt"), "--num_envs", "64",
                        "--sims", "4", "--epoch_num", "2", "--timesteps_per_epoch", "300", "--eval_episode_num", "16", "--eval_opponent",
                        "random", "--save_dir", str(tmp_path)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert any(x.get("trainer") == "PuctSelfPlayTrainer" for x in lines)
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 2 and all(math.isfinite(x["policy_loss"]) and 6 <= x["mean_game_length"] <= 69 and x["finished_fraction"] == 1.0 for x in ep)
    sd = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["sims"], sd["games_table_used"], sd["leaf_table_used"], sd["whole_games"]) == ("SELFPLAY", 4, True, False, False)
