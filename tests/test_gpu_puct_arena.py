"""The arena (ewn_puct_arena, arena_puct_games, tournament.arena) against arena_puct, its staged definition, and the
definition against the public calls composed.  The tree code, the move (csrc/ewn_puct.hpp), the network code and the compiler flags
are the same on every path, so there is no tolerance anywhere in this file: every comparison is of all bytes of all records, and any
difference is a bug.  How many columns a block has and how many blocks share the games changes no byte either.
1. the definition.  2. equal networks are self-play.  3. swapping sides.  4. phases.  5. cut games and entering plies.  6. buffers.
7. shards.  8. the tournament and the command line."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_policy import make_model, pool  # noqa: E402
from tests.test_gpu_puct_selfplay import ROWS, check_rules, reset_positions, row_shapes, same_records  # noqa: E402

GEOMETRIES = ((None, None), (32, 1), (2, 1), (3, 2), (1, 5))   # (tile, blocks); None: the library's choice
MAX_PLIES = {5: 80, 7: 128}
KW = dict(sims=8, key=11, game_offset=2 ** 32 + 5)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_NETS, _REF = {}, {}


def nets(ea, S):
    """two different networks of one size: the pool's (seed 5) and a second one (seed 9), computed once"""
    if S not in _NETS:
        _NETS[S] = (pool(ea, S)["params"], make_model(S, 9).flat_parameters())
        assert not torch.equal(*_NETS[S])
    return _NETS[S]


def alternate(M):
    return (torch.arange(M, device="cuda") & 1).to(torch.int8)


def reference(ea, S, M, first="alternate"):
    """computed once per shape and left unchanged: M reset positions, their first column and arena_puct's records of them (the staged
    definition)"""
    if (S, M, first) not in _REF:
        b, d = reset_positions(ea, S, M)
        f = alternate(M) if first == "alternate" else torch.full((M,), int(first), dtype=torch.int8, device="cuda")
        _REF[(S, M, first)] = (b, d, f, ea.arena_puct(b, d, *nets(ea, S), f, **KW))
    return _REF[(S, M, first)]


def by_hand(ea, S, b, d, pa, pb, first, sims, T, key, off, eps=0.0, temp_plies=0, game=None):
    """arena_puct written out in the public calls, without the early exit and for games that enter at any ply: per step the two
    puct_search on ALL rows, torch.where on the tree rows by the mover (ply + first) & 1, one puct_play; game m's row goes to record
    row game[m, 0], its noise row is that ply's.  A game that is over, or at ply >= T, is not played -> (records, boards, dice, game)"""
    M = b.shape[0]
    cb, cd = b.clone(), d.clone()
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda") if game is None else game.clone()
    rec = {k: torch.zeros((T, M) + s, dtype=dt, device="cuda") for k, (s, dt) in row_shapes(S).items()}
    stack = torch.stack([ea.selfplay_noise(M, 1.0, key, off, t) for t in range(T)]) if eps > 0 else None
    idx = torch.arange(M, device="cuda")
    for _ in range(T):
        ply = game[:, 0].clone()
        active = (game[:, 1] == 0) & (ply >= 0) & (ply < T)
        if not bool(active.any()):
            break
        noise = None if stack is None else stack[ply.clamp(0, T - 1).long(), idx].contiguous()
        ta = ea.puct_search(cb, cd, pa, sims, root_noise=noise, noise_eps=eps)
        tb = ea.puct_search(cb, cd, pb, sims, root_noise=noise, noise_eps=eps)
        mover_b = ((ply + first.to(torch.int32)) & 1).bool()
        tree = torch.where(mover_b[:, None], tb, ta).contiguous()
        g2 = game.clone()
        g2[~active, 1] = 1                                        # puct_play leaves a game that is over as it is
        row = ea.puct_play(tree, cb, cd, g2, S, sims, temp_plies=temp_plies, key=key, game_offset=off)
        game[active] = g2[active]
        for k in rec:
            rec[k][ply[active].long(), idx[active]] = row[k][active]
    return rec, cb, cd, game


def as_dict(ea, rec, game, first):
    """by_hand's records as arena_puct returns them"""
    out = dict(rec)
    out["live"] = out["live"].view(torch.bool)
    out["winner"], out["plies"] = game[:, 2].contiguous(), game[:, 0].contiguous()
    out["z"], out["weight"] = ea.selfplay_outcomes(out["winner"], out["live"])
    out["first"] = first.clone()
    out["result_a"] = out["winner"] * (1 - 2 * (first & 1).to(torch.int32))
    return out


# ---------------------------------------------------------------- 1. the definition

@pytest.mark.parametrize("S", [5, 7])
def test_the_definition(ea, S):
    pa, pb = nets(ea, S)
    b, d, first, want = reference(ea, S, 33)
    b0, d0, f0 = b.clone(), d.clone(), first.clone()
    h = check_rules(want, S, MAX_PLIES[S])                        # the yardstick is 33 whole games
    for tile, blocks in GEOMETRIES:
        got = ea.arena_puct_games(b, d, pa, pb, first, tile=tile, blocks=blocks, **KW)
        same_records(got, want)
    assert torch.equal(b, b0) and torch.equal(d, d0) and torch.equal(first, f0) and got["board"].data_ptr() != b.data_ptr()   # the inputs are not changed
    check_rules(got, S, MAX_PLIES[S])
    assert torch.equal(got["first"], first) and got["first"].data_ptr() != first.data_ptr() and got["result_a"].dtype == torch.int32
    assert torch.equal(got["result_a"], got["winner"] * (1 - 2 * first.to(torch.int32)))
    # the test bites: games of several lengths, both results, and other games than params_a's self-play
    assert h["plies"].min() < h["plies"].max()
    print("%dx%d: 33 games of %d .. %d plies, A wins %d, the first mover %d" % (
        S, S, h["plies"].min(), h["plies"].max(), int((got["result_a"] == 1).sum()), int((got["winner"] == 1).sum())))
    assert set(got["result_a"].tolist()) == {-1, 1} or set(got["winner"].tolist()) == {-1, 1}
    own = ea.selfplay_puct_games(b, d, pa, noise_eps=0.0, temp_plies=0, **KW)
    assert any(not torch.equal(own[k], got[k]) for k in ("board", "visits", "action"))
    same_records(ea.arena_puct(b, d, pa, pb, first, chunk=16, **KW), want)   # chunks of 16, 16 and 1
    if S == 5:                                                    # ... and the yardstick itself is the public calls composed
        rec, _, _, game = by_hand(ea, S, b, d, pa, pb, first, 8, MAX_PLIES[S], 11, 2 ** 32 + 5)
        same_records(want, as_dict(ea, rec, game, first))


# ---------------------------------------------------------------- 2. equal networks

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("eps,temp_plies", [(0.0, 0), (0.25, 8)])
def test_equal_networks_are_self_play(ea, S, eps, temp_plies):
    pa = nets(ea, S)[0]
    pb = pa.clone()
    b, d = reset_positions(ea, S, 33)
    kw = dict(KW, noise_eps=eps, temp_plies=temp_plies)
    want = ea.selfplay_puct_games(b, d, pa, **kw)
    mixed = (torch.arange(33, device="cuda") % 3 == 0)            # bool: read as int8
    for first, tile, blocks in ((torch.zeros(33, dtype=torch.int8, device="cuda"), None, None),
                                (torch.ones(33, dtype=torch.int8, device="cuda"), 4, 2), (mixed, 3, 2), (mixed, None, None)):
        got = ea.arena_puct_games(b, d, pa, pb, first, tile=tile, blocks=blocks, **kw)
        assert set(got) - set(want) == {"first", "result_a"}
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
    check_rules(want, S, MAX_PLIES[S])


# ---------------------------------------------------------------- 3. swapping sides

@pytest.mark.parametrize("S", [5, 7])
def test_swapping_sides(ea, S):
    pa, pb = nets(ea, S)
    b, d, first, want = reference(ea, S, 33)
    for tile, blocks in ((None, None), (3, 2)):
        got = ea.arena_puct_games(b, d, pb, pa, 1 - first, tile=tile, blocks=blocks, **KW)
        for k in want:
            if k not in ("first", "result_a"):
                assert torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
        assert torch.equal(got["result_a"], -want["result_a"]) and torch.equal(got["first"], 1 - first)
    assert bool((want["result_a"] != 0).all())


# ---------------------------------------------------------------- 4. phases

@pytest.mark.parametrize("S", [5, 7])
def test_phases_with_waiting_columns(ea, S):
    """70 games on two columns of one block, B moving first in all of them: the first phase must pick B, and every refill puts a game
    at an even ply beside one at any ply"""
    pa, pb = nets(ea, S)
    b, d, first, want = reference(ea, S, 70, first=1)
    assert bool((first == 1).all())
    same_records(ea.arena_puct_games(b, d, pa, pb, first, tile=2, blocks=1, **KW), want)
    same_records(ea.arena_puct_games(b, d, pa, pb, first, **KW), want)
    check_rules(want, S, MAX_PLIES[S])
    alt = ea.arena_puct(b, d, pa, pb, alternate(70), **KW)       # columns out of step from the start
    same_records(ea.arena_puct_games(b, d, pa, pb, alternate(70), tile=2, blocks=1, **KW), alt)
    assert not torch.equal(alt["action"], want["action"])


@pytest.mark.parametrize("S", [5, 7])
def test_one_game_and_how_first_is_read(ea, S):
    pa, pb = nets(ea, S)
    b, d = reset_positions(ea, S, 1)
    one = {}
    for f in (0, 1):
        first = torch.full((1,), f, dtype=torch.int8, device="cuda")
        one[f] = ea.arena_puct(b, d, pa, pb, first, **KW)
        for tile, blocks in ((None, None), (32, 1), (2, 1)):
            same_records(ea.arena_puct_games(b, d, pa, pb, first, tile=tile, blocks=blocks, **KW), one[f])
    assert not torch.equal(one[0]["action"], one[1]["action"])    # the other network's first move
    b, d, first, want = reference(ea, S, 33)
    zeros = torch.zeros(33, dtype=torch.int8, device="cuda")
    for play in (ea.arena_puct_games, ea.arena_puct):
        same_records(play(b, d, pa, pb, None, **KW), play(b, d, pa, pb, zeros, **KW))   # None is all zeros
        got = play(b, d, pa, pb, first + 2, **KW)                 # 2 and 3 read as 0 and 1: only bit 0
        assert torch.equal(got["first"], first + 2)
        for k in want:
            if k != "first":
                assert torch.equal(got[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
        same_records(play(b, d, pa, pb, first.to(torch.bool), **KW), want)


# ---------------------------------------------------------------- 5. cut games and entering plies

def abi_call(ea, S, b, d, pa, pb, first, sims, T, tile, blocks, key, off, temp_plies=0, eps=0.0, fill=None, game=None, alloc=None):
    """ewn_puct_arena through the C ABI on buffers of exactly the needed bytes -> (records dict, boards, dice, game).  fill: the byte
    the scratch and the record buffers hold before the call; alloc: a GuardedAllocator for every buffer the kernel sees"""
    from ewn_gym_amd.vec_env import _ptr, _stream
    lib, M = ea._lib.load(), b.shape[0]
    z = (lambda shape, dtype, tag: alloc.zeros(shape, dtype=dtype, tag=tag)) if alloc is not None else (
        lambda shape, dtype, tag: torch.zeros(shape, dtype=dtype, device="cuda"))
    rec = {k: z((T, M) + s, dt, "rec_" + k) for k, (s, dt) in row_shapes(S).items()}
    nscr = int(lib.ewn_puct_arena_scratch_bytes(S, 3, M, sims, tile, blocks))
    assert nscr == lib.ewn_puct_tree_bytes(S, 3, sims) * min(blocks, -(-M // tile)) * tile
    scratch = z((nscr,), torch.uint8, "scratch")
    cb, cd, cg = z((M, S, S), torch.int8, "boards"), z((M,), torch.int8, "dice"), z((M, 4), torch.int32, "game")
    ca, cbn, cf = z(pa.shape, torch.float32, "params"), z(pb.shape, torch.float32, "params_b"), z((M,), torch.int8, "first")
    for dst, src in ((cb, b), (cd, d), (ca, pa), (cbn, pb), (cf, first)):
        dst.copy_(src)
    if game is not None:
        cg.copy_(game)
    noise = None
    if eps > 0:
        noise = z((T, M, 6), torch.float32, "noise")
        noise.copy_(torch.stack([ea.selfplay_noise(M, 1.0, key, off, t) for t in range(T)]))
    if fill is not None:
        for t in list(rec.values()) + [scratch]:
            t.view(torch.uint8).fill_(fill)
    rc = lib.ewn_puct_arena(S, 3, M, sims, T, C.c_float(1.5), C.c_float(1.0), _ptr(ca), _ptr(cbn), _ptr(noise), C.c_float(eps), temp_plies,
                            C.c_uint64(key), C.c_int64(off), tile, blocks, _ptr(cb), _ptr(cd), _ptr(cg), _ptr(cf),
                            *[_ptr(rec[k]) for k in ROWS], _ptr(scratch), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(cf, first) and torch.equal(ca, pa) and torch.equal(cbn, pb)   # only read
    return rec, cb, cd, cg


@pytest.mark.parametrize("S", [5, 7])
def test_cut_games_and_entering_plies(ea, S):
    pa, pb = nets(ea, S)
    M, T, key, off = 33, 10, 21, 2 ** 33 + 1
    b, d = reset_positions(ea, S, M)
    first = alternate(M)
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    game[3::4, 0] = 1                                             # games 3, 7 .. enter at ply 1: first[m] = 1, so A moves
    game[2::8, 0] = 2                                             # games 2, 10 .. at ply 2: first[m] = 0, A moves
    game[4::8, 0] = 1                                             # games 4, 12 .. at ply 1: first[m] = 0, B moves
    game[5] = torch.tensor([4, 1, -1, 0])                         # over on entry: not played, left as it is
    game[6] = torch.tensor([T, 0, 0, 0])                          # at the last row's end: not played
    entering = game[:, 0].clone()
    played = (game[:, 1] == 0) & (entering < T)
    rec, cb, cd, cg = by_hand(ea, S, b, d, pa, pb, first, 8, T, key, off, eps=0.25, temp_plies=3, game=game)
    for tile, blocks in ((3, 2), (32, 1), (1, 5)):
        got, gb, gd, gg = abi_call(ea, S, b, d, pa, pb, first, 8, T, tile, blocks, key, off, temp_plies=3, eps=0.25, game=game)
        for k in ROWS:
            assert torch.equal(got[k].view(torch.uint8).reshape(-1), rec[k].contiguous().view(torch.uint8).reshape(-1)), (k, tile, blocks)
        assert torch.equal(gg, cg) and torch.equal(gb, cb) and torch.equal(gd, cd)
    # the rows below the entering ply, past the end, and of the games that are not played: zeros; the rows between: live
    live = got["live"].view(torch.bool)
    t = torch.arange(T, device="cuda")[:, None]
    inside = played[None, :] & (t >= entering[None, :]) & (t < gg[None, :, 0])
    assert torch.equal(live, inside)
    for k in ROWS:
        assert not bool(got[k].reshape(T, M, -1)[~inside].any()), k
    assert gg[5].tolist() == [4, 1, -1, 0] and gg[6].tolist() == [T, 0, 0, 0] and torch.equal(gb[5], b[5]) and torch.equal(gb[6], b[6])
    # the test bites: games cut at T (not over, no winner), games entered at plies 1 and 2, both movers at the entering ply
    cut = played & (gg[:, 1] == 0)
    assert bool(cut.any()) and bool((gg[cut, 0] == T).all()) and not bool(gg[cut, 2].any())
    late = played & (entering > 0)
    assert {0, 1, 2} <= set(entering[played].tolist()) and set(((entering + first) & 1)[late].tolist()) == {0, 1}
    # ... and from ply 0 the binding, cut at the same row, is the staged call
    want = ea.arena_puct(b, d, pa, pb, first, max_plies=T, temp_plies=3, noise_eps=0.25, sims=8, key=key, game_offset=off)
    same_records(ea.arena_puct_games(b, d, pa, pb, first, max_plies=T, temp_plies=3, noise_eps=0.25, sims=8, key=key, game_offset=off, tile=3,
                                     blocks=2), want)
    assert bool((want["result_a"] == 0).any()) and bool((want["plies"] == T).any())


# ---------------------------------------------------------------- 6. buffers

@pytest.mark.parametrize("S", [5, 7])
def test_what_the_buffers_held_does_not_matter_and_guard_zones(ea, S):
    pa, pb = nets(ea, S)
    M, T, key, off = 33, 24, 21, 2 ** 33
    b, d = reset_positions(ea, S, M)
    first = alternate(M)
    want = ea.arena_puct(b, d, pa, pb, first, sims=8, max_plies=T, noise_eps=0.25, temp_plies=4, key=key, game_offset=off)
    alloc = GuardedAllocator()
    for fill in (0xA5, 0x00):
        rec, cb, cd, cg = abi_call(ea, S, b, d, pa, pb, first, 8, T, 4, 2, key, off, temp_plies=4, eps=0.25, fill=fill, alloc=alloc)
        alloc.check("fill %#x" % fill)
        assert len(alloc.buffers) == 14                           # six record rows, the scratch, boards, dice, game, params, params_b, first, noise
        alloc.clear()
        for k in ROWS:
            assert torch.equal(rec[k].view(torch.uint8).reshape(-1), want[k].contiguous().view(torch.uint8).reshape(-1)), (fill, k)
        assert torch.equal(cg[:, 0], want["plies"]) and torch.equal(cg[:, 2], want["winner"])
    assert int(want["live"].sum()) > 33


# ---------------------------------------------------------------- 7. shards

@pytest.mark.parametrize("S", [5, 7])
def test_two_shards_are_the_whole(ea, S):
    pa, pb = nets(ea, S)
    b, d = reset_positions(ea, S, 70)
    first = alternate(70)
    kw = dict(KW, noise_eps=0.25, temp_plies=8)                  # the noise rows and the draws follow the global game
    off = kw["game_offset"]
    lo = ea.arena_puct_games(b[:34], d[:34], pa, pb, first[:34], **dict(kw, game_offset=off))
    hi = ea.arena_puct_games(b[34:], d[34:], pa, pb, first[34:], **dict(kw, game_offset=off + 34))
    whole = ea.arena_puct_games(b, d, pa, pb, first, **kw)
    for k in whole:
        dim = 0 if whole[k].dim() == 1 else 1                      # winner, plies, first, result_a [M]; every other [T, M, ...]
        assert torch.equal(torch.cat([lo[k], hi[k]], dim), whole[k]), k
    assert not torch.equal(whole["action"], ea.arena_puct_games(b, d, pa, pb, first, **KW)["action"])   # the noise and the draws are read


# ---------------------------------------------------------------- 8. the tournament and the command line

def test_the_tournament_entry(ea):
    from ewn_gym_amd import tournament
    ma, mb = pool(ea, 5)["model"], make_model(5, 9)
    r = tournament.arena(ma, mb, num=64, sims=8)
    s = tournament.arena(ma, mb, num=64, sims=8, whole_games=False)
    assert (r["engine"], s["engine"]) == ("ewn_puct_arena", "ewn_puct_search")
    for k in r:
        if k != "engine":
            assert r[k] == s[k], k
    assert r["wins_a"] + r["wins_b"] + r["undecided"] == r["episodes"] == 64 and r["undecided"] == 0
    assert r["a_first"]["episodes"] == r["b_first"]["episodes"] == 32 and r["a_first"]["wins_a"] + r["b_first"]["wins_a"] == r["wins_a"]
    assert r["win_rate"] == r["wins_a"] / 64 and r["ci95"][0] <= r["win_rate"] <= r["ci95"][1] and 6 <= r["avg_length"] <= 69
    # seed_offset moves the start positions and the global games together: the second half of the 64 games is the call on seeds 16 ..
    tail = tournament.arena(ma, mb, num=32, sims=8, seed_offset=16)
    head = tournament.arena(ma, mb, num=32, sims=8)
    assert tail["episodes"] == 32 and head["wins_a"] + tail["wins_a"] == r["wins_a"] and head["wins_b"] + tail["wins_b"] == r["wins_b"]


def test_the_command_line_end_to_end(ea, tmp_path):
    """the row of --arena on two saved checkpoints, in a fresh child process: the command line is what this test is about"""
    import json
    import os
    import subprocess
    import sys
    pa, pb = nets(ea, 5)
    a, b = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    torch.save({"params": pa.cpu()}, a)
    torch.save({"params": pb.cpu()}, b)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.tournament", "--model", a, "--opponent_model", b, "--arena", "8", "--num", "64"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("arena(8): model vs opponent_model") and "ewn_puct_arena" in lines[0]
    t = json.loads(lines[-1])
    row = t["arena(8): model vs opponent_model"]
    assert row["wins_a"] + row["wins_b"] + row["undecided"] == row["episodes"] == 64 and row["engine"] == "ewn_puct_arena"
    from ewn_gym_amd import tournament
    want = tournament.arena(pool(ea, 5)["model"], make_model(5, 9), num=64, sims=8)
    assert (row["wins_a"], row["wins_b"], row["a_first"], row["b_first"]) == (want["wins_a"], want["wins_b"], want["a_first"], want["b_first"])
