"""Whole self-play games in one launch (ewn_puct_selfplay, selfplay_puct_games, whole_games=True) against selfplay_puct,
the staged ply-by-ply path.  The tree code, the move (csrc/ewn_puct.hpp), the network code and the compiler flags are the same on
both paths, so there is no tolerance anywhere in this file: every comparison is of all bytes of all records, and any difference is a
bug.  How many columns a block has and how many blocks share the games changes no byte either: every comparison runs under the
library's choice and under geometries that force refills (more games than columns), uneven sets and two columns on one wave.
1. the records are selfplay_puct's.  2. without noise.  3. cut games.  4. planted rows.  5. sims 0 and 40.  6. buffers.  7. shards.
8. the trainer and the command line."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct_fused import planted  # noqa: E402
from tests.test_gpu_puct_selfplay import ROWS, by_hand, check_rules, reset_positions, row_shapes, same_records, selfplay_trainer  # noqa: E402

GEOMETRIES = ((None, None), (32, 1), (2, 1), (3, 2), (1, 5))   # (tile, blocks); None: the library's choice
MAX_PLIES = {5: 80, 7: 128}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_REF = {}


def reference(ea, S, M):
    """computed once per shape and left unchanged: M reset positions, selfplay_puct's records of them (the staged path) and the
    arguments they were played with"""
    if (S, M) not in _REF:
        b, d = reset_positions(ea, S, M)
        kw = dict(sims=8, key=11, game_offset=2 ** 32 + 5)
        _REF[(S, M)] = (b, d, kw, ea.selfplay_puct(b, d, pool(ea, S)["params"], **kw))
    return _REF[(S, M)]


# ---------------------------------------------------------------- 1. the records are selfplay_puct's

@pytest.mark.parametrize("S", [5, 7])
def test_the_records_are_the_staged_path_s(ea, S):
    params = pool(ea, S)["params"]
    b, d, kw, want = reference(ea, S, 33)
    b0, d0 = b.clone(), d.clone()
    h = check_rules(want, S, MAX_PLIES[S])                        # the yardstick is 33 whole games
    for tile, blocks in GEOMETRIES:
        got = ea.selfplay_puct_games(b, d, params, tile=tile, blocks=blocks, **kw)
        same_records(got, want)
    assert torch.equal(b, b0) and torch.equal(d, d0) and got["board"].data_ptr() != b.data_ptr()   # the inputs are not changed
    check_rules(got, S, MAX_PLIES[S])
    assert h["plies"].min() < h["plies"].max()                    # games of several lengths: columns fall free at different plies
    if S == 5:                                                    # ... and the yardstick itself is the public calls composed
        same_records(want, by_hand(ea, S, b, d, params, 8, MAX_PLIES[S], 11, 2 ** 32 + 5))


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 70])
def test_one_game_and_seventy(ea, S, M):
    params = pool(ea, S)["params"]
    b, d, kw, want = reference(ea, S, M)
    for tile, blocks in ((None, None), (8, 2)):
        same_records(ea.selfplay_puct_games(b, d, params, tile=tile, blocks=blocks, **kw), want)
    assert int(want["plies"].min()) >= 1 and bool((want["winner"] != 0).all())


# ---------------------------------------------------------------- 2. without noise

@pytest.mark.parametrize("S", [5, 7])
def test_without_noise_other_keys_and_again(ea, S):
    params = pool(ea, S)["params"]
    b, d, kw, noisy = reference(ea, S, 33)
    want = ea.selfplay_puct(b, d, params, noise_eps=0.0, **kw)
    got = ea.selfplay_puct_games(b, d, params, noise_eps=0.0, **kw)
    same_records(got, want)
    same_records(ea.selfplay_puct_games(b, d, params, noise_eps=0.0, tile=3, blocks=2, **kw), want)
    assert not torch.equal(want["visits"], noisy["visits"])       # the noise instance is another search
    other = ea.selfplay_puct_games(b, d, params, **dict(kw, key=12))
    assert not torch.equal(other["action"], noisy["action"])
    check_rules(other, S, MAX_PLIES[S])
    same_records(ea.selfplay_puct_games(b, d, params, **dict(kw, key=12)), other)   # the same arguments: the same bytes


# ---------------------------------------------------------------- 3. cut games

def abi_call(ea, S, b, d, params, sims, T, tile, blocks, key, off, temp_plies=8, eps=0.25, fill=None, game=None, skip=None, alloc=None):
    """ewn_puct_selfplay through the C ABI on buffers of exactly the needed bytes -> (records dict without `skip`, boards, dice, game).
    fill: the byte the scratch and the record buffers hold before the call; alloc: a GuardedAllocator for every buffer the kernel sees"""
    from ewn_gym_amd.vec_env import _ptr, _stream
    lib, M = ea._lib.load(), b.shape[0]
    z = (lambda shape, dtype, tag: alloc.zeros(shape, dtype=dtype, tag=tag)) if alloc is not None else (
        lambda shape, dtype, tag: torch.zeros(shape, dtype=dtype, device="cuda"))
    rec = {k: z((T, M) + s, dt, "rec_" + k) for k, (s, dt) in row_shapes(S).items() if k != skip}
    nscr = int(lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, tile, blocks))
    assert nscr == lib.ewn_puct_tree_bytes(S, 3, sims) * min(blocks, -(-M // tile)) * tile
    scratch = z((nscr,), torch.uint8, "scratch")
    cb, cd, cg, cp = z((M, S, S), torch.int8, "boards"), z((M,), torch.int8, "dice"), z((M, 4), torch.int32, "game"), z(params.shape, torch.float32, "params")
    cb.copy_(b)
    cd.copy_(d)
    cp.copy_(params)
    if game is not None:
        cg.copy_(game)
    noise = None
    if eps > 0:
        noise = z((T, M, 6), torch.float32, "noise")
        noise.copy_(torch.stack([ea.selfplay_noise(M, 1.0, key, off, t) for t in range(T)]))
    if fill is not None:
        for t in list(rec.values()) + [scratch]:
            t.view(torch.uint8).fill_(fill)
    rc = lib.ewn_puct_selfplay(S, 3, M, sims, T, C.c_float(1.5), C.c_float(1.0), _ptr(cp), _ptr(noise), C.c_float(eps), temp_plies,
                               C.c_uint64(key), C.c_int64(off), tile, blocks, _ptr(cb), _ptr(cd), _ptr(cg),
                               *[_ptr(rec.get(k)) for k in ROWS], _ptr(scratch), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return rec, cb, cd, cg


@pytest.mark.parametrize("S", [5, 7])
def test_cut_games(ea, S):
    p = pool(ea, S)
    b, d = p["boards"][:33], p["dice"][:33]
    kw = dict(sims=8, max_plies=12, temp_plies=4, key=11, game_offset=5)
    want = ea.selfplay_puct(b, d, p["params"], **kw)
    for tile, blocks in GEOMETRIES:
        got = ea.selfplay_puct_games(b, d, p["params"], tile=tile, blocks=blocks, **kw)
        same_records(got, want)
    cut = got["live"][11] & (got["winner"] == 0)                  # played at row 11 and not won there
    assert bool(cut.any()) and bool((got["winner"] != 0).any()) and int(got["live"].sum()) > 33
    assert bool((got["plies"][cut] == 12).all()) and bool(got["live"][:, cut].all()) and not bool(got["weight"][:, cut].any())
    assert not bool(got["z"][:, cut].any())
    rec, _, _, game = abi_call(ea, S, b, d, p["params"], 8, 12, 3, 2, 11, 5, temp_plies=4)
    assert game[cut].tolist() == [[12, 0, 0, 0]] * int(cut.sum())  # over == 0, winner == 0
    assert bool((game[~cut, 1] == 1).all()) and torch.equal(game[:, 2], want["winner"]) and torch.equal(game[:, 0], want["plies"])
    for k in ROWS:
        assert torch.equal(rec[k].view(torch.uint8).reshape(-1), want[k].contiguous().view(torch.uint8).reshape(-1)), k


# ---------------------------------------------------------------- 4. planted rows

@pytest.mark.parametrize("S", [5, 7])
def test_planted_rows(ea, S):
    p = pool(ea, S)
    b, d = p["boards"][400:433].clone(), p["dice"][400:433].clone()
    pb, pd, dead = planted(S)
    b[1:29:2], d[1:29:2] = pb, pd                                  # rows 1, 3 .. 27: a plain row between any two of them
    kw = dict(sims=8, key=4, game_offset=77)
    want = ea.selfplay_puct(b, d, p["params"], **kw)
    for tile, blocks in ((4, 1), (None, None)):
        same_records(ea.selfplay_puct_games(b, d, p["params"], tile=tile, blocks=blocks, **kw), want)
    at = 1 + 2 * torch.nonzero(torch.tensor(dead)).reshape(-1).cuda()
    assert not bool(want["live"][:, at].any()) and not bool(want["plies"][at].any()) and not bool(want["winner"][at].any())
    assert int(want["live"].sum()) > 33                           # ... among games that are played


# ---------------------------------------------------------------- 5. sims 0 and 40

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("sims", [0, 40])
def test_no_simulations_and_forty(ea, S, sims):
    params = pool(ea, S)["params"]
    b, d, _, _ = reference(ea, S, 33)
    kw = dict(sims=sims, key=3, game_offset=9, max_plies=40 if sims == 40 else None)
    want = ea.selfplay_puct(b, d, params, **kw)
    same_records(ea.selfplay_puct_games(b, d, params, tile=4, blocks=2, **kw), want)
    live = want["live"]
    assert int(want["visits"].sum()) == sims * int(live.sum())   # every recorded root was searched with the whole budget
    assert int(live.sum()) > 33


# ---------------------------------------------------------------- 6. buffers

@pytest.mark.parametrize("S", [5, 7])
def test_what_the_buffers_held_does_not_matter_and_guard_zones(ea, S):
    p = pool(ea, S)
    M, T, sims, key, off = 33, 24, 8, 21, 2 ** 33
    b, d = reset_positions(ea, S, M)
    want = ea.selfplay_puct(b, d, p["params"], sims=sims, max_plies=T, key=key, game_offset=off)
    # games the kernel must not play: over on entry (with a winner and a ply), and at or past the last row; word 3 is nobody's
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    game[4] = torch.tensor([3, 1, -1, 7])
    game[5] = torch.tensor([0, 1, 0, 0])
    game[9] = torch.tensor([T, 0, 0, 0])
    game[10] = torch.tensor([T + 5, 0, 0, -1])
    game[32] = torch.tensor([-1, 0, 0, 0])
    game[11, 3] = 0x5A5A
    idle = torch.tensor([4, 5, 9, 10, 32], device="cuda")
    played = torch.ones(M, dtype=torch.bool, device="cuda")
    played[idle] = False
    alloc = GuardedAllocator()
    full = None
    for fill, skips in ((0xFF, ROWS + (None,)), (0x7F, (None,))):
        for skip in skips:
            rec, cb, cd, cg = abi_call(ea, S, b, d, p["params"], sims, T, 4, 2, key, off, fill=fill, game=game, skip=skip, alloc=alloc)
            alloc.check("fill %#x, without %s" % (fill, skip))
            alloc.clear()
            for k in ROWS:
                if k == skip:
                    continue
                got, ref = rec[k].view(torch.uint8).reshape(T, M, -1), want[k].contiguous().view(torch.uint8).reshape(T, M, -1)
                assert torch.equal(got[:, played], ref[:, played]), (fill, skip, k)
                assert not bool(got[:, idle].any()), (fill, skip, k)           # every row of a game that is not played: zeros
            assert torch.equal(cg[idle], game[idle]) and torch.equal(cb[idle], b[idle]) and torch.equal(cd[idle], d[idle])
            assert torch.equal(cg[played, 0], want["plies"][played]) and torch.equal(cg[played, 2], want["winner"][played])
            assert int(cg[11, 3]) == 0x5A5A
            if full is None:
                full = (cb, cd, cg)
            else:
                assert all(torch.equal(x, y) for x, y in zip(full, (cb, cd, cg))), (fill, skip)
    assert int(want["live"][:, played].sum()) > 33 and bool((want["plies"] < T).any())


# ---------------------------------------------------------------- 7. shards

@pytest.mark.parametrize("S", [5, 7])
def test_two_shards_are_the_whole(ea, S):
    params = pool(ea, S)["params"]
    b, d, kw, want = reference(ea, S, 70)
    off = kw["game_offset"]
    lo = ea.selfplay_puct_games(b[:33], d[:33], params, **dict(kw, game_offset=off))
    hi = ea.selfplay_puct_games(b[33:], d[33:], params, **dict(kw, game_offset=off + 33))
    whole = ea.selfplay_puct_games(b, d, params, **kw)
    same_records(whole, want)
    for k in whole:
        dim = 0 if whole[k].dim() == 1 else 1                      # winner, plies [M]; every other [T, M, ...]
        assert torch.equal(torch.cat([lo[k], hi[k]], dim), whole[k]), k


# ---------------------------------------------------------------- 8. the trainer and the command line

def test_the_trainer_takes_whole_games(ea, tmp_path):
    tr, ref = selfplay_trainer(ea, whole_games=True), selfplay_trainer(ea, fused=True)
    assert tr.whole_games is True and ref.whole_games is False and selfplay_trainer(ea).whole_games is False
    tr.collect_and_update()
    ref.collect_and_update()
    same_records(tr.records, ref.records)
    assert torch.equal(bits(tr.grad), bits(ref.grad)) and torch.equal(bits(tr.params), bits(ref.params))
    assert bool((tr.records["winner"] == 0).any()) and bool((tr.records["winner"] != 0).any())    # 16 plies: cut and finished games
    path = str(tmp_path / "selfplay.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["whole_games"] is True and sd["fused_search"] is False and sd["algorithm"] == "SELFPLAY"
    other = selfplay_trainer(ea)
    other.load(path)
    assert other.whole_games is True and other.fused is False
    ref.save(path)
    other.load(path)
    assert other.whole_games is False and other.fused is True
    tr.collect_and_update()                                       # the second update plays other games, on both paths the same
    ref.collect_and_update()
    same_records(tr.records, ref.records)
    assert torch.equal(bits(tr.params), bits(ref.params))


def test_train_a2c_selfplay_whole_games_end_to_end(ea, tmp_path):
    """two epochs of one update each with tiny numbers, in a fresh child process: the command line is what this test is about"""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SELFPLAY", "--whole_games", "--num_envs", "64", "--sims", "4",
                        "--epoch_num", "2", "--timesteps_per_epoch", "300", "--eval_episode_num", "16", "--eval_opponent", "random",
                        "--save_dir", str(tmp_path)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert any(x.get("trainer") == "PuctSelfPlayTrainer" for x in lines)
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 2 and all(math.isfinite(x["policy_loss"]) and 6 <= x["mean_game_length"] <= 69 and x["finished_fraction"] == 1.0 for x in ep)
    assert 300 <= ep[0]["timesteps"] < ep[1]["timesteps"] <= 2 * 64 * 69
    sd = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["sims"], sd["whole_games"], sd["fused_search"]) == ("SELFPLAY", 4, True, False) and sd["seed_counter"] in (1, 2)
