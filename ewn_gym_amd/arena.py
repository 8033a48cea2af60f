"""The arena: the PUCT searches of two networks play whole games against each other.  arena_puct is the definition, in
stages: per ply one ewn_puct_search with the mover's parameters and one ewn_puct_play.  arena_puct_games is the same games and records,
byte for byte, from ONE launch (ewn_puct_arena), a kernel that owns its columns for whole games as ewn_puct_selfplay does and holds
one network's weights at a time.

Host side is plumbing only, as in games.py, whose checks, buffers and records these are: torch owns the buffers and the stream,
libewn_hip.so does the work.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from ._args import _at_least_one, _ptr, _stream
from .games import _games_arguments, _play_games
from .search import _PLAY_ROWS, _game_column, _puct_search, _search_setup, selfplay_noise, selfplay_outcomes

ARENA_CHECK_EVERY = 8          # arena_puct: one host read every so many plies ends a chunk whose games are all over (selfplay_puct's default)


def _arena_arguments(who, boards, dice, params_a, params_b, first, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha, temp_plies,
                     key, game_offset, cube_layer, tile=None, blocks=None):
    """_games_arguments with the arena's two further inputs, checked with the others and before the devices: params_b exactly as
    params_a, first int8 or bool [M] or None -> its dict; a["inputs"]["first"] is the int8 tensor or None"""
    if isinstance(first, torch.Tensor) and first.dtype == torch.bool:
        first = first.view(torch.int8)                         # read in place: one byte per game, 0 or 1
    return _games_arguments(who, boards, dice, params_a, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha, temp_plies, key,
                            game_offset, cube_layer, tile, blocks, more=(("params_b", params_b, torch.float32, lambda M, P: (P,)),),
                            optional=(("first", first, torch.int8, lambda M, P: (M,)),))


def _arena_result(rec, first, M, dev):
    """the two entries an arena adds to selfplay_puct's dict: first int8 [M] as read (None: zeros), result_a int32 [M]"""
    rec["first"] = torch.zeros(M, dtype=torch.int8, device=dev) if first is None else first.clone()
    rec["result_a"] = rec["winner"] * (1 - 2 * (rec["first"] & 1).to(torch.int32))
    return rec


def arena_puct(boards, dice, params_a, params_b, first=None, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.0,
               noise_alpha=1.0, temp_plies=0, key=0, game_offset=0, chunk=1024, cube_layer=3):
    """M games between the PUCT searches of two networks, from the given positions to the end: selfplay_puct with the
    network that searches a ply chosen by the ply's mover.  first int8 or bool [M] (None: zeros) names the network that moves at the
    even plies of game m, 0 for A (params_a) and 1 for B (params_b); ply t of game m is searched by A when (t + first[m]) is even and
    by B otherwise; only bit 0 of first[m] is read.  Written out in the public calls, per ply t of a chunk: that ply's selfplay_noise
    rows when noise_eps > 0, puct_search(cb, cd, params_a, ...) and puct_search(cb, cd, params_b, ...), each game's tree taken from
    the call of its mover's network, one puct_play on those trees into record row t.  Here each network searches only the games it
    moves in: observations are independent, so no byte changes.  boards, dice, max_plies, key, game_offset, the checks and the error
    texts are selfplay_puct's, params_b is checked as params_a is; `chunk` games are played at a time, each chunk to its end, and
    every 8 plies one host read ends a chunk whose games are all over.  The defaults are an arena's: no root noise and the most
    visited move (noise_eps=0, temp_plies=0); both remain arguments.
    Returns selfplay_puct's dict and two entries more: first int8 [M] as read, result_a int32 [M] = winner * (1 - 2 * first): +1 A
    won, -1 B won, 0 the game was cut at max_plies.  (winner, z and weight keep selfplay_puct's meaning: the side that moves at even
    plies.)"""
    who = "arena_puct"
    lib = _lib.load()
    _at_least_one(who, "chunk", chunk)
    a = _arena_arguments(who, boards, dice, params_a, params_b, first, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha,
                         temp_plies, key, game_offset, cube_layer)
    M, S, L, T, dev, sims, eps = a["M"], a["S"], a["L"], a["T"], a["dev"], a["sims"], a["eps"]
    b, d, first = a["inputs"]["boards"], a["inputs"]["dice"], a["inputs"]["first"]
    params = (params_a, a["inputs"]["params_b"])
    rec = {name: torch.zeros((T, M) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}
    game = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    odd = torch.zeros(M, dtype=torch.bool) if first is None else (first & 1).to(torch.bool).cpu()   # one host read per call
    c, full, cp, tv = _search_setup(lib, S, L, M, sims, chunk, c_puct, terminal_value, dev, True)
    # per chunk, its games by the network that moves at their even plies: at ply t network (t + s) & 1 searches the games of side s
    sides = [[torch.nonzero(odd[i:i + c] == bool(s)).reshape(-1) for s in (0, 1)] for i in range(0, M, c)]
    # the trees of a side that is not the whole chunk are searched apart: as many rows as the largest such side has
    most = max([r.numel() for two in sides for r in two if r.numel() < two[0].numel() + two[1].numel()], default=0)
    part = (torch.empty((most, full[0].shape[1]), dtype=torch.uint8, device=dev), None, None, None, None, None)
    with torch.cuda.device(dev):
        st = _stream()
        drawn = []
        for i in range(0, M, c):
            n = min(c, M - i)
            cb, cd, cg = b[i:i + n].clone(), d[i:i + n].clone(), game[i:i + n]
            side = [r.to(dev) for r in sides[i // c]]
            for t in range(T):
                noise = None
                if eps > 0.0:
                    if t == len(drawn):                        # a ply's noise is drawn once, for all M games: later chunks read their rows
                        drawn.append(selfplay_noise(M, a["noise_alpha"], a["key"], a["game_offset"], t, dev))
                    noise = drawn[t][i:i + n]
                for s in (0, 1):
                    rows, net = side[s], params[(t + s) & 1]
                    if rows.numel() == n:                      # every game of the chunk: searched where it stands, into the trees the move reads
                        _puct_search(lib, S, L, n, sims, cb, cd, net, cp, tv, None, full, st, noise, eps, fused=True)
                    elif rows.numel() > 0:                     # its rows alone, and their trees back to the rows' places
                        k = rows.numel()
                        _puct_search(lib, S, L, k, sims, cb[rows], cd[rows], net, cp, tv, None, part, st,
                                     None if noise is None else noise[rows], eps, fused=True)
                        full[0][rows] = part[0][:k]
                check(lib.ewn_puct_play(S, L, n, _ptr(full[0]), _ptr(cb), _ptr(cd), _ptr(cg), a["temp_plies"], C.c_uint64(a["key"]),
                                        C.c_int64(a["game_offset"] + i), *[_ptr(rec[name][t, i:i + n]) for name, _, _ in _PLAY_ROWS], st),
                      "ewn_puct_play")
                if (t + 1) % ARENA_CHECK_EVERY == 0 and bool(cg[:, 1].all()):
                    break
    rec["live"] = rec["live"].view(torch.bool)
    rec["winner"], rec["plies"] = _game_column(game, 2), _game_column(game, 0)
    rec["z"], rec["weight"] = selfplay_outcomes(rec["winner"], rec["live"])
    return _arena_result(rec, first, M, dev)


def arena_puct_games(boards, dice, params_a, params_b, first=None, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.0,
                     noise_alpha=1.0, temp_plies=0, key=0, game_offset=0, cube_layer=3, tile=None, blocks=None):
    """arena_puct's M games and its dict, byte for byte, from ONE launch (ewn_puct_arena): selfplay_puct_games' kernel
    with a network per phase.  A block holds the two weight images of one network at a time; in every phase it plays one ply of the
    columns that wait for the network with more waiting columns, and repacks the images when that network changes.  The arguments,
    the checks and the error texts are arena_puct's, without a chunk; the up-front selfplay_noise stack, tile and blocks are
    selfplay_puct_games': tile (1..32) and blocks (1..256) change no byte of the result."""
    who = "arena_puct_games"
    lib = _lib.load()
    a = _arena_arguments(who, boards, dice, params_a, params_b, first, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha,
                         temp_plies, key, game_offset, cube_layer, tile, blocks)
    pb, first = _ptr(a["inputs"]["params_b"]), a["inputs"]["first"]
    # front: ewn_puct_selfplay's arguments up to the scratch; params_b goes behind params (index 7), first behind game (index 17)
    rec = _play_games(lib, a, params_a, lambda *front: check(lib.ewn_puct_arena(*front[:8], pb, *front[8:18], _ptr(first), *front[18:], _stream()),
                                                             "ewn_puct_arena"))
    return _arena_result(rec, first, a["M"], a["dev"])
