"""Whole self-play games of the PUCT search in one launch (ewn_puct_selfplay): selfplay_puct's records from one kernel
that owns its columns for whole games and hands a column the next game the moment its game ends.

Host side is plumbing only, as in search.py, whose checks and error texts these are: torch owns the buffers and the stream,
libewn_hip.so does the work.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _positive, _ptr, _same_gpu, _stream
from .endgame import _accept_table
from .search import (_PLAY_ROWS, SELFPLAY_MAX_PLIES, _game_column, _network_inputs, _noise_eps, _play_numbers, _puct_numbers, selfplay_noise,
                     selfplay_outcomes)

PUCT_GAMES_TILE = 32           # the most columns a block of ewn_puct_selfplay has (csrc/ewn_puct_games.hip) ...
PUCT_GAMES_MAX_BLOCKS = 256    # ... and the most blocks


def _geometry(who, name, x, most):
    if x is None:
        return 0                                               # the library's choice
    if not (isinstance(x, (int, np.integer)) and 1 <= int(x) <= most):
        raise ValueError("%s: %s must be None or an integer in 1..%d, got %r" % (who, name, most, x))
    return int(x)


def selfplay_puct_games(boards, dice, params, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.25, noise_alpha=1.0,
                        temp_plies=8, key=0, game_offset=0, cube_layer=3, tile=None, blocks=None):
    """selfplay_puct's M games and its records, byte for byte, from ONE launch (ewn_puct_selfplay): a block of the
    kernel has `tile` columns, owns a fixed share of the games and plays each to its end -- per ply the search of puct_search, then
    the move of puct_play -- and a column whose game has ended takes the block's next game, so no tree-round is spent on a finished
    game.  boards [S, S] or [M, S, S], dice [M], params as predict_policy takes them; they are not changed.  The arguments are
    selfplay_puct's, with its checks and error texts; there is no chunk, no check_every (no host read) and no endgame_table (the
    exact-leaf substitution is the staged path's).  tile (1..32) and blocks (1..256): None is the library's choice (DESIGN.md 4s has
    the measurements); they change no byte of the result, and never more than ceil(M / tile) blocks run.
    The noise is selfplay_noise for plies 0 .. max_plies - 1, drawn up front and stacked to [T, M, 6] (24 M bytes per ply; none when
    noise_eps == 0): the rows selfplay_puct draws ply by ply, so the calls on the shards of M games (game_offset moved to each shard's
    first game) give the rows of the one call on all of them.  game, the records and the scratch (blocks x tile trees) are allocated
    once.  Returns selfplay_puct's dict: board int8 [T, M, S, S], dice int8 [T, M], visits int32 [T, M, 2, 3], value float32 [T, M],
    action int8 [T, M, 2], live bool [T, M], z and weight float32 [T, M], winner int32 [M], plies int32 [M]."""
    who = "selfplay_puct_games"
    lib = _lib.load()
    a = _games_arguments(who, boards, dice, params, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha, temp_plies, key,
                         game_offset, cube_layer, tile, blocks)
    return _play_games(lib, a, params, lambda *front: check(lib.ewn_puct_selfplay(*front, _stream()), "ewn_puct_selfplay"))


def _games_arguments(who, boards, dice, params, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha, temp_plies, key, game_offset,
                     cube_layer, tile, blocks, table=None, table_name="endgame_table", table_required=False, more=(), optional=()):
    """The checks of a call that plays whole games in one launch, in selfplay_puct's order and texts: the numbers, then the tensors
    (table: an EndgameTable for the boards' size, the caller's keyword table_name; None: no table, unless table_required; more and
    optional: a further entry's inputs, as _network_inputs takes them), max_plies, the devices -> a dict of the checked values, as
    _play_games takes it"""
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = _noise_eps(who, noise_eps)
    temp_plies, key, game_offset = _play_numbers(who, temp_plies, key, game_offset)
    _positive(who, "noise_alpha", noise_alpha)
    tile, blocks = _geometry(who, "tile", tile, PUCT_GAMES_TILE), _geometry(who, "blocks", blocks, PUCT_GAMES_MAX_BLOCKS)
    if table_required and table is None:                       # _network_inputs takes None for "no table"
        _accept_table(who, table, None, None, name=table_name)
    M, S, L, dev, inputs = _network_inputs(who, boards, dice, params, cube_layer, more, optional, table=table, table_name=table_name)
    T = SELFPLAY_MAX_PLIES[S] if max_plies is None else max_plies
    if not (isinstance(T, (int, np.integer)) and int(T) >= 1):
        raise ValueError("%s: max_plies must be a positive integer or None, got %r" % (who, max_plies))
    _same_gpu(who, dev, "params", inputs.items())
    return dict(sims=sims, eps=eps, temp_plies=temp_plies, key=key, game_offset=game_offset, noise_alpha=noise_alpha, tile=tile, blocks=blocks,
                M=M, S=S, L=L, dev=dev, inputs=inputs, T=int(T), c_puct=float(c_puct), terminal_value=float(terminal_value))


def _play_games(lib, a, params, launch):
    """The buffers of a call that plays whole games in one launch, the launch and the records.  a: _games_arguments' dict;
    launch(*front): the entry's call and its check, front = ewn_puct_selfplay's arguments up to the scratch -- what a further entry
    takes goes behind them.  Nothing is launched for M == 0 -> selfplay_puct's dict"""
    M, S, L, T, dev, sims = a["M"], a["S"], a["L"], a["T"], a["dev"], a["sims"]
    b, d = a["inputs"]["boards"].clone(), a["inputs"]["dice"].clone()    # played on in place
    rec = {name: torch.empty((T, M) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}   # every row is written
    game = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    if M > 0:
        noise = (torch.stack([selfplay_noise(M, a["noise_alpha"], a["key"], a["game_offset"], t, dev) for t in range(T)])
                 if a["eps"] > 0.0 else None)
        scratch = torch.empty(int(check(lib.ewn_puct_selfplay_scratch_bytes(S, L, M, sims, a["tile"], a["blocks"]),
                                        "ewn_puct_selfplay_scratch_bytes")), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            launch(S, L, M, sims, T, C.c_float(a["c_puct"]), C.c_float(a["terminal_value"]), _ptr(params), _ptr(noise), C.c_float(a["eps"]),
                   a["temp_plies"], C.c_uint64(a["key"]), C.c_int64(a["game_offset"]), a["tile"], a["blocks"], _ptr(b), _ptr(d), _ptr(game),
                   *[_ptr(rec[name]) for name, _, _ in _PLAY_ROWS], _ptr(scratch))
    rec["live"] = rec["live"].view(torch.bool)
    rec["winner"], rec["plies"] = _game_column(game, 2), _game_column(game, 0)
    rec["z"], rec["weight"] = selfplay_outcomes(rec["winner"], rec["live"])
    return rec
