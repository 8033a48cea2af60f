"""Whole self-play games of the PUCT search in one launch with exact endgame values at the leaves a table covers (ewn_puct_selfplay_eg,
DESIGN.md 4x): selfplay_puct(leaf_table=)'s records from the kernel of selfplay_puct_games, which owns its columns for whole games.

Host side is plumbing only: games.py's checks, buffers and records through its own helpers, the table through endgame.py's.
"""
import torch

from . import _lib
from ._lib import check
from ._args import _ptr, _stream
from .games import _games_arguments, _play_games


def _games_table_alone(who, games_table, endgame_table=None, leaf_table=None, leaves=1):
    """the users' keyword: games_table is the one launch of ewn_puct_selfplay_eg, which is neither the staged path's
    substitution, nor the one launch per ply, nor the wide launch -> whether there is one"""
    if games_table is None:
        return False
    if endgame_table is not None:
        raise ValueError("%s: games_table does not go with endgame_table: both put exact values at the covered leaves, games_table in one "
                         "launch for whole games (ewn_puct_selfplay_eg), endgame_table on the staged path" % who)
    if leaf_table is not None:
        raise ValueError("%s: games_table does not go with leaf_table: both read one table at the covered leaves, games_table in one launch "
                         "for whole games (ewn_puct_selfplay_eg), leaf_table in one launch per ply (ewn_puct_search_eg)" % who)
    if leaves != 1:
        raise ValueError("%s: games_table does not go with leaves=%r: ewn_puct_selfplay_eg evaluates one leaf per tree and round (leaves=1)" % (
            who, leaves))
    return True


def selfplay_puct_games_exact(boards, dice, params, leaf_table, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.25,
                              noise_alpha=1.0, temp_plies=8, key=0, game_offset=0, cube_layer=3, tile=None, blocks=None,
                              return_leaf_counts=False):
    """selfplay_puct(boards, dice, params, leaf_table=leaf_table, ...)'s M games and its records, in every byte of every key, from ONE
    launch (ewn_puct_selfplay_eg): selfplay_puct_games with a ply's search that of puct_search_exact -- a pending leaf
    that the table covers is worth float32(terminal_value * q) at the action EndgameTable.lookup returns, every other leaf the value
    head's output.  leaf_table: an EndgameTable for the boards' size on the boards' GPU, complete before this call in stream order.
    The other arguments, the checks and the error texts, the up-front selfplay_noise stack, tile and blocks are selfplay_puct_games'.
    Returns selfplay_puct's dict; return_leaf_counts adds "leaf_counts" int32 [M, 2]: per game the sums of puct_search_exact's
    leaf_counts over the plies played -- the rounds whose pending leaf the table valued, and those the value head valued; zeros for a
    game that is not played."""
    who = "selfplay_puct_games_exact"
    lib = _lib.load()
    a = _games_arguments(who, boards, dice, params, sims, max_plies, c_puct, terminal_value, noise_eps, noise_alpha, temp_plies, key,
                         game_offset, cube_layer, tile, blocks, table=leaf_table, table_name="leaf_table", table_required=True)
    counts = torch.empty((a["M"], 2), dtype=torch.int32, device=a["dev"]) if return_leaf_counts else None   # every element is written
    rec = _play_games(lib, a, params, lambda *front: check(lib.ewn_puct_selfplay_eg(
        *front, leaf_table.max_cubes, leaf_table.max_total, _ptr(leaf_table.table), _ptr(counts), _stream()), "ewn_puct_selfplay_eg"))
    if return_leaf_counts:
        rec["leaf_counts"] = counts
    return rec
