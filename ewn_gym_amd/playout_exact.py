"""The playout tree search with exact endgame values at the leaves a table covers (ewn_playout_search_eg):
playout_search's trees, where a pending leaf that the EndgameTable covers takes EndgameTable.lookup's value at the action it
returns and runs no playouts, and every other leaf is played out exactly as without a table.

Host side is plumbing only, with playout_search.py's checks and error texts through its own helpers.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from ._args import _at_least_one, _ptr, _same_gpu, _stream
from .endgame import _accept_table
from .playout_search import _numbers, _observations, _rounds_and_blocks, _trees
from .search import _outputs


def _table(who, endgame_table, M, S, dev):
    """the table for the boards' size on the boards' GPU"""
    t = _accept_table(who, endgame_table, S, "boards of shape %s, the table is for %%dx%%d" % [M, S, S])
    _same_gpu(who, dev, "boards", (("endgame_table", t.table),))
    return t


def _launch(lib, S, L, n, sims, rounds, playouts, cp, key, obs_id0, blocks, t, b, d, tree, counts, st):
    check(lib.ewn_playout_search_eg(S, L, n, sims, rounds, playouts, cp, C.c_uint64(key), C.c_uint32(obs_id0 & 0xFFFFFFFF), blocks,
                                    t.max_cubes, t.max_total, _ptr(t.table), _ptr(b), _ptr(d), _ptr(tree), _ptr(counts), st),
          "ewn_playout_search_eg")


def playout_search_exact(boards, dice, sims, endgame_table, playouts=64, c_puct=1.5, key=0, obs_id0=0, rounds=None, blocks=None,
                         cube_layer=3, out=None, return_leaf_counts=False):
    """playout_search with exact values at covered leaves, in one launch (ewn_playout_search_eg) -> tree uint8
    [M, tree_bytes], or (tree, leaf_counts int32 [M, 2]) if return_leaf_counts.  Byte for byte playout_search's definition with one
    change: in every round, acts, covered, q = endgame_table.lookup(leaf rows, leaf dice, return_q=True) of the trees with a pending
    leaf; where covered, the value handed to puct_advance is q at the action the lookup returns (its first maximum under a strict >)
    and the leaf runs no playouts; elsewhere it is (2 wins - playouts) / playouts of playout_wins under the same key
    key + r * 0x9E3779B97F4A7C15 and row index obs_id0 + m as without a table.  leaf_counts[m] = (rounds whose pending leaf the table
    valued, rounds whose pending leaf playouts valued) over the rounds run.  endgame_table: an EndgameTable for the boards' size on
    the boards' GPU, complete before this call in stream order (EndgameTable.build and this call on the same stream are).
    Everything else, and every check, is playout_search's."""
    who = "playout_search_exact"
    lib = _lib.load()
    sims, playouts, key, obs_id0 = _numbers(who, sims, playouts, c_puct, key, obs_id0)
    rounds, blocks = _rounds_and_blocks(who, rounds, blocks, sims)
    M, S, dev, b, d = _observations(who, boards, dice, cube_layer)
    L = int(cube_layer)
    t = _table(who, endgame_table, M, S, dev)
    out = _trees(who, lib, out, M, S, L, sims, dev)
    counts = torch.empty((M, 2), dtype=torch.int32, device=dev) if return_leaf_counts else None
    with torch.cuda.device(dev):
        _launch(lib, S, L, M, sims, rounds, playouts, C.c_float(float(c_puct)), key, obs_id0, blocks, t, b, d, out, counts, _stream())
    return (out, counts) if return_leaf_counts else out


def predict_playout_search_exact(boards, dice, endgame_table, sims=64, playouts=64, c_puct=1.5, key=0, obs_id0=0, return_visits=False,
                                 return_q=False, return_value=False, return_leaf_counts=False, chunk=1024, cube_layer=3):
    """What predict_playout_search plays when the leaves an EndgameTable covers are worth their exact value -> actions
    int8 [M, 2], or the tuple (actions, visits, q, value, leaf_counts int32 [M, 2]) of what was asked for, the first four as
    puct_result returns them, leaf_counts as playout_search_exact does.  predict_playout_search's chunk loop: chunk i passes
    obs_id0 + i, so neither the chunk nor a split of the rows over several calls changes a bit.  playout_search_exact's checks."""
    who = "predict_playout_search_exact"
    lib = _lib.load()
    sims, playouts, key, obs_id0 = _numbers(who, sims, playouts, c_puct, key, obs_id0)
    _at_least_one(who, "chunk", chunk)
    M, S, dev, b, d = _observations(who, boards, dice, cube_layer)
    L = int(cube_layer)
    t = _table(who, endgame_table, M, S, dev)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    counts = torch.zeros((M, 2), dtype=torch.int32, device=dev) if return_leaf_counts else None
    c = max(1, min(int(chunk), M))
    tree = torch.empty((c, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    cp = C.c_float(float(c_puct))
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            sl = slice(i, i + n)
            _launch(lib, S, L, n, sims, -1, playouts, cp, key, obs_id0 + i, 0, t, b[sl], d[sl], tree, None if counts is None else counts[sl], st)
            check(lib.ewn_puct_result(S, L, n, _ptr(tree), _ptr(acts[sl]), _ptr(None if visits is None else visits[sl]),
                                      _ptr(None if q is None else q[sl]), _ptr(None if val is None else val[sl]), st), "ewn_puct_result")
    return _outputs(acts, visits, q, val, counts)
