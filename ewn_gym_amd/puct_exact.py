"""The PUCT search on the trained network in one launch with exact endgame values at the leaves a table covers (ewn_puct_search_eg,
DESIGN.md 4w): puct_search's trees, where a pending leaf that the EndgameTable covers is worth terminal_value times
EndgameTable.lookup's q at the action it returns instead of the value head's output, and every other leaf is the value head's.

Host side is plumbing only, with search.py's and wide.py's checks and error texts through their own helpers.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from ._args import _ptr, _same_gpu, _stream
from .endgame import _accept_table
from .search import _network_inputs, _noise_eps, _puct_numbers, _rounds, _search_out
from .wide import _tile_and_blocks

PUCT_EXACT_MAX_TILE = 32      # the trees a block holds at a time: the columns of its tile (include/ewn_puct_exact.h) ...
PUCT_EXACT_MAX_BLOCKS = 256   # ... and the grid's cap: more tiles are walked grid-stride


def _launch(lib, S, L, n, sims, rounds, cp, tv, b, d, params, noise, eps, tile, blocks, t, tree, counts, st):
    check(lib.ewn_puct_search_eg(S, L, n, sims, rounds, cp, tv, _ptr(b), _ptr(d), _ptr(params), _ptr(noise), C.c_float(eps), tile, blocks,
                                 t.max_cubes, t.max_total, _ptr(t.table), _ptr(tree), _ptr(counts), st), "ewn_puct_search_eg")


def puct_search_exact(boards, dice, params, sims, leaf_table, c_puct=1.5, terminal_value=1.0, root_noise=None, noise_eps=0.25, rounds=None,
                      tile=None, blocks=None, cube_layer=3, out=None, return_leaf_counts=False):
    """puct_search with exact values at covered leaves, in one launch (ewn_puct_search_eg) -> tree uint8
    [M, tree_bytes], or (tree, leaf_counts int32 [M, 2]) if return_leaf_counts.  Byte for byte puct_search's definition with one
    change: in every round, acts, covered, q = leaf_table.lookup(leaf rows, leaf dice, return_q=True); where covered, the value handed
    to puct_advance is float32(terminal_value * q) at the action the lookup returns (its first maximum under a strict >) instead of
    predict_policy's; the logits are always the policy head's.  That is predict_puct(endgame_table=)'s search with the sign of a zero
    fixed.  leaf_counts[m] = (rounds whose pending leaf the table valued, rounds whose pending leaf the value head valued) over the
    rounds run.  leaf_table: an EndgameTable for the boards' size on the boards' GPU, complete before this call in stream order
    (EndgameTable.build and this call on the same stream are).  tile None: the library's trees per block, else 1..32; blocks None: the
    library's grid, else 1..256 (tuning; no byte of the result depends on either).  Everything else, and every check, is puct_search's."""
    who = "puct_search_exact"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = 0.0 if root_noise is None else _noise_eps(who, noise_eps)
    rounds = _rounds(who, rounds, sims)
    tile, blocks = _tile_and_blocks(who, tile, blocks, PUCT_EXACT_MAX_TILE, 1, PUCT_EXACT_MAX_BLOCKS)
    if leaf_table is None:                                     # _network_inputs takes None for "no table": here there must be one
        _accept_table(who, leaf_table, None, None, name="leaf_table")
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, optional=(
        ("root_noise", root_noise, torch.float32, lambda M, P: (M, 6)),), table=leaf_table, table_name="leaf_table")
    _same_gpu(who, dev, "params", t.items())
    out = _search_out(who, lib, out, M, S, L, sims, dev)
    counts = torch.empty((M, 2), dtype=torch.int32, device=dev) if return_leaf_counts else None
    with torch.cuda.device(dev):
        _launch(lib, S, L, M, sims, rounds, C.c_float(float(c_puct)), C.c_float(float(terminal_value)), t["boards"], t["dice"], params,
                t["root_noise"], eps, tile, blocks, leaf_table, out, counts, _stream())
    return (out, counts) if return_leaf_counts else out
