"""The PUCT search in one launch with several leaves per tree and round (ewn_puct_search_wide): puct_search's trees,
collected up to `leaves` leaves at a time under a virtual loss, so that a search of `sims` simulations takes about sims / leaves
rounds of the two network passes instead of sims + 1.

Host side is plumbing only, as in search.py, whose checks and error texts these are: torch owns the buffers and the stream,
libewn_hip.so does the work.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _ptr, _same_gpu, _stream
from .search import _holds_trees, _network_inputs, _noise_eps, _puct_numbers, _puct_tree

PUCT_WIDE_MAX_LEAVES = 32    # the columns of a block's tile (include/ewn_puct_wide.h): a tile holds floor(32 / leaves) trees ...
PUCT_WIDE_MAX_BLOCKS = 256   # ... and the grid has at most this many blocks: more tiles are walked grid-stride


def _leaves(who, leaves):
    if not (isinstance(leaves, (int, np.integer)) and not isinstance(leaves, bool) and 1 <= int(leaves) <= PUCT_WIDE_MAX_LEAVES):
        raise ValueError("%s: leaves must be an integer in 1..%d, got %r" % (who, PUCT_WIDE_MAX_LEAVES, leaves))
    return int(leaves)


def _leaves_alone(who, leaves, **others):
    """the users' keyword: leaves > 1 is the wide launch, which has no exact leaves and plays no whole games -> leaves"""
    leaves = _leaves(who, leaves)
    for name, (on, why) in others.items():
        if leaves > 1 and on:
            raise ValueError("%s: leaves=%d does not take %s: %s" % (who, leaves, name, why))
    return leaves


_NO_TABLE = "the exact-leaf substitution is the staged path's (leaves=1, fused=False)"
_NO_WHOLE_GAMES = "ewn_puct_selfplay evaluates one leaf per tree and round (leaves=1)"


def _tile_and_blocks(who, tile, blocks, most, leaves, max_blocks):
    """tile= and blocks= of a search on 32-column tiles as the entries take them: 0 for the library's choice"""
    if tile is not None and not (isinstance(tile, (int, np.integer)) and 1 <= int(tile) <= most):
        raise ValueError("%s: tile must be None or an integer in 1..%d (32 columns, %d a tree), got %r" % (who, most, leaves, tile))
    if blocks is not None and not (isinstance(blocks, (int, np.integer)) and 1 <= int(blocks) <= max_blocks):
        raise ValueError("%s: blocks must be None or an integer in 1..%d, got %r" % (who, max_blocks, blocks))
    return 0 if tile is None else int(tile), 0 if blocks is None else int(blocks)


def _wide_scratch(lib, S, L, n, sims, dev):
    """the marks of a wide search of n observations: what it holds does not matter"""
    return torch.empty(int(check(lib.ewn_puct_search_wide_scratch_bytes(S, L, n, sims), "ewn_puct_search_wide_scratch_bytes")),
                       dtype=torch.uint8, device=dev)


def _launch(lib, S, L, n, sims, leaves, cp, tv, b, d, params, noise, eps, tile, blocks, tree, marks, st):
    check(lib.ewn_puct_search_wide(S, L, n, sims, leaves, cp, tv, _ptr(b), _ptr(d), _ptr(params), _ptr(noise), C.c_float(eps), tile, blocks,
                                   _ptr(tree), _ptr(marks), st), "ewn_puct_search_wide")


def puct_search_wide(boards, dice, params, sims, leaves, c_puct=1.5, terminal_value=1.0, root_noise=None, noise_eps=0.25, tile=None,
                     blocks=None, cube_layer=3, out=None):
    """The whole PUCT search of M observations in one launch, up to `leaves` leaves per tree and round (ewn_puct_search_wide,
    DESIGN.md 4u) -> tree uint8 [M, tree_bytes], puct_search's layout: puct_result, puct_play and puct_tree_views read it.  A round
    evaluates the leaves a tree collected in the round before and collects up to `leaves` more, each walk seeing the leaves in
    flight as one visit and one lost value on every edge above them; a walk that reaches a node of its own round ends the round's
    collection.  leaves=1 is puct_search, byte for byte; a larger value searches a different (and equally deterministic) tree in
    about sims / leaves rounds.  root_noise, noise_eps: puct_search's.  tile None: the library's trees per block, else
    1..floor(32 / leaves); blocks None: the library's grid, else 1..256 (tuning; no byte of the result depends on either).  out: a
    contiguous, 4-byte aligned uint8 tensor [M, tree_bytes] to write into (what it held does not matter).  predict_puct's argument
    checks."""
    who = "puct_search_wide"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    leaves = _leaves(who, leaves)
    eps = 0.0 if root_noise is None else _noise_eps(who, noise_eps)
    tile, blocks = _tile_and_blocks(who, tile, blocks, PUCT_WIDE_MAX_LEAVES // leaves, leaves, PUCT_WIDE_MAX_BLOCKS)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, optional=(
        ("root_noise", root_noise, torch.float32, lambda M, P: (M, 6)),))
    _same_gpu(who, dev, "params", t.items())
    if out is None:
        out = torch.empty((M, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    else:
        _holds_trees(who, "out", out, _puct_tree(who, out, S, sims, cube_layer)[0], M, dev)
    with torch.cuda.device(dev):
        _launch(lib, S, L, M, sims, leaves, C.c_float(float(c_puct)), C.c_float(float(terminal_value)), t["boards"], t["dice"], params,
                t["root_noise"], eps, tile, blocks, out, _wide_scratch(lib, S, L, M, sims, dev), _stream())
    return out
