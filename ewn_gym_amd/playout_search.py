"""The PUCT tree search that needs no network (ewn_playout_search): the trees of puct_begin / puct_advance with
uniform priors and random playouts at the leaves, a whole search per launch.  Elsewhere this is plain MCTS with chance nodes.

Host side is plumbing only, as in search.py, whose checks and error texts these are: torch owns the buffers and the stream,
libewn_hip.so does the work.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _at_least_one, _lookahead_shape, _policy_input, _ptr, _same_gpu, _stream
from .search import _device_of, _holds_trees, _outputs, _puct_numbers, _puct_tree

PLAYOUT_SEARCH_MAX_PLAYOUTS = 4096   # playouts per leaf (include/ewn_playout_search.h) ...
PLAYOUT_SEARCH_MAX_BLOCKS = 4096     # ... and the most blocks of the grid: four trees per block and trip, further trees grid-stride
KEY_STEP = 0x9E3779B97F4A7C15        # round r draws under key + r * KEY_STEP (mod 2^64)
KEY_PLY = 0xD1B54A32D192ED03         # the users' stride per ply of a game (tournament._policy, PlayoutSearchAgent): step t searches under
                                     # key + KEY_PLY * (t + 1), so that a ply's rounds and the next ply's share no key


def _numbers(who, sims, playouts, c_puct, key, obs_id0):
    sims = _puct_numbers(who, sims, c_puct)
    if not (isinstance(playouts, (int, np.integer)) and 1 <= int(playouts) <= PLAYOUT_SEARCH_MAX_PLAYOUTS):
        raise ValueError("%s: playouts must be an integer in 1..%d, got %r" % (who, PLAYOUT_SEARCH_MAX_PLAYOUTS, playouts))
    if not isinstance(key, (int, np.integer)):
        raise ValueError("%s: key must be an integer, got %r" % (who, key))
    if not (isinstance(obs_id0, (int, np.integer)) and 0 <= int(obs_id0) < 2 ** 32):
        raise ValueError("%s: obs_id0 must be an integer in 0..2^32 - 1, got %r" % (who, obs_id0))
    return sims, int(playouts), int(key) & 0xFFFFFFFFFFFFFFFF, int(obs_id0)


def _observations(who, boards, dice, cube_layer):
    """boards [S, S] or [M, S, S], dice [M], as predict_lookahead checks its own; the device is the first tensor's (host arrays are
    copied there) and must be a GPU -> (M, S, the device, boards, dice)"""
    M, S, _ = _lookahead_shape(who, boards, cube_layer)
    dev = _device_of(next((x for x in (boards, dice) if isinstance(x, torch.Tensor)), None))
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
    d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
    _same_gpu(who, dev, "boards", (("boards", b), ("dice", d)))
    return M, S, dev, b, d


def _launch(lib, S, L, n, sims, rounds, playouts, cp, key, obs_id0, blocks, b, d, tree, st):
    check(lib.ewn_playout_search(S, L, n, sims, rounds, playouts, cp, C.c_uint64(key), C.c_uint32(obs_id0 & 0xFFFFFFFF), blocks, _ptr(b), _ptr(d),
                                 _ptr(tree), st), "ewn_playout_search")


def playout_search(boards, dice, sims, playouts=64, c_puct=1.5, key=0, obs_id0=0, rounds=None, blocks=None, cube_layer=3, out=None):
    """The whole playout-valued PUCT search of M observations in one launch (ewn_playout_search) -> tree uint8
    [M, tree_bytes]: byte for byte what puct_begin and then `rounds` rounds of playout_wins(leaf rows, first_player=1, n_sims=playouts,
    key=key + r * 0x9E3779B97F4A7C15) with tree m's row at index obs_id0 + m, value = (2 wins - playouts) / playouts, and
    puct_advance with zero logits leave.  boards [S, S] or [M, S, S], dice [M] (outside 1..6: clamped).  rounds None: all sims + 1;
    an integer: min(rounds, sims + 1), 0 is puct_begin alone.  blocks None: the library's grid; 1..4096 pins it (tuning; no byte of
    the result depends on it).  puct_result, puct_play and puct_tree_views read the tree.  out: a contiguous, 4-byte aligned uint8
    tensor [M, tree_bytes] to write into (what it held does not matter).  Anything the kernel cannot read in place raises ValueError
    before a launch."""
    who = "playout_search"
    lib = _lib.load()
    sims, playouts, key, obs_id0 = _numbers(who, sims, playouts, c_puct, key, obs_id0)
    rounds, blocks = _rounds_and_blocks(who, rounds, blocks, sims)
    M, S, dev, b, d = _observations(who, boards, dice, cube_layer)
    L = int(cube_layer)
    out = _trees(who, lib, out, M, S, L, sims, dev)
    with torch.cuda.device(dev):
        _launch(lib, S, L, M, sims, rounds, playouts, C.c_float(float(c_puct)), key, obs_id0, blocks, b, d, out, _stream())
    return out


def _rounds_and_blocks(who, rounds, blocks, sims):
    """rounds= and blocks= of a whole search as the entry takes them: -1 for all rounds, 0 for the library's grid"""
    if rounds is not None and not (isinstance(rounds, (int, np.integer)) and int(rounds) >= 0):
        raise ValueError("%s: rounds must be None or an integer that is not negative, got %r" % (who, rounds))
    if blocks is not None and not (isinstance(blocks, (int, np.integer)) and 1 <= int(blocks) <= PLAYOUT_SEARCH_MAX_BLOCKS):
        raise ValueError("%s: blocks must be None or an integer in 1..%d, got %r" % (who, PLAYOUT_SEARCH_MAX_BLOCKS, blocks))
    return -1 if rounds is None else min(int(rounds), sims + 1), 0 if blocks is None else int(blocks)


def _trees(who, lib, out, M, S, L, sims, dev):
    """out= of a whole search: a fresh buffer of M trees, or the caller's, checked"""
    if out is None:
        return torch.empty((M, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    _holds_trees(who, "out", out, _puct_tree(who, out, S, sims, L)[0], M, dev)
    return out


def predict_playout_search(boards, dice, sims=64, playouts=64, c_puct=1.5, key=0, obs_id0=0, return_visits=False, return_q=False,
                           return_value=False, chunk=1024, cube_layer=3):
    """What a PUCT search of `sims` simulations plays when it has no network: every legal move gets the same prior, a
    leaf is worth the share of `playouts` uniformly random playouts its side to move wins, on [-1, 1]; a move that wins on the
    board is worth +1 and is played; the dice are chance nodes sampled in a fixed stratified order.  boards [S, S] or [M, S, S],
    dice [M] (outside 1..6: clamped) -> actions int8 [M, 2], or the tuple (actions, visits int32 [M, 2, 3], q float32 [M, 2, 3],
    value float32 [M]) of what was asked for, as puct_result returns them.  The playouts of observation m are keyed by (key,
    obs_id0 + m) alone: `chunk` observations are searched at a time on a tree buffer allocated once per call, chunk i passing
    obs_id0 + i, so neither the chunk nor a split of the rows over several calls (each with obs_id0 moved to its first row) changes
    a bit.  playout_search's argument checks."""
    who = "predict_playout_search"
    lib = _lib.load()
    sims, playouts, key, obs_id0 = _numbers(who, sims, playouts, c_puct, key, obs_id0)
    _at_least_one(who, "chunk", chunk)
    M, S, dev, b, d = _observations(who, boards, dice, cube_layer)
    L = int(cube_layer)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    c = max(1, min(int(chunk), M))
    tree = torch.empty((c, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    cp = C.c_float(float(c_puct))
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            sl = slice(i, i + n)
            _launch(lib, S, L, n, sims, -1, playouts, cp, key, obs_id0 + i, 0, b[sl], d[sl], tree, st)
            check(lib.ewn_puct_result(S, L, n, _ptr(tree), _ptr(acts[sl]), _ptr(None if visits is None else visits[sl]),
                                      _ptr(None if q is None else q[sl]), _ptr(None if val is None else val[sl]), st), "ewn_puct_result")
    return _outputs(acts, visits, q, val)
