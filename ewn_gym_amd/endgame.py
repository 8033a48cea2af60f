"""Exact endgame values: EndgameTable, the retrograde table of every position with few cubes left.

EWN's game graph is acyclic -- every move brings the mover's cube closer to its corner or removes a cube -- so with at most
`max_cubes` cubes a side and `max_total` in all the expectiminimax value of every position is a finite dynamic program.  The table
is built on the device (ewn_endgame_build, one launch per level of the summed Manhattan distances) and read by ewn_endgame_lookup:
the exact q of the six env actions, the exact move and the exact value wherever the position is covered.  It is what the critic and
the lookahead are measured against, and the exact target and move where it applies; it does not replace the search.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _describe, _lookahead_shape, _policy_input, _ptr, _require_gpu, _same_gpu, _stream


class EndgameTable:
    """E(b) for every live position with 1..max_cubes cubes a side and at most max_total in all, seen from the side to move before
    its dice (the mover is TOP_LEFT); (1 + E) / 2 is the mover's win probability under optimal play by both sides.
    Attributes: board_size, max_cubes, max_total, table (the float32 device tensor; its layout is the library's, versioned as LAYOUT
    in saved files), levels (the 2 * max_total * (board_size - 1) levels of the build)."""

    LAYOUT = 1   # csrc/ewn_endgame.hip: a block per (ka, ko), side = mask rank * C^k + the cells in cube-number order

    def __init__(self, board_size, max_cubes, max_total, table):
        """wraps a built table; use EndgameTable.build or EndgameTable.load"""
        board_size, max_cubes, max_total = self._parameters(board_size, max_cubes, max_total)
        n = int(_lib.load().ewn_endgame_table_bytes(board_size, max_cubes, max_total))
        if not (isinstance(table, torch.Tensor) and table.dtype == torch.float32 and table.is_contiguous() and table.numel() * 4 == n):
            raise ValueError("EndgameTable: the table of (%d, %d, %d) is a contiguous float32 tensor of %d elements, got %s" % (
                board_size, max_cubes, max_total, n // 4, _describe(table)))
        self.board_size, self.max_cubes, self.max_total, self.table = board_size, max_cubes, max_total, table
        self.levels = 2 * max_total * (board_size - 1)

    @staticmethod
    def _parameters(board_size, max_cubes, max_total):
        S, K = int(board_size), int(max_cubes)
        T = 2 * K if max_total is None else int(max_total)
        if _lib.load().ewn_endgame_table_bytes(S, K, T) < 0:
            raise ValueError("EndgameTable: board_size 3..11, max_cubes 1..3 and max_total 2..2 * max_cubes, got (%r, %r, %r)" % (
                board_size, max_cubes, max_total))
        return S, K, T

    @staticmethod
    def table_bytes(board_size=5, max_cubes=2, max_total=None):
        S, K, T = EndgameTable._parameters(board_size, max_cubes, max_total)
        return int(_lib.load().ewn_endgame_table_bytes(S, K, T))

    @classmethod
    def build(cls, board_size=5, max_cubes=2, max_total=None, device=None, out=None):
        """max_total None: 2 * max_cubes.  device None: the current GPU.  out: a float32 device tensor of table_bytes() / 4 elements to
        build into (its contents do not matter: every slot is written)."""
        S, K, T = cls._parameters(board_size, max_cubes, max_total)
        n = int(_lib.load().ewn_endgame_table_bytes(S, K, T))
        if out is None:
            dev = _require_gpu("cuda" if device is None else device)
            out = torch.empty(n // 4, dtype=torch.float32, device=dev)
        self = cls(S, K, T, out)
        if not out.is_cuda:
            raise ValueError("EndgameTable.build: the table must live on the GPU, got %s" % _describe(out))
        with torch.cuda.device(out.device):
            check(_lib.load().ewn_endgame_build(S, K, T, _ptr(out), n, _stream()), "ewn_endgame_build")
        return self

    def lookup(self, boards, dice, return_q=False, return_value=False):
        """boards [S, S] or [M, S, S], dice [M] (outside 1..6: clamped) -> (actions int8 [M, 2], covered bool [M]), then q float32
        [M, 2, 3] if return_q and value float32 [M] if return_value.  Where covered: q is the exact value of each env action (f, r)
        under that dice (-inf where it leaves the board, +1 where it wins), actions the first maximum of q, value E(b).  Elsewhere:
        (0, 0), six -inf, 0.  predict_policy's argument checks: a tensor is read in place and must be a contiguous int8 tensor on the
        table's GPU; host arrays are copied over; anything else raises ValueError before a launch."""
        who = "EndgameTable.lookup"
        S, dev = self.board_size, self.table.device
        M, Sb, _ = _lookahead_shape(who, boards)
        if Sb != S:
            raise ValueError("%s: boards of shape %s, the table is for %dx%d" % (who, [M, Sb, Sb], S, S))
        b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
        d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
        _same_gpu(who, dev, "the table", (("table", self.table), ("boards", b), ("dice", d)))
        acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
        covered = torch.zeros(M, dtype=torch.bool, device=dev)
        q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
        value = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
        with torch.cuda.device(dev):
            check(_lib.load().ewn_endgame_lookup(S, self.max_cubes, self.max_total, _ptr(self.table), M, _ptr(b), _ptr(d), _ptr(acts),
                                                 _ptr(q), _ptr(value), _ptr(covered), _stream()), "ewn_endgame_lookup")
        return (acts, covered) + ((q,) if return_q else ()) + ((value,) if return_value else ())

    def value(self, boards):
        """E(b) float32 [M] of the positions `boards` (0 where a position is not covered; lookup tells which)"""
        shp = tuple(boards.shape) if isinstance(boards, torch.Tensor) else np.asarray(boards).shape
        dice = torch.ones(1 if len(shp) == 2 else int(shp[0]), dtype=torch.int8, device=self.table.device)
        return self.lookup(boards, dice, return_value=True)[2]

    def save(self, path):
        torch.save({"endgame_layout": self.LAYOUT, "board_size": self.board_size, "max_cubes": self.max_cubes,
                    "max_total": self.max_total, "table": self.table}, path)

    @classmethod
    def load(cls, path, device=None):
        """a table written by save(); ValueError for a file of another layout version, or one whose table does not fit its parameters"""
        dev = _require_gpu("cuda" if device is None else device)
        sd = torch.load(os.fspath(path), map_location=dev, weights_only=True)
        if not isinstance(sd, dict) or "endgame_layout" not in sd:
            raise ValueError("%s is not an endgame table (EndgameTable.save)" % (path,))
        if sd["endgame_layout"] != cls.LAYOUT:
            raise ValueError("%s holds table layout %r, this library reads layout %d: build it again" % (path, sd["endgame_layout"], cls.LAYOUT))
        return cls(sd["board_size"], sd["max_cubes"], sd["max_total"], sd["table"].contiguous())


def _accept_table(who, table, board_size, other_size, name="endgame_table", load=None):
    """The endgame table that a caller was given as its argument `name`: an EndgameTable, or -- where the caller says how it loads
    one, load(path) -- the path of a saved one.  board_size: what the caller plays (None: any); other_size: its own sentence about a
    table of another size, the table's size left open twice.  -> the table, else ValueError"""
    if load is not None and isinstance(table, (str, os.PathLike)):
        table = load(table)
    if not isinstance(table, EndgameTable):
        raise ValueError("%s: %s must be an EndgameTable%s, got %s" % (who, name, "" if load is None else " or the path of a saved one",
                                                                       type(table).__name__))
    if board_size is not None and table.board_size != board_size:
        raise ValueError("%s: %s" % (who, other_size % (table.board_size, table.board_size)))
    return table
