"""ewn_lookahead_expand / ewn_lookahead_reduce and predict_lookahead(plies=2) on the host: the declarations and the exports,
the arguments the two entry points refuse before anything is launched and the order they are looked at in (ewn_predict_lookahead's:
arguments, geometry, the empty batch, pointers, then the values), the Python bindings' ValueErrors, the agent's and the tournament's
`plies`.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
INT_MAX = 2 ** 31 - 1
M_LAST = INT_MAX // 648            # 3 314 017: the largest batch whose 648 M leaf rows an int counts
M_BIG = 3313962                    # a batch of that order that is still served


def p(a):
    return None if a is None else C.c_void_p(a)


def expand(board_size=5, cube_layer=3, M=4, boards=16, dice=16, leaf_boards=16, leaf_dice=16, kind=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_lookahead_expand(board_size, cube_layer, M, p(boards), p(dice), p(leaf_boards), p(leaf_dice), p(kind), None)


def reduce(board_size=5, cube_layer=3, M=4, boards=16, dice=16, kind=16, leaf=16, leaf_width=1, terminal_value=1.0, actions=16, q=None):
    return _lib.load().ewn_lookahead_reduce(board_size, cube_layer, M, p(boards), p(dice), p(kind), p(leaf), leaf_width, terminal_value,
                                            p(actions), p(q), None)


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    for name in ("ewn_lookahead_expand", "ewn_lookahead_reduce"):
        assert re.search(r"^int %s\(" % name, hdr, re.M)
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.ewn_lookahead_expand.argtypes) == 9 and len(lib.ewn_lookahead_reduce.argtypes) == 12
    assert lib.ewn_lookahead_reduce.argtypes[8] is C.c_float and lib.ewn_lookahead_reduce.argtypes[7] is C.c_int
    assert lib.ewn_abi_version() == 4          # the exports are additive


@pytest.mark.parametrize("name", ["boards", "dice", "leaf_boards", "leaf_dice", "kind"])
def test_expand_missing_pointer(name):
    assert expand(**{name: None}) == ENULL
    assert expand(board_size=7, **{name: None}) == ENULL
    assert expand(M=M_BIG, **{name: None}) == ENULL                          # 648 M still fits an int: the pointers are looked at
    assert expand(M=M_LAST, **{name: None}) == ENULL


@pytest.mark.parametrize("name", ["boards", "dice", "kind", "leaf", "actions"])
def test_reduce_missing_pointer(name):
    assert reduce(**{name: None}) == ENULL
    assert reduce(board_size=7, leaf_width=6, **{name: None}) == ENULL
    assert reduce(terminal_value=float("nan"), **{name: None}) == ENULL     # the pointers are looked at before the terminal value ...
    assert reduce(leaf_width=2, **{name: None}) == ENULL                    # ... and before the width
    assert reduce(M=M_BIG, **{name: None}) == ENULL
    assert reduce(M=M_LAST, **{name: None}) == ENULL


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert expand(M=0) == OK and reduce(M=0) == OK
    assert expand(M=0, boards=None, dice=None, leaf_boards=None, leaf_dice=None, kind=None) == OK
    assert reduce(M=0, boards=None, dice=None, kind=None, leaf=None, actions=None) == OK
    assert reduce(M=0, board_size=7, q=16, terminal_value=float("inf"), leaf_width=2) == OK   # M == 0 comes before the values


def test_invalid_and_unsupported_arguments():
    lib = _lib.load()
    for call in (expand, reduce):
        assert call(M=-1) == EINVAL
        assert call(M=-1, board_size=6) == EINVAL                            # M < 0 comes first
        assert call(M=M_LAST + 1) == EINVAL and call(M=INT_MAX) == EINVAL    # 648 M > INT_MAX
        assert call(M=M_LAST + 1, board_size=6) == EINVAL and call(M=M_LAST + 1, boards=None) == EINVAL
        assert call(M=M_BIG, board_size=6) == EUNSUPPORTED                   # in range: the geometry is looked at next
        for S in (6, 8):
            assert call(board_size=S) == EUNSUPPORTED
            assert call(board_size=S, M=0) == EUNSUPPORTED
            assert call(board_size=S, boards=None) == EUNSUPPORTED           # the geometry is looked at before the pointers
        for L in (2, 4):
            assert call(cube_layer=L) == EUNSUPPORTED
            assert call(board_size=7, cube_layer=L) == EUNSUPPORTED
        for S in range(3, 12):                                               # ... exactly where ewn_policy_param_count is unsupported
            for L in range(1, 5):
                assert (call(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    for tv in (float("nan"), float("inf"), float("-inf")):
        assert reduce(terminal_value=tv) == EINVAL
        assert reduce(board_size=7, terminal_value=tv, q=16, leaf_width=6) == EINVAL
        assert reduce(board_size=6, terminal_value=tv) == EUNSUPPORTED       # the geometry is looked at before the terminal value
    for w in (0, 2, 3, 5, 7, -1, 648):
        assert reduce(leaf_width=w) == EINVAL
        assert reduce(board_size=7, leaf_width=w, q=16) == EINVAL
        assert reduce(board_size=8, leaf_width=w) == EUNSUPPORTED
        assert reduce(M=M_BIG, leaf_width=w) == EINVAL


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.vec_env import lookahead_expand, lookahead_reduce, predict_lookahead
    assert ewn_gym_amd.lookahead_expand is lookahead_expand and ewn_gym_amd.lookahead_reduce is lookahead_reduce
    assert "lookahead_expand" in ewn_gym_amd.__all__ and "lookahead_reduce" in ewn_gym_amd.__all__
    boards, dice = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    kind, leaf = torch.zeros((4, 108), dtype=torch.int8), torch.zeros((4, 648))
    # expand
    with pytest.raises(ValueError, match="lookahead_expand: boards.*GPU"):   # everything well-formed, but host tensors
        lookahead_expand(boards, dice)
    with pytest.raises(ValueError, match="lookahead_expand: boards.*not contiguous"):
        lookahead_expand(torch.zeros((4, 5, 8), dtype=torch.int8)[:, :, :5], dice)
    with pytest.raises(ValueError, match="lookahead_expand: boards"):        # int64 boards are not converted behind the caller's back
        lookahead_expand(boards.to(torch.int64), dice)
    with pytest.raises(ValueError, match="lookahead_expand: dice"):
        lookahead_expand(boards, torch.ones(3, dtype=torch.int8))
    with pytest.raises(ValueError, match="shape"):
        lookahead_expand(torch.zeros((4, 5, 6), dtype=torch.int8), dice)
    with pytest.raises(ValueError, match="6x6"):
        lookahead_expand(torch.zeros((4, 6, 6), dtype=torch.int8), dice)
    with pytest.raises(ValueError, match="cube_layer 2"):
        lookahead_expand(boards, dice, cube_layer=2)
    # reduce
    with pytest.raises(ValueError, match="lookahead_reduce: boards.*GPU"):
        lookahead_reduce(boards, dice, kind, leaf)
    with pytest.raises(ValueError, match="lookahead_reduce: boards.*GPU"):
        lookahead_reduce(boards, dice, kind, torch.zeros((4, 648, 6)), return_q=True)
    with pytest.raises(ValueError, match="lookahead_reduce: kind"):
        lookahead_reduce(boards, dice, kind.to(torch.int32), leaf)
    with pytest.raises(ValueError, match="lookahead_reduce: kind"):
        lookahead_reduce(boards, dice, kind[:3], leaf)
    with pytest.raises(ValueError, match="lookahead_reduce: leaf"):
        lookahead_reduce(boards, dice, kind, leaf.double())
    with pytest.raises(ValueError, match="lookahead_reduce: leaf"):
        lookahead_reduce(boards, dice, kind, leaf[:3])
    with pytest.raises(ValueError, match=r"leaf must have shape \[M, 648\] or \[M, 648, 6\]"):
        lookahead_reduce(boards, dice, kind, torch.zeros((4, 648, 2)))
    with pytest.raises(ValueError, match=r"leaf must have shape"):
        lookahead_reduce(boards, dice, kind, torch.zeros(4 * 648))
    with pytest.raises(ValueError, match="terminal_value"):
        lookahead_reduce(boards, dice, kind, leaf, terminal_value=float("inf"))
    with pytest.raises(ValueError, match="6x6"):
        lookahead_reduce(torch.zeros((4, 6, 6), dtype=torch.int8), dice, kind, leaf)
    # predict_lookahead's new keywords, looked at first
    n = _lib.load().ewn_policy_param_count(5, 3)
    for plies in (0, 3, -1, 1.5, None):
        with pytest.raises(ValueError, match="plies"):
            predict_lookahead(boards, dice, torch.zeros(n), plies=plies)
    for chunk in (0, -5):
        with pytest.raises(ValueError, match="chunk"):
            predict_lookahead(boards, dice, torch.zeros(n), plies=2, chunk=chunk)
    with pytest.raises(ValueError, match="GPU"):               # plies=2 keeps the checks of plies=1
        predict_lookahead(boards, dice, torch.zeros(n), plies=2)
    with pytest.raises(ValueError, match="params"):
        predict_lookahead(boards, dice, torch.zeros(n + 1), plies=2, chunk=7)
    with pytest.raises(ValueError, match="GPU"):
        predict_lookahead(np.zeros((5, 5), np.int8), [3], torch.zeros(n), plies=2)


def test_the_agent_takes_plies(monkeypatch):
    torch = pytest.importorskip("torch")
    from classical_policies import ValueSearchAgent
    n = _lib.load().ewn_policy_param_count(5, 3)
    with pytest.raises(ValueError, match="plies"):
        ValueSearchAgent(torch.zeros(n), plies=3)
    with pytest.raises(ValueError, match="plies"):
        ValueSearchAgent(torch.zeros(n), plies=0)
    real = torch.Tensor.to                 # the constructor on a host without a device: its parameters stay where they are
    monkeypatch.setattr(torch.Tensor, "to", lambda t, *a, **k: t if a[:1] == ("cuda",) else real(t, *a, **k))
    assert ValueSearchAgent(torch.zeros(n), plies=2).plies == 2
    assert ValueSearchAgent(torch.zeros(n)).plies == 1
    assert ValueSearchAgent(torch.zeros(n), terminal_value=0.5, plies=2).terminal_value == 0.5


def test_the_command_line_takes_an_optional_depth():
    from ewn_gym_amd.tournament import _parser
    ap = _parser()
    assert ap.parse_args([]).lookahead is None
    assert ap.parse_args(["--model", "m.pt", "--lookahead"]).lookahead == 1            # the bare flag: one move, as before
    assert ap.parse_args(["--lookahead", "--model", "m.pt"]).lookahead == 1
    assert ap.parse_args(["--model", "m.pt", "--lookahead", "1"]).lookahead == 1
    assert ap.parse_args(["--model", "m.pt", "--lookahead", "2"]).lookahead == 2
    for bad in ("3", "0", "two"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--model", "m.pt", "--lookahead", bad])
