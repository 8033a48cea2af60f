"""ewn_predict_lookahead on the host: the declaration and the export, the arguments the entry point refuses before anything is launched
(ewn_predict_policy's order, then the terminal value), and the checks of the Python binding predict_lookahead (no kernel runs here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4


def call(board_size=5, cube_layer=3, M=4, boards=16, dice=16, params=16, terminal_value=1.0, actions=16, q=None):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    p = lambda a: None if a is None else C.c_void_p(a)   # noqa: E731
    return _lib.load().ewn_predict_lookahead(board_size, cube_layer, M, p(boards), p(dice), p(params), terminal_value, p(actions), p(q), None)


def test_entry_point_is_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int ewn_predict_lookahead\(", hdr, re.M)
    assert "ewn_predict_lookahead" in _lib.EXPORTS and lib.ewn_predict_lookahead is not None
    assert lib.ewn_abi_version() == 4          # the export is additive


@pytest.mark.parametrize("name", ["boards", "dice", "params", "actions"])
def test_missing_required_pointer(name):
    assert call(**{name: None}) == ENULL
    assert call(board_size=7, **{name: None}) == ENULL
    assert call(terminal_value=float("nan"), **{name: None}) == ENULL      # the pointers are looked at before the terminal value


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert call(M=0) == OK
    assert call(M=0, boards=None, dice=None, params=None, actions=None) == OK
    assert call(M=0, board_size=7, q=16, terminal_value=float("inf")) == OK


def test_invalid_and_unsupported_arguments():
    assert call(M=-1) == EINVAL
    assert call(M=-1, board_size=6) == EINVAL                              # M < 0 comes first
    for S in (6, 8):
        assert call(board_size=S) == EUNSUPPORTED
        assert call(board_size=S, M=0) == EUNSUPPORTED
    for L in (2, 4):
        assert call(cube_layer=L) == EUNSUPPORTED
        assert call(board_size=7, cube_layer=L) == EUNSUPPORTED
    # ... exactly where ewn_policy_param_count is unsupported
    lib = _lib.load()
    for S in range(3, 12):
        for L in range(1, 5):
            assert (call(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    for tv in (float("nan"), float("inf"), float("-inf")):
        assert call(terminal_value=tv) == EINVAL
        assert call(board_size=7, terminal_value=tv, q=16) == EINVAL
        assert call(board_size=6, terminal_value=tv) == EUNSUPPORTED       # the geometry is looked at before the terminal value


def test_predict_lookahead_checks_its_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.vec_env import predict_lookahead
    assert ewn_gym_amd.predict_lookahead is predict_lookahead
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    with pytest.raises(ValueError, match="params"):            # wrong size: a 7x7 vector for 5x5 boards
        predict_lookahead(boards, dice, torch.zeros(_lib.load().ewn_policy_param_count(7, 3)))
    with pytest.raises(ValueError, match="params"):
        predict_lookahead(boards, dice, torch.zeros(n, dtype=torch.float64))
    with pytest.raises(ValueError, match="params"):
        predict_lookahead(boards, dice, torch.zeros(2 * n)[::2])
    with pytest.raises(ValueError, match="GPU"):               # everything well-formed, but host tensors
        predict_lookahead(boards, dice, torch.zeros(n))
    with pytest.raises(ValueError, match="GPU"):
        predict_lookahead(np.zeros((5, 5), np.int8), [3], torch.zeros(n))
    with pytest.raises(ValueError, match="predict_lookahead: boards.*not contiguous"):
        predict_lookahead(torch.zeros((4, 5, 8), dtype=torch.int8)[:, :, :5], dice, torch.zeros(n))
    with pytest.raises(ValueError, match="boards"):            # int64 boards are not converted behind the caller's back
        predict_lookahead(boards.to(torch.int64), dice, torch.zeros(n))
    with pytest.raises(ValueError, match="dice"):
        predict_lookahead(boards, torch.ones(3, dtype=torch.int8), torch.zeros(n))
    with pytest.raises(ValueError, match="terminal_value"):
        predict_lookahead(boards, dice, torch.zeros(n), terminal_value=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        predict_lookahead(torch.zeros((4, 5, 6), dtype=torch.int8), dice, torch.zeros(n))
    with pytest.raises(ValueError, match="6x6"):
        predict_lookahead(torch.zeros((4, 6, 6), dtype=torch.int8), dice, torch.zeros(n))


def test_the_agent_class_is_exported_and_the_placeholder_points_at_it():
    import classical_policies as cp
    from classical_policies.model import ModelAgent, ValueSearchAgent
    assert cp.ValueSearchAgent is ValueSearchAgent and "ValueSearchAgent" in cp.__all__ and issubclass(ValueSearchAgent, ModelAgent)
    with pytest.raises(NotImplementedError, match="ValueSearchAgent"):
        cp.AlphaZeroMinimaxAgent(3, 3, 5)
