"""ewn_predict_lookahead_eg on the host: the declaration and the export, the refusals of the entry point in their order
(small fake addresses: every call here returns before a launch), and the checks and signatures of the Python layers that take an
endgame table for the leaves (no kernel runs here)."""
import ctypes as C
import inspect
import os
import re

import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
NAN = float("nan")


def call(board_size=5, cube_layer=3, M=4, boards=16, dice=16, params=16, terminal_value=1.0, max_cubes=2, max_total=4, table=16, actions=16,
         q=None, leaf_counts=None):
    p = lambda a: None if a is None else C.c_void_p(a)   # noqa: E731
    return _lib.load().ewn_predict_lookahead_eg(board_size, cube_layer, M, p(boards), p(dice), p(params), terminal_value, max_cubes, max_total,
                                                p(table), p(actions), p(q), p(leaf_counts), None)


def test_entry_point_is_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int ewn_predict_lookahead_eg\(", hdr, re.M)
    assert "ewn_predict_lookahead_eg" in _lib.EXPORTS and lib.ewn_predict_lookahead_eg is not None
    assert lib.ewn_abi_version() == 4          # the export is additive


def test_refusals_and_their_order():
    lib = _lib.load()
    nothing = dict(boards=None, dice=None, params=None, table=None, actions=None)
    # 1. M < 0 before everything
    assert call(M=-1) == EINVAL
    assert call(M=-1, board_size=6, max_cubes=9, terminal_value=NAN, **nothing) == EINVAL
    # 2. the geometry of the network before the table's parameters
    for S, L in ((6, 3), (8, 3), (5, 2), (7, 4), (3, 3)):
        assert call(board_size=S, cube_layer=L) == EUNSUPPORTED
        assert call(board_size=S, cube_layer=L, max_cubes=9, M=0, terminal_value=NAN, **nothing) == EUNSUPPORTED
    # 3. the table's parameters exactly where ewn_endgame_table_bytes refuses them, before the empty batch and the pointers
    for S in (5, 7):
        for K in range(0, 5):
            for T in range(0, 9):
                ok = lib.ewn_endgame_table_bytes(S, K, T) >= 0
                assert (call(board_size=S, max_cubes=K, max_total=T, M=0, **nothing) == OK) == ok, (S, K, T)
                assert call(board_size=S, max_cubes=K, max_total=T, terminal_value=NAN, **nothing) == (ENULL if ok else EINVAL), (S, K, T)
    # 4. the empty batch is OK with nothing touched, before the pointers and the terminal value
    assert call(M=0) == OK and call(M=0, terminal_value=float("inf"), q=16, leaf_counts=16, **nothing) == OK
    # 5. every required pointer, before the terminal value; q and leaf_counts are optional
    for name in nothing:
        assert call(**{name: None}) == ENULL
        assert call(board_size=7, max_total=3, terminal_value=NAN, **{name: None}) == ENULL
    # 6. the terminal value last
    for tv in (NAN, float("inf"), float("-inf")):
        assert call(terminal_value=tv) == EINVAL
        assert call(board_size=7, max_total=3, terminal_value=tv, q=16, leaf_counts=16) == EINVAL


def test_the_new_keyword_arguments_and_their_defaults():
    from classical_policies.model import PuctAgent, ValueSearchAgent
    from ewn_gym_amd import tournament, train_a2c
    from ewn_gym_amd.distill import SearchDistillTrainer
    from ewn_gym_amd.vec_env import predict_lookahead, predict_puct
    default = lambda f, name: inspect.signature(f).parameters[name].default   # noqa: E731
    assert default(predict_lookahead, "endgame_table") is None and default(predict_lookahead, "return_leaf_counts") is False
    assert default(predict_puct, "endgame_table") is None
    assert default(ValueSearchAgent.__init__, "endgame_table") is None and default(PuctAgent.__init__, "endgame_table") is None
    assert default(SearchDistillTrainer.__init__, "endgame_leaves") is False
    assert default(tournament.evaluate_model, "endgame_leaves") is False
    assert tournament._parser().parse_args([]).endgame_leaves is False
    assert tournament._parser().parse_args(["--model", "m.pt", "--lookahead", "--endgame_table", "t.pt", "--endgame_leaves"]).endgame_leaves is True
    assert train_a2c._parser().parse_args(["SEARCH"]).endgame_leaves is False
    assert train_a2c._parser().parse_args(["SEARCH", "--endgame_table", "t.pt", "--endgame_leaves"]).endgame_leaves is True


def test_the_bindings_check_the_table_before_any_launch():
    torch = pytest.importorskip("torch")
    from classical_policies.model import PuctAgent, ValueSearchAgent
    from ewn_gym_amd.distill import SearchDistillTrainer
    from ewn_gym_amd.endgame import EndgameTable
    from ewn_gym_amd.tournament import evaluate_model
    from ewn_gym_amd.vec_env import predict_lookahead, predict_puct
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, params = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    small = EndgameTable(3, 1, 2, torch.zeros(EndgameTable.table_bytes(3, 1, 2) // 4))      # a 3x3 table, on the host: never read
    host = EndgameTable(5, 1, 2, torch.zeros(EndgameTable.table_bytes(5, 1, 2) // 4))
    for f in (predict_lookahead, predict_puct):
        with pytest.raises(ValueError, match="endgame_table must be an EndgameTable, got Tensor"):
            f(boards, dice, params, endgame_table=small.table)
        with pytest.raises(ValueError, match="endgame_table must be an EndgameTable, got str"):
            f(boards, dice, params, endgame_table="table.pt")
        with pytest.raises(ValueError, match=r"boards of shape \[4, 5, 5\], the table is for 3x3"):
            f(boards, dice, params, endgame_table=small)
        with pytest.raises(ValueError, match="GPU"):               # the right table, but nothing lives on a GPU
            f(boards, dice, params, endgame_table=host)
    with pytest.raises(ValueError, match="3x3"):
        predict_lookahead(boards, dice, params, endgame_table=small, plies=2)
    with pytest.raises(ValueError, match="return_leaf_counts.*plies"):
        predict_lookahead(boards, dice, params, endgame_table=host, plies=2, return_leaf_counts=True)
    with pytest.raises(ValueError, match="return_leaf_counts.*plies"):
        predict_lookahead(boards, dice, params, plies=2, return_leaf_counts=True)
    with pytest.raises(ValueError, match="return_leaf_counts needs an endgame_table"):
        predict_lookahead(boards, dice, params, return_leaf_counts=True)
    with pytest.raises(ValueError, match="endgame_leaves=True needs an endgame_table"):
        SearchDistillTrainer(None, endgame_leaves=True)
    with pytest.raises(ValueError, match="endgame_leaves=True needs an endgame_table"):
        SearchDistillTrainer(None, endgame_leaves=True, search="puct", plies=2)
    with pytest.raises(ValueError, match="endgame_leaves goes with lookahead and an endgame_table"):
        evaluate_model(None, endgame_leaves=True, lookahead=1)
    with pytest.raises(ValueError, match="endgame_leaves goes with lookahead and an endgame_table"):
        evaluate_model(None, endgame_leaves=True, endgame_table=host)
    for agent in (ValueSearchAgent, PuctAgent):                    # the agents load their parameters first: they need a GPU for that
        assert "endgame_table" in inspect.signature(agent.__init__).parameters
