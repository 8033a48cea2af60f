"""ewn_policy_eval_mcts / ewn_policy_eval_mcts_supported on the host: which configurations the network-against-MCTS rollout serves,
the arguments the entry point refuses before anything is launched, and the answers of the older entry points it must not change
(no kernel runs here)."""
import ctypes as C
import os
import re

import pytest

from ewn_gym_amd import _lib
from ewn_gym_amd._lib import AGENT, EwnAgent, EwnConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
MCTS = _lib.OPP["mcts"]


def cfg(**kw):
    base = dict(board_size=5, cube_layer=3, n_lanes=64, opponent_kind=MCTS, max_depth=3, heuristic=0, num_simulations=10,
                num_env_copies=5, rng_kind=0, shaped=0, illegal_move_tolerance=10, autoreset=0, shaped_refresh_on_reset=0,
                lane_offset=0, seed_stride=64, mt_window=0, reward=1.0, illegal_move_reward=-1.0, philox_key=0)
    base.update(kw)
    return EwnConfig(**base)


def supported(**kw):
    return _lib.load().ewn_policy_eval_mcts_supported(C.byref(cfg(**kw)))


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    for name in ("ewn_policy_eval_mcts_supported", "ewn_policy_eval_mcts"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.ewn_abi_version() == 4


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng_kind", [0, 1])
@pytest.mark.parametrize("sims", [(10, 5), (3, 2), (1, 1), (100, 10)])
def test_supported_configurations(S, rng_kind, sims):
    assert supported(board_size=S, rng_kind=rng_kind, num_simulations=sims[0], num_env_copies=sims[1]) == 1


def test_unsupported_configurations():
    assert supported(shaped=1) == 0
    assert supported(rng_kind=1, autoreset=1) == 0
    assert supported(rng_kind=0, autoreset=1) == 0
    for S in (6, 8, 9):
        assert supported(board_size=S) == 0, S
    assert supported(board_size=5, cube_layer=2) == 0
    assert supported(board_size=7, cube_layer=2) == 0
    assert supported(board_size=7, cube_layer=4) == 0
    assert supported(opponent_kind=0) == 0                                                           # RandomAgent: ewn_policy_eval's
    assert supported(opponent_kind=1, max_depth=5) == 0                                              # minimax: ewn_policy_eval's


def test_invalid_configurations():
    assert supported(n_lanes=0) < 0
    assert supported(rng_kind=7) < 0
    assert supported(num_simulations=0) < 0


def _state(tables=True):
    fake = C.c_void_p(16)       # never dereferenced: every call below returns before a launch
    return _lib.EwnState(fake, fake, fake, fake, None, None, fake if tables else None)


def _out(**kw):
    fake = C.c_void_p(16)
    base = dict(return_sum=fake, n_steps=fake, n_episodes=fake, n_wins=fake)
    base.update(kw)
    return _lib.EwnRolloutOut(**base)


def test_malformed_calls_are_refused_on_the_host():
    lib = _lib.load()
    fn = lib.ewn_policy_eval_mcts
    c, st, p = cfg(), _state(), C.c_void_p(16)
    assert fn(C.byref(c), C.byref(st), 0, p, C.byref(_out()), None) == EINVAL                     # K >= 1
    assert fn(C.byref(c), C.byref(st), -3, p, C.byref(_out()), None) == EINVAL
    assert fn(C.byref(c), None, 4, p, C.byref(_out()), None) == ENULL
    for i in range(4):                                                                             # board, dice, done, rng
        ptrs = [C.c_void_p(16)] * 4
        ptrs[i] = None
        assert fn(C.byref(c), C.byref(_lib.EwnState(*ptrs, None, None, None)), 4, p, C.byref(_out()), None) == ENULL, i
    assert fn(C.byref(c), C.byref(st), 4, None, C.byref(_out()), None) == ENULL                    # params
    assert fn(C.byref(c), C.byref(st), 4, p, None, None) == ENULL                                  # the totals are required
    for name in ("return_sum", "n_steps", "n_episodes", "n_wins"):
        assert fn(C.byref(c), C.byref(st), 4, p, C.byref(_out(**{name: None})), None) == ENULL, name
    for name in ("board", "dice", "reward", "terminated", "truncated", "info", "record"):
        assert fn(C.byref(c), C.byref(st), 4, p, C.byref(_out(**{name: C.c_void_p(16)})), None) == EINVAL, name
    # unsupported configurations, well-formed otherwise
    for bad in (cfg(shaped=1), cfg(rng_kind=1, autoreset=1), cfg(board_size=6), cfg(board_size=8), cfg(cube_layer=2),
                cfg(board_size=7, cube_layer=4), cfg(opponent_kind=0), cfg(opponent_kind=1, max_depth=5)):
        assert fn(C.byref(bad), C.byref(st), 4, p, C.byref(_out()), None) == EUNSUPPORTED
    assert fn(C.byref(cfg(n_lanes=0)), C.byref(st), 4, p, C.byref(_out()), None) == EINVAL
    assert fn(C.byref(cfg(num_simulations=0)), C.byref(st), 4, p, C.byref(_out()), None) == EINVAL


def test_a_missing_table_image_is_not_a_reason_to_refuse():
    """ewn_state.tables is not needed: with tables NULL the call gets past its NULL checks to the checks behind them (a forbidden
    column: EINVAL; an unsupported configuration: EUNSUPPORTED), where ewn_policy_eval answers ENULL"""
    lib = _lib.load()
    st, p = _state(tables=False), C.c_void_p(16)
    assert lib.ewn_policy_eval_mcts(C.byref(cfg()), C.byref(st), 4, p, C.byref(_out(board=C.c_void_p(16))), None) == EINVAL
    assert lib.ewn_policy_eval_mcts(C.byref(cfg(shaped=1)), C.byref(st), 4, p, C.byref(_out()), None) == EUNSUPPORTED
    assert lib.ewn_policy_eval(C.byref(cfg(opponent_kind=1, max_depth=5)), C.byref(st), 4, p, C.byref(_out()), None) == ENULL


def test_the_older_entry_points_answer_as_before():
    lib = _lib.load()
    assert lib.ewn_policy_eval_supported(C.byref(cfg(opponent_kind=MCTS))) == 0
    assert lib.ewn_policy_eval(C.byref(cfg(opponent_kind=MCTS)), C.byref(_state()), 4, C.c_void_p(16), C.byref(_out()), None) == EUNSUPPORTED
    assert C.sizeof(EwnAgent) == 32
    mlp = EwnAgent(kind=AGENT["mlp"], max_depth=0, heuristic=0, num_simulations=0, num_env_copies=0, step_base=0, key=0)
    assert lib.ewn_step_k_agent_supported(C.byref(cfg(rng_kind=1)), C.byref(mlp)) == 0
    # ewn_step_k_supported(cfg, EWN_AGENT_MLP, 0): the policy rollout's own plan (Philox dice, RandomAgent / minimax max_depth <= 4)
    assert lib.ewn_step_k_supported(C.byref(cfg(opponent_kind=MCTS, rng_kind=1)), AGENT["mlp"], 0) == 0
    assert lib.ewn_step_k_supported(C.byref(cfg(opponent_kind=1, rng_kind=0, max_depth=3)), AGENT["mlp"], 0) == 0
    assert lib.ewn_step_k_supported(C.byref(cfg(opponent_kind=1, rng_kind=1, max_depth=5)), AGENT["mlp"], 0) == 0
    assert lib.ewn_step_k_supported(C.byref(cfg(opponent_kind=1, rng_kind=1, max_depth=3)), AGENT["mlp"], 0) == 1
