"""ewn_step_k_agent / ewn_step_k_agent_supported on the host: which cells of the agent-vs-opponent matrix the K-step kernel with an
agent of its own serves (the MCTS agent; the minimax agent against MCTS), and the arguments it refuses before anything is launched
(no kernel runs here)."""
import ctypes as C
import os
import re

import pytest

from ewn_gym_amd import _lib
from ewn_gym_amd._lib import HEUR, OPP, EwnConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL, EUNSUPPORTED = 0, -1, -2, -4
MINIMAX, SAMPLE, MLP, MCTS = 1, 2, 3, 4


def cfg(**kw):
    base = dict(board_size=5, cube_layer=3, n_lanes=64, opponent_kind=OPP["mcts"], max_depth=5, heuristic=0, num_simulations=10,
                num_env_copies=5, rng_kind=0, shaped=0, illegal_move_tolerance=10, autoreset=0, shaped_refresh_on_reset=0,
                lane_offset=0, seed_stride=64, mt_window=0, reward=1.0, illegal_move_reward=-1.0, philox_key=0)
    base.update(kw)
    return EwnConfig(**base)


def agent(kind=MCTS, max_depth=5, heuristic=0, num_simulations=10, num_env_copies=5, step_base=0, key=0):
    return _lib.EwnAgent(kind, max_depth, heuristic, num_simulations, num_env_copies, step_base, key)


def supported(a=None, **kw):
    return _lib.load().ewn_step_k_agent_supported(C.byref(cfg(**kw)), C.byref(a if a is not None else agent()))


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    for name in ("ewn_step_k_agent_supported", "ewn_step_k_agent"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert re.search(r"^#define EWN_AGENT_MCTS 4\b", hdr, re.M)
    assert lib.ewn_abi_version() == 4


def test_struct_layout_matches_header():
    assert C.sizeof(_lib.EwnAgent) == 6 * 4 + 8 and _lib.EwnAgent.key.offset == 24
    assert C.sizeof(EwnConfig) == 14 * 4 + 2 * 4 + 2 * 8 + 8        # unchanged
    assert C.sizeof(_lib.EwnRolloutOut) == 12 * 8


@pytest.mark.parametrize("S", [5, 6, 7, 8])
@pytest.mark.parametrize("rng_kind", [0, 1])
def test_the_four_cells_are_served(S, rng_kind):
    g = dict(board_size=S, rng_kind=rng_kind)
    assert supported(agent(MCTS), opponent_kind=OPP["random"], **g) == 1
    assert supported(agent(MCTS), opponent_kind=OPP["mcts"], **g) == 1
    for h in ("hybrid", "min_dist", "two_min_dist", "attk"):
        for d in range(1, 7):
            assert supported(agent(MCTS), opponent_kind=OPP["minimax"], max_depth=d, heuristic=HEUR[h], **g) == 1, (h, d)
            assert supported(agent(MINIMAX, max_depth=d, heuristic=HEUR[h]), opponent_kind=OPP["mcts"], **g) == 1, (h, d)
    # Philox dice also with auto-reset
    if rng_kind == 1:
        assert supported(agent(MCTS), autoreset=1, **g) == 1
        assert supported(agent(MINIMAX, max_depth=3), autoreset=1, **g) == 1


def test_everything_else_is_refused():
    assert supported(agent(MCTS), rng_kind=0, autoreset=1) == 0                         # MT19937 windows are rebuilt between launches
    assert supported(agent(MINIMAX, max_depth=3), rng_kind=0, autoreset=1) == 0
    assert supported(agent(MCTS), shaped=1) == 0
    assert supported(agent(MCTS), board_size=7, cube_layer=4) == 0                      # ten cubes a side
    assert supported(agent(MCTS), board_size=9) == 0
    # three cubes a side: the MCTS agent's playouts roll dice 1..6 (mcts.py:29), so ewn_predict_mcts itself refuses cube_num < 6
    assert supported(agent(MCTS), opponent_kind=OPP["random"], cube_layer=2) == 0
    assert supported(agent(MCTS), opponent_kind=OPP["random"], cube_layer=1, board_size=5) == 0
    assert supported(agent(MCTS), opponent_kind=OPP["minimax"], max_depth=2, heuristic=HEUR["sim_winrate"]) == 0
    assert supported(agent(MINIMAX, max_depth=2, heuristic=HEUR["sim_winrate"])) == 0
    assert supported(agent(MINIMAX, max_depth=0)) == EINVAL
    assert supported(agent(MINIMAX, max_depth=7)) == 0
    assert supported(agent(MINIMAX, heuristic=5)) == EINVAL
    assert supported(agent(MINIMAX, max_depth=3), opponent_kind=OPP["random"]) == 0     # ewn_step_k's cells
    assert supported(agent(MINIMAX, max_depth=3), opponent_kind=OPP["minimax"]) == 0
    assert supported(agent(MCTS, num_simulations=0)) == EINVAL
    assert supported(agent(MCTS, num_env_copies=0)) == EINVAL
    for k in (0, SAMPLE, MLP):                                                          # ewn_step_k / ewn_step_k_policy's agents
        assert supported(agent(k)) == 0
    for k in (-1, 5, 99):
        assert supported(agent(k)) == EINVAL
    assert supported(agent(MCTS), n_lanes=0) == EINVAL


def test_null_pointers_and_bad_arguments_are_refused_without_a_launch():
    lib = _lib.load()
    c, a = cfg(), agent()
    assert lib.ewn_step_k_agent_supported(None, C.byref(a)) == ENULL
    assert lib.ewn_step_k_agent_supported(C.byref(c), None) == ENULL
    st = _lib.EwnState()                                                                # every pointer NULL
    assert lib.ewn_step_k_agent(C.byref(c), C.byref(st), 4, C.byref(a), None, None) == ENULL
    assert lib.ewn_step_k_agent(C.byref(c), None, 4, C.byref(a), None, None) == ENULL
    assert lib.ewn_step_k_agent(C.byref(c), C.byref(st), 4, None, None, None) == ENULL
    assert lib.ewn_step_k_agent(None, C.byref(st), 4, C.byref(a), None, None) == ENULL
    assert lib.ewn_step_k_agent(C.byref(c), C.byref(st), 0, C.byref(a), None, None) == EINVAL
    # unsupported (agent, configuration) pairs are refused before the state is looked at
    fake = _lib.EwnState(*([C.c_void_p(16)] * 4 + [None] * 3))
    assert lib.ewn_step_k_agent(C.byref(cfg(autoreset=1)), C.byref(fake), 4, C.byref(a), None, None) == EUNSUPPORTED
    assert lib.ewn_step_k_agent(C.byref(cfg(opponent_kind=0)), C.byref(fake), 4, C.byref(agent(MINIMAX, max_depth=3)), None,
                                None) == EUNSUPPORTED
    assert lib.ewn_step_k_agent(C.byref(c), C.byref(fake), 4, C.byref(agent(7)), None, None) == EINVAL
    # the minimax side searches from the table image: ewn_state.tables is required there (not for MCTS against RandomAgent / MCTS)
    assert lib.ewn_step_k_agent(C.byref(c), C.byref(fake), 4, C.byref(agent(MINIMAX, max_depth=3)), None, None) == ENULL
    assert lib.ewn_step_k_agent(C.byref(cfg(opponent_kind=OPP["minimax"])), C.byref(fake), 4, C.byref(a), None, None) == ENULL


def test_predict_mcts_refuses_what_the_plan_refuses():
    """cube_layer < 3 is refused by the per-step MCTS agent too (EWN_EUNSUPPORTED): no cell falls back to a path that exists"""
    lib = _lib.load()
    assert lib.ewn_predict_mcts(5, 2, 0, None, None, 10, 5, 0, None, None, None, None) == EUNSUPPORTED
    assert lib.ewn_predict_mcts(5, 3, 0, None, None, 10, 5, 0, None, None, None, None) == OK


def test_step_k_answers_are_unchanged():
    """ewn_step_k keeps every answer: the minimax agent against MCTS stays unserved there, and agent kind 4 stays invalid"""
    lib = _lib.load()
    sk = lambda c, k, d: lib.ewn_step_k_supported(C.byref(c), k, d)  # noqa: E731
    assert sk(cfg(rng_kind=1), MINIMAX, 3) == 0
    assert sk(cfg(rng_kind=1), 0, 0) == 1 and sk(cfg(rng_kind=1), SAMPLE, 0) == 1
    assert sk(cfg(rng_kind=1), MCTS, 0) == EINVAL
    assert sk(cfg(opponent_kind=0, rng_kind=1), MCTS, 0) == EINVAL
    assert lib.ewn_lanes_per_game(C.byref(cfg(rng_kind=1)), 0) == 0
