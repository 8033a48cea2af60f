"""The host side of the model-opponent step calls (ewn_step_vs, ewn_step_k_vs) without a GPU: which configurations and agents they
serve and the codes for null / invalid arguments (nothing is launched on any of these paths)."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from ewn_gym_amd import _lib  # noqa: E402
from ewn_gym_amd._lib import AGENT, AGENT_MCTS, EwnConfig, EwnOpponentPolicy, EwnRolloutOut, EwnState, EwnStepOut  # noqa: E402

EWN_EINVAL, EWN_ENULL, EWN_EUNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def cfg(S=5, L=3, N=64, opp=0, depth=3, rng=1, shaped=0, autoreset=0, heur=0, sims=10, copies=5):
    return EwnConfig(S, L, N, opp, depth, heur, sims, copies, rng, shaped, 10, autoreset, 0, 0, N, 0, 1.0, -1.0, 0)


@pytest.mark.parametrize("S,want", [(5, 1), (7, 1), (6, 0), (8, 0)])
def test_supported_by_board(lib, S, want):
    for rng in (0, 1):
        assert lib.ewn_step_vs_supported(C.byref(cfg(S=S, rng=rng))) == want
        for agent in ("random", "sample", "minimax"):
            assert lib.ewn_step_k_vs_supported(C.byref(cfg(S=S, rng=rng)), AGENT[agent], 3) == want


def test_supported_matrix(lib):
    for shaped in (0, 1):
        for autoreset in (0, 1):
            for rng in (0, 1):
                want = 0 if (rng == 0 and autoreset) else 1            # MT19937-compat dice: one episode per lane only
                c = cfg(shaped=shaped, autoreset=autoreset, rng=rng)
                assert lib.ewn_step_vs_supported(C.byref(c)) == want, (shaped, autoreset, rng)
                assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["random"], 0) == want
                assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["minimax"], 5) == want
    assert lib.ewn_step_vs_supported(C.byref(cfg(L=2))) == 0
    assert lib.ewn_step_k_vs_supported(C.byref(cfg(L=2)), AGENT["random"], 0) == 0
    assert lib.ewn_step_vs_supported(C.byref(cfg(N=0))) == EWN_EINVAL
    assert lib.ewn_step_k_vs_supported(C.byref(cfg(rng=7)), AGENT["random"], 0) == EWN_EINVAL
    assert lib.ewn_step_vs_supported(None) == EWN_ENULL
    assert lib.ewn_step_k_vs_supported(None, AGENT["random"], 0) == EWN_ENULL


def test_agents(lib):
    c = cfg()
    for depth in range(1, 7):
        assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["minimax"], depth) == 1
    assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["minimax"], 0) == EWN_EINVAL
    assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["minimax"], 7) == 0
    assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT["mlp"], 0) == 0          # the model agent is ewn_step_k_selfplay's
    assert lib.ewn_step_k_vs_supported(C.byref(c), AGENT_MCTS, 0) == 0            # not built
    assert lib.ewn_step_k_vs_supported(C.byref(c), 5, 0) == EWN_EINVAL
    assert lib.ewn_step_k_vs_supported(C.byref(c), -1, 0) == EWN_EINVAL


def test_the_opponent_fields_of_cfg_are_not_read(lib):
    wild = cfg(opp=9, depth=-4, heur=77, sims=0, copies=-1)
    assert lib.ewn_step_vs_supported(C.byref(wild)) == 1
    assert lib.ewn_step_k_vs_supported(C.byref(wild), AGENT["minimax"], 4) == 1
    assert lib.ewn_rng_words(C.byref(wild)) == EWN_EINVAL
    assert lib.ewn_rng_words(C.byref(cfg(opp=3))) == EWN_EINVAL            # no fourth opponent kind in ewn_config
    assert lib.ewn_abi_version() == 4


def test_null_and_invalid_arguments(lib):
    """every pointer below is a small host address no kernel may ever see: a launch would fault, a code comes back instead"""
    c = cfg()
    st = EwnState(8, 8, 8, 8, None, None, 8)
    opp = EwnOpponentPolicy(8, 1, 0, None)
    so = EwnStepOut(8, 8, 8, 8, None, None, None)
    ro = EwnRolloutOut()
    sv, sk = lib.ewn_step_vs, lib.ewn_step_k_vs
    assert sv(None, C.byref(st), 8, C.byref(opp), C.byref(so), None) == EWN_ENULL
    assert sv(C.byref(c), None, 8, C.byref(opp), C.byref(so), None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(st), None, C.byref(opp), C.byref(so), None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(st), 8, None, C.byref(so), None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(st), 8, C.byref(EwnOpponentPolicy()), C.byref(so), None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(st), 8, C.byref(opp), None, None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(st), 8, C.byref(opp), C.byref(EwnStepOut(8, 8, 8, None, None, None, None)), None) == EWN_ENULL
    assert sv(C.byref(c), C.byref(EwnState(8, 8, 8, 8, None, None, None)), 8, C.byref(opp), C.byref(so), None) == EWN_ENULL   # tables
    assert sv(C.byref(cfg(shaped=1)), C.byref(st), 8, C.byref(opp), C.byref(so), None) == EWN_ENULL                          # prev_score / tolerance
    assert sv(C.byref(c), C.byref(st), 8, C.byref(opp), C.byref(EwnStepOut(8, 8, 8, 8, None, None, 8)), None) == EWN_EINVAL  # random_action
    assert sv(C.byref(cfg(rng=0, autoreset=1)), C.byref(st), 8, C.byref(opp), C.byref(so), None) == EWN_EUNSUPPORTED
    assert sv(C.byref(cfg(S=6)), C.byref(st), 8, C.byref(opp), C.byref(so), None) == EWN_EUNSUPPORTED
    assert sv(C.byref(cfg(N=0)), C.byref(st), 8, C.byref(opp), C.byref(so), None) == EWN_EINVAL
    R = AGENT["random"]
    assert sk(None, C.byref(st), 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(c), C.byref(st), 0, R, 0, C.byref(opp), C.byref(ro), None) == EWN_EINVAL
    assert sk(C.byref(c), None, 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(c), C.byref(st), 4, R, 0, None, C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(c), C.byref(st), 4, R, 0, C.byref(EwnOpponentPolicy()), C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(c), C.byref(EwnState(8, 8, 8, 8, None, None, None)), 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(cfg(shaped=1)), C.byref(st), 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_ENULL
    assert sk(C.byref(c), C.byref(st), 4, AGENT["minimax"], 0, C.byref(opp), C.byref(ro), None) == EWN_EINVAL
    assert sk(C.byref(c), C.byref(st), 4, AGENT["minimax"], 7, C.byref(opp), C.byref(ro), None) == EWN_EUNSUPPORTED
    assert sk(C.byref(c), C.byref(st), 4, AGENT["mlp"], 0, C.byref(opp), C.byref(ro), None) == EWN_EUNSUPPORTED
    assert sk(C.byref(c), C.byref(st), 4, AGENT_MCTS, 0, C.byref(opp), C.byref(ro), None) == EWN_EUNSUPPORTED
    assert sk(C.byref(c), C.byref(st), 4, 9, 0, C.byref(opp), C.byref(ro), None) == EWN_EINVAL
    assert sk(C.byref(cfg(rng=0, autoreset=1)), C.byref(st), 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_EUNSUPPORTED
    assert sk(C.byref(cfg(S=8)), C.byref(st), 4, R, 0, C.byref(opp), C.byref(ro), None) == EWN_EUNSUPPORTED
