"""The slot-task rollout kernel's pair-shared work against the CPU oracle, step for step: the Philox block the two lanes of a game
compute together at step start, the opponent's move taken from the search's chosen root, the board-slot byte stores and the
auto-reset's record split between the two lanes.  Sizes are >= 65 536 games (the launcher's threshold for this kernel at two
lanes per game) and mostly not multiples of the block's 128 games, so the last block is partial."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_rollout import _rollout_vs_oracle  # noqa: E402

N_ODD = 65537     # one game in the last block
N_MID = 66000     # 80 games in the last block


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.mark.parametrize("N,lo", [(N_ODD, N_ODD - 257), (N_MID, 65700), (N_MID, 0)])
def test_pair_record_layout_bench_shape(ea, N, lo):
    """the benchmark's instance (record + reward, max_depth 3, Philox), three launches, the grid's partial last block included"""
    n = _rollout_vs_oracle(ea, N, lo, min(N, lo + 257), 20, 3, layout="record", opponent_policy="minimax", max_depth=3,
                           rng="philox", philox_key=4242)
    assert n > 257


@pytest.mark.parametrize("layout", ["record", "columns"])
def test_pair_autoreset_heavy(ea, layout):
    """action_space.sample() as the agent: about one game in ten ends per step on an illegal move and restarts (the auto-reset's
    slot record written by both lanes, a fresh Philox stream primed at the next step)"""
    n = _rollout_vs_oracle(ea, N_ODD, N_ODD - 300, N_ODD, 12, 3, agent="sample", layout=layout, opponent_policy="minimax", max_depth=3,
                           rng="philox", philox_key=17)
    assert n > 600


@pytest.mark.parametrize("layout", ["record", "columns"])
def test_pair_frozen_lanes(ea, layout):
    """no auto-reset: finished games freeze (their lanes skip the Philox block and the moves) and keep writing their rows"""
    _rollout_vs_oracle(ea, N_MID, 65600, N_MID, 15, 4, autoreset=False, layout=layout, opponent_policy="minimax", max_depth=3,
                       rng="philox", philox_key=23)


def test_pair_single_step_launches(ea):
    """K = 1: every launch starts and ends inside one env step of every game, eight launches in a row"""
    _rollout_vs_oracle(ea, N_ODD, N_ODD - 200, N_ODD, 1, 8, layout="record", opponent_policy="minimax", max_depth=3, rng="philox",
                       philox_key=31)


@pytest.mark.parametrize("kw", [dict(max_depth=1), dict(max_depth=2), dict(max_depth=4), dict(max_depth=3, board_size=6),
                                dict(max_depth=3, board_size=7), dict(max_depth=4, board_size=8)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_pair_search_depths_and_sizes(ea, kw):
    """the search's chosen root as the opponent's move in both search paths (max_depth 1-2: all six roots in one call; 3-4: one
    cube per call, carried to a second call), and record sizes of two to four 16-byte pieces"""
    _rollout_vs_oracle(ea, N_MID, 65800, N_MID, 9, 2, layout="record", opponent_policy="minimax", rng="philox",
                       philox_key=50 + kw["max_depth"], **kw)


def test_pair_one_lane_per_game(ea):
    """the same kernel at one lane per game (>= 131 072 games): the scalar Philox block and single-lane slot stores"""
    _rollout_vs_oracle(ea, 131075, 130800, 131075, 9, 2, layout="record", opponent_policy="minimax", max_depth=3, rng="philox",
                       philox_key=77)
