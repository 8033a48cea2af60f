"""The slot-task K-step kernel's step boundary and search entry against the CPU oracle: the `sel` lookups with cubes off the board
on either side, every outcome of a step (won, lost, illegal move, frozen lane), the trajectory record's meta bytes, the per-lane
search entry (first and second cube of a dice) and the loop head that ends a launch.
Every byte of every row on a window of at most 300 lanes, at the smallest lane counts at which the launcher picks the kernel
(65 537 games at two lanes per game, 131 073 at one: the window ends on the last game, in the grid's partial block)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_rollout import _rollout_vs_oracle, bits, cpu  # noqa: E402

N2, N1, W = 65537, 131073, 300      # games at two lanes per game / at one; lanes checked


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def test_record_rows_over_two_long_launches(ea):
    """K = 24 x 2: long enough for captures on both sides (cubes off the board in either alive mask) and for auto-resets"""
    n = _rollout_vs_oracle(ea, N2, N2 - W, N2, 24, 2, layout="record", opponent_policy="minimax", max_depth=3, rng="philox", philox_key=2024)
    assert n > W          # every lane of the window went through an auto-reset on average


def test_sample_agent_illegal_move_outcome(ea):
    """action_space.sample(): a draw that leaves the board ends the episode as (terminated, truncated, INVALID_PLAYER)"""
    n = _rollout_vs_oracle(ea, N2, 100, 100 + W, 12, 1, agent="sample", layout="record", opponent_policy="minimax", max_depth=3,
                           rng="philox", philox_key=314)
    assert n > W // 2


def test_frozen_lanes_without_autoreset(ea):
    """lanes freeze as their episode ends and go on writing (terminated, not truncated, no info) rows"""
    _rollout_vs_oracle(ea, N2, N2 - W, N2, 15, 3, autoreset=False, layout="record", opponent_policy="minimax", max_depth=3,
                       rng="philox", philox_key=15)


def test_columns_layout(ea):
    _rollout_vs_oracle(ea, N2, 30000, 30000 + W, 8, 1, layout="columns", opponent_policy="minimax", max_depth=3, rng="philox", philox_key=8)


def test_totals_without_a_trajectory(ea):
    """no trajectory at all (the kernel's totals-only instance): per-lane totals and the final state against the oracle's"""
    N, lo, hi, K = N2, N2 - W, N2, 20
    kw = dict(opponent_policy="minimax", max_depth=3, rng="philox", philox_key=20, autoreset=True, seed_stride=N)
    env = ea.VecEWN(N, **kw)
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)
    env.reset(seeds=seeds)
    okw = dict(kw)
    orc = po.OracleVecEnv(hi - lo, opponent=okw.pop("opponent_policy"), lane_offset=lo, **okw)
    ob, od = orc.reset(seeds=seeds[lo:hi])
    totals = env.alloc_totals()
    env.rollout(K, totals=totals)
    ret, nep, nwin = np.zeros(hi - lo), np.zeros(hi - lo, np.int64), np.zeros(hi - lo, np.int64)
    for k in range(K):
        ob, od, r, te, tr, info = orc.step(orc.random_actions())
        ret += r
        nep += te != 0
        nwin += info == 2
    assert np.array_equal(bits(cpu(totals["return_sum"][lo:hi])), bits(ret))
    assert np.array_equal(cpu(totals["n_steps"][lo:hi]), np.full(hi - lo, K))
    assert np.array_equal(cpu(totals["n_episodes"][lo:hi]), nep) and np.array_equal(cpu(totals["n_wins"][lo:hi]), nwin)
    assert np.array_equal(cpu(env.board[lo:hi]), ob) and np.array_equal(cpu(env.dice[lo:hi]), od)
    assert int(nep.sum()) > 0


@pytest.mark.parametrize("S", [7, 8])
def test_boards_with_64_bit_masks(ea, S):
    _rollout_vs_oracle(ea, N2, N2 - W, N2, 10, 1, layout="record", board_size=S, opponent_policy="minimax", max_depth=3, rng="philox",
                       philox_key=S)


def test_one_lane_per_game(ea):
    _rollout_vs_oracle(ea, N1, N1 - W, N1, 6, 1, layout="record", opponent_policy="minimax", max_depth=3, rng="philox", philox_key=6)


def test_one_step_launches(ea):
    _rollout_vs_oracle(ea, N2, N2 - W, N2, 1, 6, layout="record", opponent_policy="minimax", max_depth=3, rng="philox", philox_key=1)
