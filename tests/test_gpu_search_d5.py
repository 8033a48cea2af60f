"""The max_depth 5 / 6 closed-form search (d5c_search / d5c_reply_value, ewn_gym_amd/csrc/ewn_search_d5.hpp) on CONSTRUCTED positions,
against the CPU oracle, bit for bit and with no position or lane left out: the stateless predict (one lane per position), ewn_step
(two lanes per game, and one lane per game at the smallest lane count that picks it), ewn_step_k with the random agent (lock-step and
slot-task kernels, one and two lanes per game, Philox and MT19937 dice) and minimax(5 / 6) as the AGENT of ewn_step_k.

The positions are make_positions() of tests/test_gpu_search_keys.py, 1 024 per board size: two thirds random oracle play, one third
thinned to 1-3 cubes a side, dice redrawn.  Every special case of the closed form depends on which cube numbers are still on the
board; the Python model of tests/test_d5_closed_form_model.py (checked here against the oracle on every one of the positions) counts
the cases it meets, and the CPU test asserts that each of CASES occurs at every board size.

Which kernel a lane count runs: ewn_lanes_per_game(cfg, 0) for ewn_step, (cfg, 1) for ewn_step_k -- asserted per test; ewn_step_k
runs the slot-task kernel once lanes-per-game x games >= 131 072 and the lock-step kernel below that (ewn_rollout_tu.inc).

The 'two_min_dist' image keeps the reference's loops at max_depth 5 / 6 (d5_search, ewn_step_d3.hpp) and gets the same positions."""
import ctypes as C

import numpy as np
import pytest

from ewn_gym_amd import _lib
from oracle import pyoracle as po
from tests.test_d5_closed_form_model import CASES, d5_closed_form
from tests.test_gpu_search_keys import _bits, _cpu, _pair, ea, make_positions  # noqa: F401  (ea: the module's GPU fixture)

M_POS = 1024
SIZES = [5, 6, 7, 8]
_POS = {}


def positions(S):
    """the constructed positions of one board size, made once; nobody writes to them"""
    if S not in _POS:
        _POS[S] = make_positions(S, M_POS)
    return _POS[S]


# ---------------------------------------------------------------- CPU: what the positions contain

@pytest.mark.parametrize("S", SIZES)
def test_positions_cover_every_case_of_the_closed_form(S):
    """depth 5 on all 1 024 positions, depth 6 on the thinned third: the model equals the oracle's action and value bits on every
    one, and every case of CASES is among them (at depth 5 alone)"""
    b, d = positions(S)
    assert ((b > 0).sum(axis=(1, 2)) >= 1).all() and ((b < 0).sum(axis=(1, 2)) >= 1).all()
    assert (b[:, S - 1, S - 1] <= 0).all() and (b[:, 0, 0] >= 0).all(), "a won position among the inputs"
    thin = 2 * M_POS // 3
    assert ((b[thin:] > 0).sum(axis=(1, 2)) <= 3).all() and ((b[thin:] < 0).sum(axis=(1, 2)) <= 3).all()
    for depth, lo in ((5, 0), (6, thin)):
        oa, ov, _ = po.predict_minimax(b[lo:], d[lo:], depth, "hybrid")
        seen = dict.fromkeys(CASES, 0)
        for i in range(lo, M_POS):
            a, v = d5_closed_form(b[i], int(d[i]), depth, seen)
            assert a == (int(oa[i - lo][0]), int(oa[i - lo][1])), (depth, i, b[i], d[i])
            assert np.float64(v).tobytes() == np.float64(ov[i - lo]).tobytes(), (depth, i, v, ov[i - lo])
        print("S=%d depth=%d positions=%d seen=%s" % (S, depth, M_POS - lo, seen))
        if depth == 5:
            assert all(seen[c] > 0 for c in CASES), [c for c in CASES if seen[c] == 0]


def _cfg(S, depth, heur, rng, n, autoreset=True):
    return _lib.EwnConfig(board_size=S, cube_layer=3, n_lanes=n, opponent_kind=_lib.OPP["minimax"], max_depth=depth,
                          heuristic=_lib.HEUR[heur], num_simulations=10, num_env_copies=5, rng_kind=_lib.RNG[rng], shaped=0,
                          illegal_move_tolerance=10, autoreset=int(autoreset), shaped_refresh_on_reset=0, lane_offset=0, seed_stride=n,
                          mt_window=0, reward=1.0, illegal_move_reward=-1.0, philox_key=0)


def smallest_one_lane_count(S, depth, entry):
    """the smallest number of games at which ewn_step (entry 0) / ewn_step_k (entry 1) plays a max_depth 5 / 6 opponent on Philox
    dice with ONE lane per game: asked of the library, not written down here"""
    lanes = lambda n: _lib.load().ewn_lanes_per_game(C.byref(_cfg(S, depth, "hybrid", "philox", n)), entry)  # noqa: E731
    lo, hi = 1, 1 << 22
    assert lanes(lo) == 2 and lanes(hi) == 1
    while hi - lo > 1:      # two lanes per game below a threshold, one from it on
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if lanes(mid) == 1 else (mid, hi)
    assert lanes(hi) == 1 and lanes(hi - 1) == 2
    return hi


def test_one_lane_per_game_starts_at_a_size_the_tests_can_run():
    """the GPU tests below run ewn_step and ewn_step_k once at the smallest one-lane-per-game size: it exists and is of a size a
    test can allocate (today 131 072 games for ewn_step, 131 073 for ewn_step_k)"""
    for depth in (5, 6):
        for entry in (0, 1):
            n = smallest_one_lane_count(5, depth, entry)
            print("depth %d entry %d: one lane per game from %d games" % (depth, entry, n))
            assert 65536 < n <= 1 << 18


# ---------------------------------------------------------------- GPU

_ORACLE = {}


def oracle_predict(S, depth, heur):
    """the oracle's (actions, values) on positions(S): computed once per (size, depth, heuristic)"""
    k = (S, depth, heur)
    if k not in _ORACLE:
        b, d = positions(S)
        _ORACLE[k] = po.predict_minimax(b, d, depth, heur)[:2]
    return _ORACLE[k]


def _lanes(env, entry):
    return env.lib.ewn_lanes_per_game(C.byref(env.cfg), entry)


@pytest.mark.gpu
@pytest.mark.parametrize("heur", ["hybrid", "min_dist", "attk"])
@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("S", SIZES)
def test_predict_closed_form(ea, S, depth, heur):
    """stateless predict, max_depth 5 / 6 -> d5c_search<S, 1>, one lane per position: action and root-value bits on every position"""
    b, d = positions(S)
    oa, ov = oracle_predict(S, depth, heur)
    acts, vals = ea.predict_minimax(b, d, depth, heur)
    bad = np.flatnonzero((_cpu(acts) != oa).any(axis=1) | (_bits(_cpu(vals)) != _bits(ov)))
    assert bad.size == 0, (S, depth, heur, bad.size, bad[:5].tolist(), b[bad[:1]], d[bad[:1]])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("S", SIZES)
def test_predict_two_min_dist_loops(ea, S, depth):
    """'two_min_dist' at max_depth 5 / 6: the looped d5_search (ewn_step_d3.hpp), kept for this image alone, on the same positions"""
    b, d = positions(S)
    oa, ov = oracle_predict(S, depth, "two_min_dist")
    acts, vals = ea.predict_minimax(b, d, depth, "two_min_dist")
    bad = np.flatnonzero((_cpu(acts) != oa).any(axis=1) | (_bits(_cpu(vals)) != _bits(ov)))
    assert bad.size == 0, (S, depth, bad.size, bad[:5].tolist(), b[bad[:1]], d[bad[:1]])


# Regression: d5_search took the table's LARGEST rank for a won leaf's +10.  On the 'two_min_dist' image the leaf values are differences
# of distance sums, -2(S-1) .. 2(S-1) - 1, which reach +11 on 7x7 and +13 on 8x8: every leaf that wins was then worth 11 / 13, and 118
# of the 1 024 constructed 7x7 positions came back with a wrong root value (5x5 and 6x6 stay below +10 and were right).  In this
# position the only root move (cube 5 down, taking -3) wins at every leaf: the root value is exactly +10.
WON_LEAVES_7X7 = (np.array([[0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, -6, 0],
                            [0, -4, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 0, 0, 5],
                            [0, 0, 0, 0, 0, 0, -3],
                            [0, 0, 0, 0, 0, 0, 0]], np.int8), 2)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 6])
def test_two_min_dist_won_leaves_are_worth_ten_on_7x7(ea, depth):
    b, d = WON_LEAVES_7X7[0][None], np.array([WON_LEAVES_7X7[1]], np.int8)
    oa, ov, _ = po.predict_minimax(b, d, depth, "two_min_dist")
    assert ov[0] == 10.0 and tuple(oa[0]) == (1, 1)
    acts, vals = ea.predict_minimax(b, d, depth, "two_min_dist")
    assert np.array_equal(_cpu(acts), oa) and np.array_equal(_bits(_cpu(vals)), _bits(ov)), (_cpu(acts), _cpu(vals))


def _one_step(ea, N, lo, n, S, depth, lanes_per_game, heur="hybrid"):
    env, orc = _pair(ea, N, lo, lo + n, S, heur, 71, autoreset=False, max_depth=depth, pos=positions(S))
    assert _lanes(env, 0) == lanes_per_game
    acts = env.sample_legal_actions(0)
    oacts = orc.sample_legal_actions(0)
    assert np.array_equal(_cpu(acts[lo:lo + n]), oacts)
    ob, od, r, te, tr, info = orc.step(oacts)
    gb, gd, gr, gte, gtr, ginfo = [_cpu(x[lo:lo + n]) for x in env.step(acts)]
    assert np.array_equal(gb, ob) and np.array_equal(gd, od)
    assert np.array_equal(_bits(gr), _bits(r))
    assert np.array_equal(gte != 0, te != 0) and np.array_equal(gtr != 0, tr != 0) and np.array_equal(ginfo, info)
    assert (te == 0).sum() > n // 2      # most games went on: the reply was searched, not skipped


@pytest.mark.gpu
@pytest.mark.parametrize("S,depth", [(5, 5), (7, 5), (8, 5), (5, 6)])
def test_one_step_two_lanes_per_game(ea, S, depth):
    """ewn_step (k_step_d3 -> d5c_search<S, 2>): a legal agent move, then the opponent's depth-5 / 6 reply, from every position"""
    _one_step(ea, M_POS, 0, M_POS, S, depth, 2)


@pytest.mark.gpu
def test_one_step_two_min_dist_7x7(ea):
    """ewn_step on the 'two_min_dist' image (k_step_d3 -> d5_search<7, 2, true>, the six dice of the inner chance node over two lanes)"""
    _one_step(ea, M_POS, 0, M_POS, 7, 5, 2, heur="two_min_dist")


@pytest.mark.gpu
def test_one_step_one_lane_per_game(ea):
    """ewn_step at the smallest lane count that runs d5c_search<S, 1> inside the step kernel; the oracle replays 1 024 lanes from
    the middle of the batch"""
    N = smallest_one_lane_count(5, 5, 0)
    _one_step(ea, N, 70001, M_POS, 5, 5, 1)


def _k_steps(ea, N, lo, n, S, depth, rng, layout, lanes_per_game, slot_task, K=3, heur="hybrid"):
    """ewn_step_k, the random agent, K steps in one launch, step for step against the oracle from the constructed positions.
    Philox dice with auto-reset (a finished game restarts inside the launch); MT19937 dice without (a finished lane freezes)"""
    autoreset = rng == "philox"
    env, orc = _pair(ea, N, lo, lo + n, S, heur, 72, autoreset=autoreset, max_depth=depth, rng=rng, pos=positions(S))
    assert env.supports_rollout("random", 3)
    assert _lanes(env, 1) == lanes_per_game
    assert (N * lanes_per_game >= 131072) == slot_task       # the launcher's rule (ewn_rollout_tu.inc)
    traj = env.alloc_rollout(K, board=True, layout=layout)
    env.rollout(K, agent="random", traj=traj)
    tj = {k: _cpu(v[:, lo:lo + n]) for k, v in traj.items()}
    frozen = np.zeros(n, bool)
    for k in range(K):
        acts = orc.random_actions()
        live = ~frozen
        assert np.array_equal(tj["action"][k][live], acts[live]), k
        ob, od, r, te, tr, info = orc.step(np.where(live[:, None], acts, 0).astype(np.int8))
        assert np.array_equal(tj["board"][k], ob) and np.array_equal(tj["dice"][k], od), k
        assert np.array_equal(_bits(tj["reward"][k]), _bits(r)), k
        assert np.array_equal(tj["terminated"][k], te) and np.array_equal(tj["truncated"][k], tr) and np.array_equal(tj["info"][k], info), k
        if not autoreset:
            frozen |= te != 0
    assert np.array_equal(_cpu(env.board[lo:lo + n]), ob) and np.array_equal(_cpu(env.dice[lo:lo + n]), od)
    assert np.array_equal(_cpu(env.done[lo:lo + n]) != 0, frozen)


@pytest.mark.gpu
@pytest.mark.parametrize("S,depth,N,lo,n", [
    (5, 5, 257, 0, 257), (7, 5, 257, 0, 257), (8, 5, 257, 0, 257), (5, 5, 4099, 3000, 1024), (5, 6, 257, 0, 257),
], ids=lambda v: str(v))
def test_three_steps_lockstep_philox(ea, S, depth, N, lo, n):
    """k_rollout_d3<S, 2, 2, philox>: two lanes per game, lane counts that are no multiple of a block"""
    _k_steps(ea, N, lo, n, S, depth, "philox", "columns", 2, False)


@pytest.mark.gpu
def test_three_steps_two_min_dist_7x7(ea):
    """k_rollout_d3<7, 1, 2, philox, H2>: the looped d5_search inside the lock-step K-step kernel, one lane per game at every size"""
    _k_steps(ea, 257, 0, 257, 7, 5, "philox", "columns", 1, False, heur="two_min_dist")


@pytest.mark.gpu
@pytest.mark.parametrize("S,depth,n", [(5, 5, 1024), (7, 5, 1024), (8, 5, 1024), (5, 6, 512)], ids=lambda v: str(v))
def test_three_steps_slot_task_philox(ea, S, depth, n):
    """k_rollout_slots<S, 2, 2, philox> at its smallest size, trajectory as records; a slice that does not start at lane 0"""
    _k_steps(ea, 65536, 40001, n, S, depth, "philox", "record", 2, True)


@pytest.mark.gpu
def test_three_steps_slot_task_one_lane_per_game(ea):
    """k_rollout_slots<S, 1, 2, philox>: the smallest lane count at which ewn_step_k plays max_depth 5 with one lane per game"""
    N = smallest_one_lane_count(5, 5, 1)
    _k_steps(ea, N, N - 1024, 1024, 5, 5, "philox", "record", 1, True)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7, 8])
def test_three_steps_lockstep_mt19937(ea, S):
    """k_rollout_d3<S, 2, 2, mt19937>, without auto-reset (the evaluation shape)"""
    _k_steps(ea, 257, 0, 257, S, 5, "mt19937", "columns", 2, False)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7, 8])
def test_three_steps_slot_task_mt19937(ea, S):
    """k_rollout_slots<S, 2, 2, mt19937>, without auto-reset"""
    _k_steps(ea, 65536, 20001, 1024, S, 5, "mt19937", "record", 2, True)


@pytest.mark.gpu
@pytest.mark.parametrize("S,depth", [(5, 5), (7, 5), (5, 6)])
def test_minimax5_as_the_agent(ea, S, depth):
    """ewn_step_k with agent = minimax(5 / 6) against RandomAgent (k_rollout_d3<S, 2, 1, philox, AGENT = 2>): the recorded actions are
    the oracle's predict_minimax on the observation before them, the transitions the oracle's"""
    N, K = 257, 2
    env, orc = _pair(ea, N, 0, N, S, "hybrid", 73, max_depth=3, opponent="random", pos=positions(S))
    assert env.supports_rollout("minimax", depth)
    traj = env.alloc_rollout(K, board=True)
    env.rollout(K, agent="minimax", agent_max_depth=depth, traj=traj)
    tj = {k: _cpu(v) for k, v in traj.items()}
    ob, od = orc.obs()
    for k in range(K):
        acts = po.predict_minimax(ob, od, depth, "hybrid")[0]
        assert np.array_equal(tj["action"][k], acts), (k, np.flatnonzero((tj["action"][k] != acts).any(axis=1))[:5])
        ob, od, r, te, tr, info = orc.step(acts)
        assert np.array_equal(tj["board"][k], ob) and np.array_equal(tj["dice"][k], od), k
        assert np.array_equal(_bits(tj["reward"][k]), _bits(r)), k
        assert np.array_equal(tj["terminated"][k], te) and np.array_equal(tj["truncated"][k], tr) and np.array_equal(tj["info"][k], info), k
    assert np.array_equal(_cpu(env.board), ob) and np.array_equal(_cpu(env.dice), od)
