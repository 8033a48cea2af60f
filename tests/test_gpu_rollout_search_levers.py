"""The per-lane search of the slot-task K-step kernel against the CPU oracle, where a game's two lanes SWAP their cube keys (one lane
permute per cube; each lane carries the nearest cube above and below for its own three dice only) instead of broadcasting them.
Every byte of every trajectory row and of the final state on a window of 300 lanes that ends on the last game, at the smallest
lane counts at which the launcher picks the kernel (65 537 games at two lanes per game, 131 073 at one).

What a case's window has to contain is counted on the oracle alone, before any GPU run (`_window_events`): the position and the
dice of every opponent decision are rebuilt from the oracle's observations -- the agent's move applied to the board it saw, the
opponent's dice taken from the lane's Philox stream -- and the rebuilt stream is checked against the dice the oracle reports after
the step.  A case asserts, in this order:
  * second_cube > 0: opponent decisions whose dice cube is off the board with a cube on either side of it (the search's second call);
  * root_captures > 0: decisions in which a root move of a searched cube lands on an agent cube (a replier cube captured at the root);
  * last_cube > 0: decisions in which the opponent has ONE cube, and some agent cube can move onto the square a root move takes it
    to: a reply that captures the mover's last cube, the leaf with an empty P2 (the level table's guard byte);
  * episodes > 300: more episodes ended inside the window than it has lanes (every lane's auto-reset is exercised).
The 6x6 case runs the swap on 64-bit masks, the one-lane case the search without it (one lane holds all six keys)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_rollout import _rollout_vs_oracle  # noqa: E402

N2, N1, W = 65537, 131073, 300      # games at two lanes per game / at one; lanes checked

MM = dict(opponent_policy="minimax", rng="philox")

# id -> (games, K, launches, arguments); keys and launch counts chosen on the oracle (test_window_holds_what_the_case_needs)
CASES = {
    "default-record": (N2, 24, 2, dict(MM, layout="record", max_depth=3, philox_key=909)),
    "default-columns": (N2, 24, 2, dict(MM, layout="columns", max_depth=3, philox_key=910)),
    "max_depth=4": (N2, 16, 2, dict(MM, layout="record", max_depth=4, philox_key=94)),
    "min_dist": (N2, 24, 2, dict(MM, layout="record", max_depth=3, heuristic="min_dist", philox_key=91)),
    "attk": (N2, 24, 2, dict(MM, layout="record", max_depth=3, heuristic="attk", philox_key=93)),
    "sample-agent": (N2, 24, 3, dict(MM, agent="sample", layout="record", max_depth=3, philox_key=914)),
    "6x6": (N2, 24, 3, dict(MM, layout="record", board_size=6, max_depth=3, philox_key=96)),
    "one-lane": (N1, 24, 2, dict(MM, layout="record", max_depth=3, philox_key=911)),
}


def _philox_dice(block, seed, key):
    """the draws of one env step: word 0 of the step's Philox block is the opponent's dice, the next one the dice the agent sees
    (Lemire's bounded draw: a word whose low product half is below 2^32 mod 6 = 4 is drawn again)"""
    out = po.philox([block, seed, 0, 0x454E5631], [key & 0xFFFFFFFF, key >> 32])
    dice = []
    for w in out:
        m = int(w) * 6
        if (m & 0xFFFFFFFF) >= 4:
            dice.append(1 + (m >> 32))
    return dice


def _window_events(N, K, launches, agent="random", **kw):
    """(second_cube, root_captures, last_cube, episodes) of the window's opponent decisions, on the oracle alone"""
    okw = dict(kw)
    okw.pop("layout", None)
    opp = okw.pop("opponent_policy")
    S, key = okw.get("board_size", 5), okw.get("philox_key", 0)
    lo, hi = N - W, N
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)[lo:hi]
    orc = po.OracleVecEnv(W, opponent=opp, autoreset=True, seed_stride=N, lane_offset=lo, **okw)
    ob, od = orc.reset(seeds=seeds)
    seed = seeds.astype(np.int64)
    second = captures = last = episodes = 0
    for _ in range(K * launches):
        acts = orc.random_actions() if agent == "random" else orc.sample_actions()
        draws = orc.aux()[2]
        _, _, cs, cl, _ = po.legal_actions(ob, od, player=1)
        nb, nd, _, te, _, info = orc.step(acts)
        for i in range(W):
            b = ob[i].astype(int)
            flag, d = int(acts[i, 0]), int(acts[i, 1])
            cube = int(cl[i] if flag == 1 else cs[i])
            (x, y), = np.argwhere(b == cube)
            nx, ny = x + (d in (1, 2)), y + (d in (0, 2))
            decided = 0 <= d <= 2 and nx < S and ny < S
            if decided:
                b[x, y] = 0
                b[nx, ny] = cube
                decided = (nx, ny) != (S - 1, S - 1) and (b < 0).any()   # the agent has not won
            assert decided == (int(info[i]) not in (1, 2)), "the rebuilt agent move disagrees with the oracle"
            if decided:
                dice = _philox_dice((int(draws[i]) + 3) >> 2, int(seed[i]) & 0xFFFFFFFF, key)
                if not te[i]:
                    assert dice[1] == nd[i], "the rebuilt dice stream disagrees with the oracle"
                mine = {-int(v): tuple(int(c) for c in np.argwhere(b == v)[0]) for v in np.unique(b) if v < 0}
                roots = [dice[0]] if dice[0] in mine else [k for k in sorted(mine) if k > dice[0]][:1] + [k for k in sorted(mine, reverse=True) if k < dice[0]][:1]
                second += len(roots) == 2
                dests = [(mine[k][0] - dx, mine[k][1] - dy) for k in roots for dx, dy in ((0, 1), (1, 0), (1, 1))]
                dests = [c for c in dests if c[0] >= 0 and c[1] >= 0]
                captures += any(b[c] > 0 for c in dests)
                if len(mine) == 1:
                    last += any(b[c[0] - dx, c[1] - dy] > 0 for c in dests for dx, dy in ((0, 1), (1, 0), (1, 1)) if c[0] - dx >= 0 and c[1] - dy >= 0)
            if te[i]:
                episodes += 1
                seed[i] += N    # the next episode's seed: one stride further
        ob, od = nb, nd
    return second, captures, last, episodes


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_holds_what_the_case_needs(case):
    N, K, launches, kw = CASES[case]
    second, captures, last, episodes = _window_events(N, K, launches, **kw)
    print(case, "second_cube", second, "root_captures", captures, "last_cube", last, "episodes", episodes)
    assert second > 0 and captures > 0 and last > 0 and episodes > W, (case, second, captures, last, episodes)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_on_the_last_lanes(ea, case):
    N, K, launches, kw = CASES[case]
    n = _rollout_vs_oracle(ea, N, N - W, N, K, launches, **kw)
    assert n > W, (case, n)
