"""The per-lane search of the slot-task K-step kernel against the CPU oracle where, at two lanes per game, the expectation's six
val6[] terms are read three per lane and added once, in dice order, on the even lane (the odd lane's three doubles cross over, the
sum comes back).  Every byte of every trajectory row and of the final state on a window of 300 lanes that ends on the last game,
at the smallest lane counts at which the launcher picks the kernel (65 537 games at two lanes per game, 131 073 at one).

The file was written for that lever together with fused leaf entries (a leaf's value read with its rank, 16 bytes per leaf, the
values of a cube's prefix minima taken as minima of the leaves' values).  The leaf entries passed every case here, measured no
gain beside the shared sum and are not in the tree (profiles/r10/README.md); the cases and the window's contents are the ones
chosen for both levers, so the leaves that steer to "no such reply" and to -10, the cuts and the empty-P2 leaves stay counted.

The cases: the 5x5 record layout at max_depth 3; max_depth 4 (the image's other value variant); 'min_dist' and 'attk' (other val[]
and val6[] contents: integers, and a -10 that is not the lowest rank); one lane per game (no shared sum: the case pins the unchanged
path); 6x6 (the shared sum on 64-bit masks).

What a case's window has to contain is counted on the oracle alone, before any GPU run (`_events`, the reconstruction of
tests/test_gpu_rollout_search_levers.py: the position and the dice of every opponent decision rebuilt from the oracle's
observations and checked against what the oracle reports).  Per case, all of:
  * second_cube > 0: decisions whose dice cube is off the board with a cube on either side of it (the search's second call);
  * root_captures > 0: a root move of a searched cube lands on an agent cube;
  * two_roots > 0: decisions with at least two valid root moves (only the second root onwards has an alpha a reply can cut at);
  * off_board > 0: after a valid root move some agent cube still on the board has a direction that leaves it (leaf entry 0);
  * to_origin > 0: after a valid root move some agent cube stands one move from its goal corner (leaf entry 1, -10);
  * last_cube > 0: the opponent has ONE cube and some agent cube can move onto the square a root move takes it to (a leaf with an
    empty P2: the level table's guard byte, row 0 of the leaf table);
  * episodes > 300: more episodes ended inside the window than it has lanes."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_rollout import _rollout_vs_oracle  # noqa: E402
from tests.test_gpu_rollout_search_levers import _philox_dice  # noqa: E402

N2, N1, W = 65537, 131073, 300      # games at two lanes per game / at one; lanes checked
STEPS = ((0, 1), (1, 0), (1, 1))

MM = dict(opponent_policy="minimax", rng="philox", layout="record")

# id -> (games, K, launches, arguments); keys and launch counts chosen on the oracle (test_window_holds_what_the_case_needs)
CASES = {
    "default-record": (N2, 24, 2, dict(MM, max_depth=3, philox_key=909)),
    "max_depth=4": (N2, 24, 2, dict(MM, max_depth=4, philox_key=94)),
    "min_dist": (N2, 24, 2, dict(MM, max_depth=3, heuristic="min_dist", philox_key=91)),
    "attk": (N2, 24, 2, dict(MM, max_depth=3, heuristic="attk", philox_key=93)),
    "6x6": (N2, 24, 3, dict(MM, board_size=6, max_depth=3, philox_key=96)),
    "one-lane": (N1, 24, 2, dict(MM, max_depth=3, philox_key=911)),
}
NAMES = ("second_cube", "root_captures", "two_roots", "off_board", "to_origin", "last_cube", "episodes")


@functools.lru_cache(maxsize=None)
def _events(case):
    """the seven counts of the window's opponent decisions, on the oracle alone"""
    N, K, launches, kw = CASES[case]
    okw = dict(kw)
    okw.pop("layout")
    opp = okw.pop("opponent_policy")
    S, key = okw.get("board_size", 5), okw["philox_key"]
    lo = N - W
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)[lo:N]
    orc = po.OracleVecEnv(W, opponent=opp, autoreset=True, seed_stride=N, lane_offset=lo, **okw)
    ob, od = orc.reset(seeds=seeds)
    seed = seeds.astype(np.int64)
    n = dict.fromkeys(NAMES, 0)
    for _ in range(K * launches):
        acts = orc.random_actions()
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
                dests = [(mine[k][0] - dx, mine[k][1] - dy) for k in roots for dx, dy in STEPS]
                dests = [c for c in dests if c[0] >= 0 and c[1] >= 0]
                n["second_cube"] += len(roots) == 2
                n["root_captures"] += any(b[c] > 0 for c in dests)
                n["two_roots"] += len(dests) >= 2
                # the repliers of a root: the agent's cubes but the one the root move has captured
                theirs = [tuple(int(v) for v in c) for c in np.argwhere(b > 0)]
                left = [[c for c in theirs if c != r] for r in dests if r != (0, 0)]   # (a root onto the opponent's corner wins: no replies)
                n["off_board"] += any(c[0] == S - 1 or c[1] == S - 1 for cubes in left for c in cubes)
                n["to_origin"] += any(c in ((S - 1, S - 2), (S - 2, S - 1), (S - 2, S - 2)) for cubes in left for c in cubes)
                if len(mine) == 1:
                    n["last_cube"] += any(b[c[0] - dx, c[1] - dy] > 0 for c in dests for dx, dy in STEPS if c[0] - dx >= 0 and c[1] - dy >= 0)
            if te[i]:
                n["episodes"] += 1
                seed[i] += N    # the next episode's seed: one stride further
        ob, od = nb, nd
    return n


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_holds_what_the_case_needs(case):
    n = _events(case)
    print(case, " ".join("%s %d" % (k, n[k]) for k in NAMES))
    assert all(n[k] > 0 for k in NAMES[:-1]) and n["episodes"] > W, (case, n)


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
