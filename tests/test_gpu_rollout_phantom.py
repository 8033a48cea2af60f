"""The slot-task rollout kernel on 5x5 and 6x6 at max_depth 1-4, whose search finds "no such reply" and "reply onto the origin" in
the tables (phantom cells, ewn_gym_amd/csrc/ewn_movetab.hpp): transition for transition against the CPU oracle, from the start
position and from positions constructed so that both exceptions -- and the two cases next to them -- are in the first search."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402

SLOT_N = 66000     # two lanes per game x 66 000 games >= 131 072 lanes: the launcher picks k_rollout_slots
ONE_LANE_N = 140000  # one lane per game
M_POS = 256


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def cpu(t):
    return t.detach().cpu().numpy()


def _rollout_vs_oracle(ea, N, lo, n, K, launches, S, max_depth, pos=None, key=0):
    """record layout, the random agent, auto-reset; pos = (boards, dice) of M_POS positions: lane l starts from position l mod M_POS.
    Returns the oracle's `terminated` of the first step."""
    kw = dict(board_size=S, max_depth=max_depth, rng="philox", philox_key=key, autoreset=True, seed_stride=N)
    env = ea.VecEWN(N, opponent_policy="minimax", **kw)
    assert env.supports_rollout("random", 3)
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)
    env.reset(seeds=seeds)
    orc = po.OracleVecEnv(n, opponent="minimax", lane_offset=lo, **kw)
    ob, od = orc.reset(seeds=seeds[lo:lo + n])
    if pos is not None:
        idx = np.arange(N) % M_POS
        env.set_obs(pos[0][idx], pos[1][idx])
        orc.set_obs(pos[0][idx[lo:lo + n]], pos[1][idx[lo:lo + n]])
    traj = env.alloc_rollout(K, layout="record")
    totals = env.alloc_totals()
    ret, nst, nep, nwin = np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    first_te = None
    for launch in range(launches):
        env.rollout(K, agent="random", traj=traj, totals=totals)
        tj = {k: cpu(v[:, lo:lo + n]) for k, v in traj.items()}
        for k in range(K):
            ctx = (S, max_depth, launch, k)
            acts = orc.random_actions()
            assert np.array_equal(tj["action"][k], acts), ctx
            ob, od, r, te, tr, info = orc.step(acts)
            first_te = te.copy() if first_te is None else first_te
            assert np.array_equal(tj["board"][k], ob) and np.array_equal(tj["dice"][k], od), ctx
            assert np.array_equal(bits(tj["reward"][k]), bits(r)), ctx
            assert np.array_equal(tj["terminated"][k], te) and np.array_equal(tj["truncated"][k], tr) and np.array_equal(tj["info"][k], info), ctx
            ret += r; nst += 1; nep += te != 0; nwin += info == 2
        assert np.array_equal(cpu(env.board[lo:lo + n]), ob) and np.array_equal(cpu(env.dice[lo:lo + n]), od), (S, max_depth, launch)
    assert np.array_equal(bits(cpu(totals["return_sum"][lo:lo + n])), bits(ret))
    assert np.array_equal(cpu(totals["n_steps"][lo:lo + n]), nst) and np.array_equal(cpu(totals["n_episodes"][lo:lo + n]), nep)
    assert np.array_equal(cpu(totals["n_wins"][lo:lo + n]), nwin)
    return first_te


@pytest.mark.parametrize("S", [5, 6])
@pytest.mark.parametrize("max_depth", [3, 4])
def test_slot_kernel_two_lanes_per_game(ea, S, max_depth):
    _rollout_vs_oracle(ea, SLOT_N, 40192, 256, 7, 3, S, max_depth, key=1200 + max_depth)


@pytest.mark.parametrize("S,max_depth", [(5, 3), (6, 4)])
def test_slot_kernel_one_lane_per_game(ea, S, max_depth):
    _rollout_vs_oracle(ea, ONE_LANE_N, 139520, 256, 7, 3, S, max_depth, key=1300 + max_depth)


# ---------------------------------------------------------------- constructed positions
#
# Real coordinates: the agent's cubes are the positive numbers and run to (S-1, S-1); the opponent's are the negative ones and run to
# (0, 0).  In the opponent's search the agent is the replier and its goal corner is the search's "origin".  The four cases are
# properties of the position the search sees, that is AFTER the agent's move, which the oracle does not hand out; each is therefore
# built so that no single agent move which leaves the game going (it moves one cube and captures at most one) can undo it:
#   edge:    three or more agent cubes on the bottom row or the right column (one of their directions leaves the board);
#   origin:  two or more agent cubes on the three squares next to (S-1, S-1): a cube that moves from there stays next to the corner
#            or enters it (the game ends), a cube that captures one of them stands there itself;
#   off:     at most five agent cubes;
#   capture: the opponent has ONE cube (every dice selects it), and two or more agent cubes stand on squares it moves to: the agent
#            taking that one cube ends the game.
# A lane counts for a case if its first step does not end the game (the search ran on a position that still has the property).

def _flags(b):
    S = b.shape[-1]
    ag, op = b > 0, b < 0
    edge = (ag[:, S - 1, :].sum(1) + ag[:, :S - 1, S - 1].sum(1)) >= 3
    origin = (ag[:, S - 1, S - 2].astype(int) + ag[:, S - 2, S - 1] + ag[:, S - 2, S - 2]) >= 2
    off = ag.reshape(len(b), -1).sum(1) <= 5
    capture = np.zeros(len(b), bool)
    for i in np.flatnonzero(op.reshape(len(b), -1).sum(1) == 1):
        r, c = np.argwhere(op[i])[0]
        t = [(r - 1, c), (r, c - 1), (r - 1, c - 1)]
        capture[i] = sum(bool(ag[i, y, x]) for y, x in t if y >= 0 and x >= 0) >= 2
    return dict(edge=edge, origin=origin, off=off, capture=capture)


def constructed(S):
    rng = np.random.default_rng(100 + S)
    boards = np.zeros((M_POS, S, S), np.int8)
    for i in range(M_POS):
        b = boards[i]
        free = [(y, x) for y in range(S) for x in range(S) if (y, x) not in ((0, 0), (S - 1, S - 1))]
        ag_cells, n_op = [], 1 + int(rng.integers(6))
        kind = i % 4
        if kind in (0, 2):    # around the agent's goal corner and along the two far edges
            ag_cells += [(S - 1, S - 2), (S - 2, S - 1), (S - 2, S - 2)][:2 + int(rng.integers(2))]
            ag_cells += [(S - 1, int(rng.integers(S - 2))), (int(rng.integers(S - 2)), S - 1)]
        if kind in (1, 2):    # a single opponent cube with agent cubes in front of it
            n_op = 1
            cand = [(y, x) for y in range(1, S) for x in range(1, S) if (y, x) != (S - 1, S - 1)
                    and not {(y - 1, x), (y, x - 1), (y - 1, x - 1)} & set(ag_cells) and (y, x) not in ag_cells]
            oy, ox = cand[int(rng.integers(len(cand)))]
            t = [(oy - 1, ox), (oy, ox - 1), (oy - 1, ox - 1)]
            t = [c for c in t if c != (0, 0)]
            ag_cells += [t[j] for j in rng.permutation(len(t))[:2 + int(rng.integers(2))]]
            b[oy, ox] = -(1 + int(rng.integers(6)))
            free.remove((oy, ox))
            n_op = 0
        ag_cells = list(dict.fromkeys(ag_cells))[:6]
        n_ag = max(len(ag_cells), int(rng.integers(2, 7))) if kind != 3 else int(rng.integers(1, 7))
        free = [c for c in free if c not in ag_cells]
        rest = [free[j] for j in rng.permutation(len(free))]
        fill = n_ag - len(ag_cells)
        ag_cells += rest[:fill]
        rest = rest[fill:]
        for num, (y, x) in zip(rng.permutation(6)[:len(ag_cells)] + 1, ag_cells):
            b[y, x] = num
        for num, (y, x) in zip(rng.permutation(6)[:n_op] + 1, rest):
            b[y, x] = -num
    dice = rng.integers(1, 7, M_POS).astype(np.int8)
    return boards, dice


@pytest.mark.parametrize("S,max_depth", [(5, 3), (6, 3), (5, 4)])
def test_slot_kernel_from_positions_with_both_exceptions(ea, S, max_depth):
    pos = constructed(S)
    b = pos[0]
    assert ((b > 0).reshape(M_POS, -1).sum(1) >= 1).all() and ((b < 0).reshape(M_POS, -1).sum(1) >= 1).all()
    for side in (b, -b):
        for i in range(M_POS):
            v = side[i][side[i] > 0]
            assert len(set(v.tolist())) == len(v) and (v <= 6).all()
    lo = 30208                     # a multiple of M_POS: lane lo + j starts from position j
    first_te = _rollout_vs_oracle(ea, SLOT_N, lo, M_POS, 7, 3, S, max_depth, pos=pos, key=1400 + S)
    # from the oracle alone: every case is among the positions whose first step went through the search and on
    went_on = first_te == 0
    f = _flags(b)
    n = {k: int((v & went_on).sum()) for k, v in f.items()}
    assert all(v >= 1 for v in n.values()), n
    assert int((f["edge"] & f["origin"] & f["off"] & went_on).sum()) >= 1, "both exceptions and an absent cube in one search"
