"""The depth-3 search's per-cube keys, cube selection and levels (d3_search, ewn_gym_amd/csrc/ewn_step_d3.hpp) on CONSTRUCTED positions,
against the CPU oracle: the stateless predict kernel (one lane per position), the one-step kernel (two lanes per game), the lock-step
K-step kernel and the slot-task K-step kernel (65 536 games: the smallest size at which the launcher picks it).

The positions are random oracle play from the benchmark's seeds plus few-cube endgames made by removing cubes from such positions.
A Python model of the search as the kernel states it (per replier cube three prefix minima and one key; per dice the pair F, G) is
first checked against the oracle bit for bit, and then says which situations the positions contain; the CPU test asserts that every
one the kernel treats on its own path is there:

 * a cube whose replies cut at the first, the second and the third reply, and one that does not cut;
 * the first root, searched while `best` is still -inf;
 * a replier cube that is off the board;
 * a root move that captures a replier cube, the one on the replier's highest ring cell included (the level then comes from the next);
 * a reply onto the origin, a reply that leaves the board;
 * the replier reduced to one cube, the mover's last cube captured by a reply;
 * a second root cube whose replies are cut by the first cube's best.

The table builder's check that no val6[] entry is -0.0 (the search starts a root's expectation from its first term) is exercised for
every image of every board size by building them."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.test_d5_closed_form_model import DIRS_N, DIRS_P, INF, dests, leaf_value, move, pair_for

M_POS = 2048        # positions per board size
CASES = ("cut_first", "cut_second", "cut_third", "no_cut", "first_root_minus_inf", "replier_cube_off_board", "root_captures_replier",
         "root_captures_replier_top", "reply_onto_origin", "reply_off_board", "replier_one_cube", "mover_last_cube_captured",
         "second_cube_cut_by_first")


def ring_key(q):
    return (min(q), q[0], q[1])     # ring order of ewn_fast.hpp: ascending min(row, col), then row-major


def d3_model(board, dice, seen):
    """(action, value) of ExpectiMinimaxAgent(max_depth=3, 'hybrid').predict the way d3_search computes it; counts its cases in `seen`"""
    S = board.shape[0]
    P = {int(v): (i, j) for (i, j), v in np.ndenumerate(board) if v > 0}
    N = {int(-v): (i, j) for (i, j), v in np.ndenumerate(board) if v < 0}
    if len(N) < 6:
        seen["replier_cube_off_board"] += 1
    best, action = -INF, (0, 0)
    F0, G0 = pair_for(P, dice)
    roots = [(F0, 1 if F0 > dice else 0)] + ([(G0, 0)] if G0 is not None else [])
    for slot, (cube, flag) in enumerate(roots):
        for d, q in enumerate(dests(P[cube], DIRS_P, S)):
            if q is None:
                continue
            if q in N.values():
                seen["root_captures_replier"] += 1
                if len(N) > 1 and q == max(N.values(), key=ring_key):
                    seen["root_captures_replier_top"] += 1
            P1, N1 = move(P, N, True, cube, q)
            if q == (S - 1, S - 1) or not N1:
                v = 10
            else:
                if best == -INF:
                    seen["first_root_minus_inf"] += 1
                if len(N1) == 1:
                    seen["replier_one_cube"] += 1
                key = {}        # replier cube -> (cuts?, value): the first prefix minimum <= best, else the minimum
                for k in N1:
                    pre, worst = [], INF
                    for q2 in dests(N1[k], DIRS_N, S):
                        if q2 is None:
                            seen["reply_off_board"] += 1
                            pre.append(worst)
                            continue
                        P2, N2 = move(P1, N1, False, k, q2)
                        if q2 == (0, 0):
                            seen["reply_onto_origin"] += 1
                        if not P2:
                            seen["mover_last_cube_captured"] += 1
                        worst = min(worst, leaf_value(P2, N2, S, False))
                        pre.append(worst)
                    at = next((n for n in range(3) if pre[n] <= best), None)
                    seen[("cut_first", "cut_second", "cut_third")[at] if at is not None else "no_cut"] += 1
                    if at is not None and slot == 1:
                        seen["second_cube_cut_by_first"] += 1
                    key[k] = (True, pre[at]) if at is not None else (False, pre[2])
                v = 0
                for d1 in range(1, 7):
                    F, G = pair_for(N1, d1)
                    if key[F][0] or G is None:
                        w = key[F][1]
                    elif key[G][0]:
                        w = key[G][1]
                    else:
                        w = min(key[F][1], key[G][1])
                    v += w / 6
            if v > best:
                best, action = v, (flag, d)
    return action, best


def make_positions(S, n=M_POS):
    """random oracle play from the benchmark's seeds (9487 + lane, Philox key 2024), two thirds as they are, one third thinned to endgames"""
    env = po.OracleVecEnv(n, board_size=S, opponent="random", rng="philox", philox_key=2024)
    env.reset(np.arange(n, dtype=np.uint32) + 9487)
    rs = np.random.RandomState(2024 + S)
    max_steps = 3 * S
    stop = rs.randint(0, max_steps, n)
    b, d = env.obs()
    b, d = b.copy(), d.copy()
    for t in range(max_steps):
        nb, nd, r, te, tr, info = env.step(env.sample_legal_actions(t))
        live = (te == 0) & (stop > t)
        b[live], d[live] = nb[live], nd[live]
        stop[te != 0] = 0       # a finished game keeps its last live position
    for i in range(2 * n // 3, n):
        for sign in (1, -1):
            cubes = [c for c in range(1, 7) if (b[i] == sign * c).any()]
            keep = rs.choice(cubes, size=min(len(cubes), rs.randint(1, 4)), replace=False)
            for c in cubes:
                if c not in keep:
                    b[i][b[i] == sign * c] = 0
    d[:] = rs.randint(1, 7, n)
    return b, d


_POS = {}


def positions(S):
    if S not in _POS:
        _POS[S] = make_positions(S)
    return _POS[S]


@pytest.mark.parametrize("S", [5, 7])
def test_positions_cover_every_case_of_the_search(S):
    b, d = positions(S)
    assert ((b > 0).sum(axis=(1, 2)) >= 1).all() and ((b < 0).sum(axis=(1, 2)) >= 1).all()
    assert (b[:, S - 1, S - 1] <= 0).all() and (b[:, 0, 0] >= 0).all(), "a won position among the inputs"
    oa, ov, _ = po.predict_minimax(b, d, 3, "hybrid")
    seen = dict.fromkeys(CASES, 0)
    for i in range(len(b)):
        a, v = d3_model(b[i], int(d[i]), seen)
        assert a == (int(oa[i][0]), int(oa[i][1])), (i, b[i], d[i])
        assert np.float64(v).tobytes() == np.float64(ov[i]).tobytes(), (i, v, ov[i])
    print(S, seen)
    assert all(seen[c] > 0 for c in CASES), seen


@pytest.mark.parametrize("S", [5, 6, 7, 8])
def test_every_table_image_builds(S):
    """build_fast_tables refuses an image that holds a -0.0 in val6[] (d3_search's expectation starts from its first term, which
    equals 0.0 + term bit for bit for every other value); every image of every board size passes, and none holds one"""
    from ewn_gym_amd import _lib
    lib = _lib.load()
    n = lib.ewn_tables_bytes(S, 3)
    buf = np.zeros(n, np.uint8)
    assert lib.ewn_build_tables(S, 3, buf.ctypes.data_as(C.c_void_p)) == 0
    img = buf.reshape(8, n // 8)
    end = (max(lib.ewn_tables_rank_offset(S, 63, iy) for iy in range(64)) + 2 + 7) // 8 * 8   # val[] and val6[] follow rank[]
    for im in range(8):
        val = img[im][end:end + 2 * 8 * 1024].view(np.float64).reshape(2, 1024)
        assert val[0][0] == -INF and (val[0][1:] >= val[0][:-1]).all(), (S, im)      # really val[]: ascending from -inf
        assert np.array_equal(val[1], val[0] / 6.0), (S, im)
        assert not (np.signbit(val) & (val == 0)).any(), (S, im)


# ---------------------------------------------------------------- GPU

def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _cpu(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ea():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


HEURS = ["hybrid", "min_dist", "attk"]


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("heur", HEURS)
def test_predict_on_constructed_positions(ea, S, heur):
    """stateless predict (fast_d3 -> d3_search, one lane per position; 32-bit masks on 5x5, 64-bit on 7x7): action and root value bits"""
    b, d = positions(S)
    for depth in (3, 4):
        oa, ov, _ = po.predict_minimax(b, d, depth, heur)
        acts, vals = ea.predict_minimax(b, d, depth, heur)
        bad = np.flatnonzero((_cpu(acts) != oa).any(axis=1) | (_bits(_cpu(vals)) != _bits(ov)))
        assert bad.size == 0, (S, heur, depth, bad[:5].tolist(), b[bad[:1]], d[bad[:1]])


def _pair(ea, N, lo, hi, S, heur, key, autoreset=True, max_depth=3, rng="philox", opponent="minimax", pos=None):
    """engine env of N lanes and oracle env of its lanes lo..hi, both holding the constructed positions (lane l: position 7 l mod M);
    pos: (boards, dice) to use instead of this module's positions(S)"""
    b, d = positions(S) if pos is None else pos
    idx = (np.arange(N) * 7) % len(b)
    kw = dict(board_size=S, max_depth=max_depth, heuristic=heur, rng=rng, philox_key=key, autoreset=autoreset, seed_stride=N)
    env = ea.VecEWN(N, opponent_policy=opponent, **kw)
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)
    env.reset(seeds=seeds)
    env.set_obs(b[idx], d[idx])
    orc = po.OracleVecEnv(hi - lo, opponent=opponent, lane_offset=lo, **kw)
    orc.reset(seeds=seeds[lo:hi])
    orc.set_obs(b[idx[lo:hi]], d[idx[lo:hi]])
    return env, orc


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("heur", HEURS)
def test_one_step_on_constructed_positions(ea, S, heur):
    """ewn_step (k_step_d3, two lanes per game): a legal agent move, then the opponent's depth-3 reply, on every position"""
    N = M_POS
    env, orc = _pair(ea, N, 0, N, S, heur, 61, autoreset=False)
    acts = orc.sample_legal_actions(0)
    ob, od, r, te, tr, info = orc.step(acts)
    gb, gd, gr, gte, gtr, ginfo = [_cpu(x) for x in env.step(acts)]
    assert np.array_equal(gb, ob) and np.array_equal(gd, od)
    assert np.array_equal(_bits(gr), _bits(r))
    assert np.array_equal(gte != 0, te != 0) and np.array_equal(gtr != 0, tr != 0) and np.array_equal(ginfo, info)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("heur", HEURS)
@pytest.mark.parametrize("N,lo,n,layout", [(257, 0, 257, "columns"), (4099, 2000, 2099, "columns"), (65536, 63488, 2048, "record")],
                         ids=["lockstep-257", "lockstep-4099", "slots-65536"])
def test_four_steps_on_constructed_positions(ea, S, heur, N, lo, n, layout):
    """ewn_step_k, K = 4, the random agent: the lock-step kernel (two sizes that are no multiple of a block) and the slot-task kernel
    at its smallest size, with the record layout -- step for step against the oracle from the constructed positions"""
    K = 4
    env, orc = _pair(ea, N, lo, lo + n, S, heur, 62)
    traj = env.alloc_rollout(K, board=True, layout=layout)
    env.rollout(K, agent="random", traj=traj)
    tj = {k: _cpu(v[:, lo:lo + n]) for k, v in traj.items()}
    for k in range(K):
        acts = orc.random_actions()
        assert np.array_equal(tj["action"][k], acts), k
        ob, od, r, te, tr, info = orc.step(acts)
        assert np.array_equal(tj["board"][k], ob) and np.array_equal(tj["dice"][k], od), k
        assert np.array_equal(_bits(tj["reward"][k]), _bits(r)), k
        assert np.array_equal(tj["terminated"][k], te) and np.array_equal(tj["truncated"][k], tr) and np.array_equal(tj["info"][k], info), k
    assert np.array_equal(_cpu(env.board[lo:lo + n]), ob) and np.array_equal(_cpu(env.dice[lo:lo + n]), od)
