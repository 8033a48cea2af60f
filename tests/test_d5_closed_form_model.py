"""A Python model of the CLOSED FORM the max_depth 5 / 6 kernel search uses (ewn_gym_amd/csrc/ewn_search_d5.hpp),
checked on the CPU against the oracle's literal recursion (classical_policies/minimax.py:19-73).

The reference searches root move -> dice -> reply -> dice -> move -> leaf with its alpha-beta window handed through
the chance nodes unchanged.  The model below states what that loop computes WITHOUT recursion, breaks or a window:

* a root's value is  sum_d1 M3(d1) / 6;  M3(d1) scans the replies of the cube pair (F = the dice cube or its larger
  neighbour, G = the smaller neighbour) the dice selects (envs/ewn.py:338-375);
* the value of one reply, C2(reply, beta) = sum_d2 X1(d2) / 6, depends on the scan only through beta = the running
  minimum in front of it; X1 stops at the first prefix maximum >= beta (the root's alpha never reaches beta);
* a cube's three replies AS F start from beta = +inf: their values are the same for every dice that selects the cube
  as F.  AS G the chain starts from its F partner's minimum -- and a cube's F partner is always the next cube above it
  that is still on the board, so that chain too is computed once.  At most 6 cubes x (3 + 3) reply evaluations per root
  instead of 6 dice x 6 replies, over <= 18 x 18 distinct leaf positions per root instead of 6 x 6 x 6 x 6.

The HIP kernel evaluates exactly these quantities (leaves as table ranks); this file pins the derivation itself.
"""
import numpy as np
import pytest

from oracle import pyoracle as po

INF = float("inf")
DIRS_P = ((0, 1), (1, 0), (1, 1))      # TOP_LEFT (the searcher, positive cubes): right, down, diagonal
DIRS_N = ((0, -1), (-1, 0), (-1, -1))  # BOTTOM_RIGHT (the replier, negative cubes)


def hybrid(P, N, S):
    """envs/minimax_ewn.py:56-86 for agent_player = TOP_LEFT on a position nobody has won"""
    mdp = min(max(S - 1 - i, S - 1 - j) for (i, j) in P.values())
    mdn = min(max(S - 1 - i, S - 1 - j) for (i, j) in N.values())
    score = 0
    score += (S - mdp) * (1 / len(P))
    score -= (S - mdn) * (1 / len(N))
    return score


def leaf_value(P, N, S, depth6):
    if (S - 1, S - 1) in P.values() or not N:
        return 10
    if (0, 0) in N.values() or not P:
        return -10
    e = hybrid(P, N, S)
    if not depth6:
        return e
    acc = 0
    for _ in range(6):  # the extra chance node of max_depth 6: evaluate() / 6 summed over the dice
        acc += e / 6
    return acc


def move(P, N, mover_is_p, k, dest):
    """envs/ewn.py:252-261: whatever stands on dest leaves the board, own cubes included"""
    P2 = {c: q for c, q in P.items() if q != dest}
    N2 = {c: q for c, q in N.items() if q != dest}
    (P2 if mover_is_p else N2)[k] = dest
    return P2, N2


def pair_for(side, d):
    """cubes a dice value selects, in list order: (F, G); cube numbers 1..6 (envs/ewn.py:144-176, 338-375)"""
    if d in side:
        return d, None
    up = next((k for k in range(d + 1, 7) if k in side), None)
    down = next((k for k in range(d - 1, 0, -1) if k in side), None)
    if up is not None:
        return up, down
    return down, None


def dests(pos, dirs, S):
    out = []
    for di, dj in dirs:
        i, j = pos[0] + di, pos[1] + dj
        out.append((i, j) if 0 <= i < S and 0 <= j < S else None)
    return out


# Every situation the kernel treats on a path of its own (ewn_search_d5.hpp).  With a `seen` dict the model counts how often each
# occurs in what it is given; tests/test_gpu_search_d5.py asserts that its constructed positions contain every one of them.
_CUT = ("cut_first", "cut_second", "cut_third", "no_cut")
CASES = (
    # root
    "root_one_cube", "root_two_cubes", "root_off_board", "root_captures_replier", "root_captures_own", "root_wins_corner",
    "root_wins_last_cube", "first_root_minus_inf", "later_root_ties_best",
    # the replier's dice d1
    "d1_own_cube", "d1_only_above", "d1_only_below", "d1_pair_F_cut", "d1_pair_G_chain",
    # a replier cube's chain as F, and as G (odd / even cube number: lane 0 / lane 1 of a two-lane pair)
    *("f_" + c for c in _CUT), *("g_odd_" + c for c in _CUT), *("g_even_" + c for c in _CUT),
    # G's F partner: two numbers above (on two lanes it comes from the previous step's carry) or further; and a G chain that is
    # never started because that partner cut
    "g_odd_partner_two_above", "g_even_partner_two_above", "g_odd_partner_further", "g_even_partner_further", "g_skipped_partner_cut",
    # replies
    "reply_off_board", "reply_first_off_board", "reply_onto_origin", "reply_captures_searcher", "reply_captures_last_searcher",
    "reply_captures_own", "reply_from_far_corner",
    # the inner max node (d5c_reply_value)
    *("x_" + c for c in _CUT), "x_beta_inf", "x_own_cube", "x_only_above", "x_only_below", "x_pair_F_cut", "x_pair_G_cut",
    "x_pair_both_cut_G_higher", "x_pair_max",
    # leaves
    "leaf_off_board_replaced", "leaf_captures_own", "leaf_reaches_corner", "leaf_takes_last_replier",
)


def _hit(seen, name):
    if seen is not None:
        seen[name] += 1


def leaf_dests(pos, S):
    """a searcher cube's three leaf moves as the kernel takes them: a direction that leaves the board is replaced by one of the
    cube's directions that does not (a repeated leaf changes neither the prefix maxima nor the value the scan stops at)
    -> (destinations, how many were replaced)"""
    d0, d1, d2 = dests(pos, DIRS_P, S)
    q0 = d0 if d0 is not None else d1
    q1 = d1 if d1 is not None else d0
    q2 = d2 if d2 is not None else q0
    assert q0 is not None, "a searcher cube on the far corner below a root that did not win"
    return (q0, q1, q2), (d0 is None) + (d1 is None) + (d2 is None)


def c2(P2, N2, S, beta, depth6, seen=None):
    """chance node under a reply: sum over dice of the depth-1 max node's value / 6, the max node cut at beta"""
    # key of a searcher cube: (cut?, value) -- the first of the three prefix maxima of its leaves that is >= beta, else the last
    key = {}
    for k, pos in P2.items():
        best, seq = -INF, []
        qs, replaced = leaf_dests(pos, S)
        if seen is not None:
            seen["leaf_off_board_replaced"] += replaced
        for q in qs:
            P3, N3 = move(P2, N2, True, k, q)
            if seen is not None:
                seen["leaf_captures_own"] += q in P2.values()
                seen["leaf_reaches_corner"] += q == (S - 1, S - 1)
                seen["leaf_takes_last_replier"] += not N3
            best = max(best, leaf_value(P3, N3, S, depth6))
            seq.append(best)
        at = next((n for n in range(3) if seq[n] >= beta), None)
        key[k] = (True, seq[at]) if at is not None else (False, seq[2])
        _hit(seen, "x_beta_inf" if beta == INF else "x_" + _CUT[3 if at is None else at])
    val = 0
    for d in range(1, 7):
        F, G = pair_for(P2, d)
        if G is None:
            x = key[F][1]
            _hit(seen, "x_own_cube" if F == d else "x_only_above" if F > d else "x_only_below")
        elif key[F][0]:
            x = key[F][1]
            _hit(seen, "x_pair_F_cut")
            if key[G][0] and key[G][1] > x:     # the kernel takes one max over both keys: F's cut flag has to outrank G's
                _hit(seen, "x_pair_both_cut_G_higher")
        elif key[G][0]:
            x = key[G][1]
            _hit(seen, "x_pair_G_cut")
        else:
            x = max(key[F][1], key[G][1])
            _hit(seen, "x_pair_max")
        val += x / 6
    return val


def chain(P1, N1, S, k, start, alpha, depth6, seen=None, tag="f"):
    """min node restricted to cube k's replies, entered with running minimum `start`:
    -> (cut?, value): the value at which `worst <= alpha` stops the loop inside this cube, else the minimum reached.
    The cube's replies are counted in `seen` on its chain as F only (tag "f"): as G it makes the same ones again."""
    worst = start
    replies = seen if tag == "f" else None
    if N1[k] == (S - 1, S - 1):
        _hit(replies, "reply_from_far_corner")
    for j, q in enumerate(dests(N1[k], DIRS_N, S)):
        if q is None:
            _hit(replies, "reply_off_board")
            if j == 0:
                _hit(replies, "reply_first_off_board")   # the second reply then runs the cutting path with beta = +inf
            continue
        P2, N2 = move(P1, N1, False, k, q)
        if replies is not None:
            replies["reply_onto_origin"] += q == (0, 0)
            replies["reply_captures_searcher"] += q in P1.values()
            replies["reply_captures_last_searcher"] += not P2
            replies["reply_captures_own"] += q in N1.values()
        if q == (0, 0) or not P2:
            val = -10
        else:
            val = c2(P2, N2, S, worst, depth6, seen)
        if val < worst:
            worst = val
        if worst <= alpha:
            _hit(seen, tag + "_" + _CUT[j])
            return True, worst
    _hit(seen, tag + "_no_cut")
    return False, worst


def d5_closed_form(board, dice, depth, seen=None):
    """(action, value) of ExpectiMinimaxAgent(max_depth = 5 or 6, 'hybrid').predict in closed form; `seen`: a dict with the keys
    CASES in which the situations this position contains are counted"""
    S = board.shape[0]
    depth6 = depth == 6
    P = {int(v): (i, j) for (i, j), v in np.ndenumerate(board) if v > 0}
    N = {int(-v): (i, j) for (i, j), v in np.ndenumerate(board) if v < 0}
    best, action = -INF, (0, 0)
    F0, G0 = pair_for(P, dice)
    roots = [(F0, 1 if F0 > dice else 0)] + ([(G0, 0)] if G0 is not None else [])
    _hit(seen, "root_one_cube" if G0 is None else "root_two_cubes")
    for cube, flag in roots:
        for d, q in enumerate(dests(P[cube], DIRS_P, S)):
            if q is None:
                _hit(seen, "root_off_board")
                continue
            if seen is not None:
                seen["root_captures_replier"] += q in N.values()
                seen["root_captures_own"] += q in P.values()
            P1, N1 = move(P, N, True, cube, q)
            if q == (S - 1, S - 1) or not N1:
                v = 10
                _hit(seen, "root_wins_corner" if q == (S - 1, S - 1) else "root_wins_last_cube")
            else:
                alpha = best
                if alpha == -INF:
                    _hit(seen, "first_root_minus_inf")
                # every replier cube once as F; and once as G behind the next cube above it -- if a dice can select it as G at all
                # (the cube directly above it is off the board) and that F partner did not cut (else the scan never reaches G)
                A, B = {}, {}
                for k in sorted(N1, reverse=True):
                    A[k] = chain(P1, N1, S, k, INF, alpha, depth6, seen)
                    up = next((u for u in range(k + 1, 7) if u in N1), None)
                    if up is None or up == k + 1:
                        continue
                    if A[up][0]:
                        _hit(seen, "g_skipped_partner_cut")
                        continue
                    tag = "g_odd" if k % 2 else "g_even"
                    _hit(seen, tag + ("_partner_two_above" if up == k + 2 else "_partner_further"))
                    B[k] = chain(P1, N1, S, k, A[up][1], alpha, depth6, seen, tag)
                v = 0
                for d1 in range(1, 7):
                    F, G = pair_for(N1, d1)
                    if G is None:
                        w = A[F][1]
                        _hit(seen, "d1_own_cube" if F == d1 else "d1_only_above" if F > d1 else "d1_only_below")
                    elif A[F][0]:
                        w = A[F][1]
                        _hit(seen, "d1_pair_F_cut")
                    else:
                        w = B[G][1]
                        _hit(seen, "d1_pair_G_chain")
                    v += w / 6
            if v == best:
                _hit(seen, "later_root_ties_best")      # the first root is kept
            if v > best:
                best, action = v, (flag, d)
    return action, best


def positions(S, n, seed, max_steps):
    env = po.OracleVecEnv(n, board_size=S, opponent="random", rng="philox", philox_key=seed)
    env.reset(np.arange(n, dtype=np.uint32) + seed)
    rs = np.random.RandomState(seed)
    stop = rs.randint(0, max_steps, n)
    keep_b, keep_d = env.obs()
    keep_b, keep_d = keep_b.copy(), keep_d.copy()
    for t in range(max_steps):
        b, d, r, te, tr, info = env.step(env.sample_legal_actions(t))
        live = (te == 0) & (stop > t)
        keep_b[live], keep_d[live] = b[live], d[live]
        if not live.any():
            break
    return keep_b, keep_d


@pytest.mark.parametrize("S,depth,n", [(5, 5, 60), (5, 6, 16), (6, 5, 12)])
def test_closed_form_equals_the_reference_recursion(S, depth, n):
    b, d = positions(S, n, 77 + S + depth, 12 if S == 5 else 18)
    oa, ov, _ = po.predict_minimax(b, d, depth, "hybrid")
    for i in range(n):
        a, v = d5_closed_form(b[i], int(d[i]), depth)
        assert (a[0], a[1]) == (int(oa[i][0]), int(oa[i][1])), (i, b[i], d[i])
        assert np.float64(v).tobytes() == np.float64(ov[i]).tobytes(), (i, v, ov[i])
