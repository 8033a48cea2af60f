"""ewn_lookahead_expand / ewn_lookahead_reduce and the two-move lookahead built from them (predict_lookahead(plies=2)).
1. expand -> predict_policy's value -> reduce is the one-move tree cut at its two ends, so it must give ewn_predict_lookahead's Q bit for
bit: two HIP implementations of one definition.  2. expand against the rules (the numpy model of tests/test_gpu_predict_lookahead.py).
3. Two moves against a numpy model: tree() for the structure, a leaf's value L = the maximum of the finite entries of
predict_lookahead(b2, d2, return_q=True), means and minima in float64.  The tolerance is 4k's, derived there and not tuned: the two nested
six-term fp32 means are the same, so atol = 32 * 2^-24 * max(1, max |L|, terminal_value).  4. constructed positions.  5. plumbing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, cube_moves, find_cube, i8, tree  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def cubes(board, player):
    return {abs(int(v)) for v in board.flat if v * player > 0}


def lost(b2):
    return bool(b2[0, 0] < 0 or not (b2 > 0).any())


# ---------------------------------------------------------------- 1. the stages against the existing kernel

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 31, 33, 300])     # a lone row, a partial tile of the leaf kernel, one past it, several blocks
def test_stages_reproduce_the_one_move_kernel(ea, S, M):
    p = pool(ea, S)
    b, d = p["boards"][:M], p["dice"][:M]
    lb, ld, kind = ea.lookahead_expand(b, d)
    assert lb.shape == (M, 648, S, S) and ld.shape == (M, 648) and kind.shape == (M, 108)
    assert lb.dtype == ld.dtype == kind.dtype == torch.int8
    v = ea.predict_policy(lb.reshape(-1, S, S), ld.reshape(-1), p["params"], return_value=True)[1]
    act, q = ea.lookahead_reduce(b, d, kind, v.reshape(M, 648), return_q=True)
    act1, q1 = ea.predict_lookahead(b, d, p["params"], return_q=True)
    assert act.shape == (M, 2) and act.dtype == torch.int8 and q.shape == (M, 2, 3) and q.dtype == torch.float32
    fin = torch.isfinite(q1) & torch.isfinite(q)
    print("S=%d M=%d: max |Q_stages - Q_kernel| %.3g, %d of %d entries differ by bit pattern"
          % (S, M, float((q[fin] - q1[fin]).abs().max()) if bool(fin.any()) else 0.0, int((bits(q) != bits(q1)).sum()), q.numel()))
    assert torch.equal(bits(q), bits(q1))
    assert torch.equal(act, act1)
    assert torch.equal(ea.lookahead_reduce(b, d, kind, v.reshape(M, 648)), act1)           # q NULL: the same actions


# ---------------------------------------------------------------- 2. expand against the rules

def tuples(board, d):
    """None for a degenerate row; else {t: "lost" | b2} over the tuples t = 18 (3 f + r) + 3 (k - 1) + e that exist: the agent's move
    (f, r) is searched (on the board, not a win, not a repeat of roots 0..2) and cube k's reply in direction e stays on the board"""
    d = min(max(int(d), 1), 6)
    if board[0, 0] < 0 or board[-1, -1] > 0 or not (board > 0).any() or not (board < 0).any():
        return None
    mine = cubes(board, 1)
    c = (find_cube(mine, d, False), find_cube(mine, d, True))
    out = {}
    for f in (0, 1):
        if f == 1 and c[1] == c[0]:
            continue
        for r, b1 in cube_moves(board, c[f], 1):
            if b1[-1, -1] > 0 or not (b1 < 0).any():
                continue
            for k in cubes(b1, -1):
                for e, b2 in cube_moves(b1, k, -1):
                    out[18 * (3 * f + r) + 3 * (k - 1) + e] = "lost" if lost(b2) else b2
    return out


def check_expand(ea, b, d):
    M, S = b.shape[0], b.shape[1]
    lb, ld, kind = (x.cpu().numpy() for x in ea.lookahead_expand(b, d))
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(ld, np.tile(np.arange(1, 7, dtype=np.int8), (M, 108)))           # every row's dice is its d2
    nleaf = 0
    for m in range(M):
        tp, tr = tuples(hb[m], hd[m]), tree(hb[m], hd[m])
        assert (tp is None) == (tr is None)
        want_kind, want = np.zeros(108, np.int8), np.zeros((648, S, S), np.int8)
        for t, node in (tp or {}).items():
            want_kind[t] = 1 if isinstance(node, str) else 2
            if not isinstance(node, str):
                want[6 * t:6 * t + 6] = node
                nleaf += 1
        assert np.array_equal(kind[m], want_kind), (m, kind[m], want_kind)
        assert np.array_equal(lb[m], want), m                                              # b2 on the leaves, zero everywhere else
        # ... and the tuples are tree()'s: under d1 = k both flags name cube k, so tree()'s replies there are cube k's, in direction order
        mine = cubes(hb[m], 1) if tr is not None else set()
        for (f, r), node in (tr or {}).items():
            dd = min(max(int(hd[m]), 1), 6)
            root = 3 * f + r
            if f == 1 and find_cube(mine, dd, True) == find_cube(mine, dd, False):
                assert not (kind[m, 18 * root:18 * root + 18] != 0).any()
                continue
            if node == "win":
                assert not (kind[m, 18 * root:18 * root + 18] != 0).any()
                continue
            seen = 0
            for k in range(1, 7):
                ks = kind[m, 18 * root + 3 * (k - 1):18 * root + 3 * k]
                if not ks.any():
                    continue
                reps = node[k - 1]
                assert [1 if isinstance(x, str) else 2 for x in reps] == [int(x) for x in ks if x != 0]
                seen += len(reps)
            assert seen == int((kind[m, 18 * root:18 * root + 18] != 0).sum())
    return nleaf


@pytest.mark.parametrize("S", [5, 7])
def test_expand_against_the_rules(ea, S):
    p = pool(ea, S)
    M = 33
    n = check_expand(ea, p["boards"][:M], p["dice"][:M])
    print("S=%d: %.1f leaves per observation" % (S, n / M))
    assert n > 20 * M                                                                       # real play: the tree is near its full size
    b = p["boards"][:M].clone()
    dead = boards_of(S, {(S - 1, S - 1): 3, (0, 1): -2}, {(0, 0): -1, (2, 2): 4}, {(2, 2): -3}, {(2, 2): 3}, {})
    b[[0, 7, 30, 31, 32]] = dead
    check_expand(ea, b, p["dice"][:M])
    lb, ld, kind = ea.lookahead_expand(b, p["dice"][:M])
    assert int(kind[[0, 7, 30, 31, 32]].abs().sum()) == 0 and int(lb[[0, 7, 30, 31, 32]].abs().sum()) == 0


# ---------------------------------------------------------------- 3. two moves against a numpy model

def model_q2(ea, boards, dice, params, tv=1.0):
    """(Q2_model float64 [M, 2, 3], atol): the structure from tree(), L from predict_lookahead's q, everything else float64"""
    boards, dice = boards.cpu().numpy(), dice.cpu().numpy()
    M = boards.shape[0]
    trees = [tree(boards[m], dice[m]) for m in range(M)]
    leaves, index = [], {}
    for t in trees:
        for node in (t or {}).values():
            if node == "win":
                continue
            for reps in node:
                for b2 in reps:
                    if not isinstance(b2, str) and b2.tobytes() not in index:
                        index[b2.tobytes()] = len(leaves)
                        leaves.append(b2)
    L = np.zeros((0, 6))
    if leaves:
        lb = torch.as_tensor(np.stack(leaves)).to(torch.int8).cuda().repeat_interleave(6, 0).contiguous()
        ld = torch.arange(1, 7, dtype=torch.int8, device="cuda").repeat(len(leaves)).contiguous()
        q1 = ea.predict_lookahead(lb, ld, params, terminal_value=tv, return_q=True)[1].double().cpu().numpy().reshape(-1, 6)
        assert np.isfinite(q1).any(1).all()                         # a non-terminal board always has a move that stays on it
        L = np.where(np.isfinite(q1), q1, -np.inf).max(1).reshape(-1, 6)
    Q = np.full((M, 2, 3), -np.inf)
    for m, t in enumerate(trees):
        for (f, r), node in (t or {}).items():
            if node == "win":
                Q[m, f, r] = tv
            else:
                Q[m, f, r] = np.mean([min((-tv if isinstance(b2, str) else L[index[b2.tobytes()]].mean()) for b2 in reps) for reps in node])
    atol = 32 * 2.0 ** -24 * max(1.0, float(np.abs(L).max()) if leaves else 0.0, tv)
    return Q, atol


def check2(ea, boards, dice, params, tv=1.0, model=None, what="", **kw):
    """the two-move Q against the model's and the pick against both; returns (actions, q, Q_model) as numpy"""
    act, q = ea.predict_lookahead(boards, dice, params, terminal_value=tv, return_q=True, plies=2, **kw)
    M = boards.shape[0]
    assert act.shape == (M, 2) and act.dtype == torch.int8 and q.shape == (M, 2, 3) and q.dtype == torch.float32
    Qm, atol = model if model is not None else model_q2(ea, boards, dice, params, tv)
    Qm = Qm[:M]
    a, qk = act.cpu().numpy().astype(np.int64), q.double().cpu().numpy()
    fin = np.isfinite(Qm)
    err = float(np.abs(qk[fin] - Qm[fin]).max()) if fin.any() else 0.0
    print("%s M=%d: max |Q2 - Q2_model| %.3g (atol %.3g)" % (what, M, err, atol))
    assert np.array_equal(qk == -np.inf, ~fin) and not np.isnan(qk).any() and not (qk == np.inf).any()
    assert err <= atol, (err, atol)
    flat = a[:, 0] * 3 + a[:, 1]
    assert np.array_equal(flat, qk.reshape(M, 6).argmax(1))          # the first row-major maximum of the RETURNED Q2, exactly
    chosen = Qm.reshape(M, 6)[np.arange(M), flat]
    assert (chosen >= Qm.reshape(M, 6).max(1) - 2 * atol).all()      # every row, none excluded
    return a, qk, Qm


_MODEL = {}


def pool_model2(ea, S):
    """the model's Q2 of the pool's first 70 observations, computed once per board size and left unchanged"""
    if S not in _MODEL:
        p = pool(ea, S)
        _MODEL[S] = model_q2(ea, p["boards"][:70], p["dice"][:70], p["params"])
    return _MODEL[S]


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 33, 70])
def test_two_moves_against_the_model(ea, S, M):
    p = pool(ea, S)
    b, d = p["boards"][:M], p["dice"][:M]
    a, qk, _ = check2(ea, b, d, p["params"], model=pool_model2(ea, S), what="S=%d" % S)
    if M == 1:                                        # a single [S, S] board
        assert np.array_equal(ea.predict_lookahead(b[0], d, p["params"], plies=2).cpu().numpy(), a)


# ---------------------------------------------------------------- 4. constructed positions

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("tv", [1.0, 0.5])
def test_a_win_forced_in_two(ea, S, tv):
    """the agent's only cube two diagonal steps from the corner, the opponent's only cube on (S-1, 0): after the diagonal move the only
    reply is up, and the second diagonal move wins under every dice -- the two-move Q of that root is the terminal value itself"""
    params = pool(ea, S)["params"]
    b = boards_of(S, {(S - 3, S - 3): 1, (S - 1, 0): -1})
    d = i8(1)
    a, q2, _ = check2(ea, b, d, params, tv=tv, what="S=%d tv=%g forced win" % (S, tv))
    q1 = ea.predict_lookahead(b, d, params, terminal_value=tv, return_q=True)[1].cpu().numpy()
    print("S=%d tv=%g: Q2 %s, Q1 %s" % (S, tv, q2[0].tolist(), q1[0].tolist()))
    assert q2[0, 0, 2] == tv and q2[0, 1, 2] == tv
    assert q1[0, 0, 2] != tv and np.isfinite(q1[0, 0, 2])


@pytest.mark.parametrize("S", [5, 7])
def test_constructed_positions(ea, S):
    params = pool(ea, S)["params"]
    E = S - 1
    specs = [
        ({(1, 1): 3, (E - 1, E - 1): -2}, 4),                                             # 0 one cube a side
        ({(0, 2): 2, (2, 0): 5, (E, E - 1): -1, (E - 1, E): -4, (E - 2, E - 2): -6}, 3),  # 1 dice's cube gone, two neighbours: the flags differ
        ({(0, 2): 4, (2, 0): 5, (E, E - 1): -1, (E - 1, E): -4, (E - 2, E - 2): -6}, 2),  # 2 ... one neighbour only: both flags name cube 4
        ({(E - 1, E): 1, (0, 1): 2, (E, 0): -1, (E - 1, 1): -5}, 1),                      # 3 down wins at the corner; right and diagonal leave the board
        ({(1, 1): 3, (2, 2): -4}, 6),                                                     # 4 the diagonal captures the last opposing cube
        ({(2, 2): 1, (1, 3): 4, (0, 1): -3}, 1),                                          # 5 the only reply takes (0, 0), under every dice
        ({(1, 1): 1, (1, 2): 2, (2, 3): -2, (E, E): -5}, 1),                              # 6 right captures the own cube 2; then a reply can take the last cube
        ({(E, 1): 2, (1, 1): 5, (E - 1, E - 1): -3, (2, E): -1}, 3),                      # 7 flag 0's cube on the last row: down and diagonal leave the board
        ({(E, E): 2, (1, 1): 5, (E - 1, 2): -3}, 2),                                      # 8 all three directions leave the board: only on the far corner = already won
    ]
    b = boards_of(S, *[s for s, _ in specs])
    d = i8(*[x for _, x in specs])
    check_expand(ea, b, d)
    for tv in (1.0, 0.5):
        a, qk, Qm = check2(ea, b, d, params, tv=tv, what="S=%d tv=%g constructed" % (S, tv))
        q32 = ea.predict_lookahead(b, d, params, terminal_value=tv, return_q=True, plies=2)[1]
        assert np.isfinite(qk[0]).all()
        assert not np.array_equal(qk[1, 0], qk[1, 1])                                         # cube 2 and cube 5: other moves, other values
        assert torch.equal(bits(q32[2, 0]), bits(q32[2, 1])) and a[2, 0] == 0                  # one cube under both flags: bit for bit, and the first wins
        assert qk[3, 0, 1] == tv and qk[3, 1, 1] == tv and np.isneginf(qk[3, :, [0, 2]]).all() and tuple(a[3]) == (0, 1)
        assert qk[4, 0, 2] == tv and tuple(a[4]) == (0, 2) and np.isfinite(qk[4]).all()
        assert (qk[5] == -tv).all() and tuple(a[5]) == (0, 0)
        assert np.isfinite(qk[6]).all()                                                       # the own-cube capture is a move like any other
        assert np.isneginf(qk[7, 0, 1]) and np.isneginf(qk[7, 0, 2]) and np.isfinite(qk[7, 0, 0]) and np.isfinite(qk[7, 1]).all()
        assert np.isneginf(qk[8]).all() and tuple(a[8]) == (0, 0)


@pytest.mark.parametrize("S", [5, 7])
def test_degenerate_rows_among_live_ones_and_dice_out_of_range(ea, S):
    p = pool(ea, S)
    M = 40
    la2 = lambda bb, dd: ea.predict_lookahead(bb, dd, p["params"], return_q=True, plies=2)   # noqa: E731
    b, d = p["boards"][:M].clone(), p["dice"][:M].clone()
    act0, q0 = la2(b, d)
    dead = boards_of(S, {(S - 1, S - 1): 3, (0, 1): -2}, {(0, 0): -1, (2, 2): 4}, {(2, 2): -3}, {(2, 2): 3}, {})
    rows = [0, 7, 31, 32, 39]       # agent on the far corner, opponent on (0, 0), no agent cube, no opposing cube, an empty board
    b[rows] = dead
    check2(ea, b, d, p["params"], what="S=%d mixed" % S)
    act, q = la2(b, d)
    live = torch.ones(M, dtype=torch.bool, device="cuda")
    live[rows] = False
    assert torch.isneginf(q[rows]).all() and int(act[rows].abs().sum()) == 0
    assert torch.equal(bits(q[live]), bits(q0[live])) and torch.equal(act[live], act0[live])
    # dice 0 and 7 are dice 1 and 6
    lo, hi, one, six = la2(b, torch.zeros_like(d)), la2(b, torch.full_like(d, 7)), la2(b, torch.ones_like(d)), la2(b, torch.full_like(d, 6))
    assert torch.equal(lo[0], one[0]) and torch.equal(bits(lo[1]), bits(one[1]))
    assert torch.equal(hi[0], six[0]) and torch.equal(bits(hi[1]), bits(six[1]))
    assert not torch.equal(bits(one[1]), bits(six[1]))
    for dd in (torch.zeros_like(d), torch.full_like(d, 7)):                                # ... in the stages themselves
        x, y = ea.lookahead_expand(b, dd), ea.lookahead_expand(b, dd.clamp(1, 6))
        assert all(torch.equal(u, v) for u, v in zip(x, y))


# ---------------------------------------------------------------- 5. plumbing

@pytest.mark.parametrize("S", [5, 7])
def test_chunks_give_the_same_bits(ea, S):
    p = pool(ea, S)
    b, d = p["boards"][:70], p["dice"][:70]
    act, q = ea.predict_lookahead(b, d, p["params"], return_q=True, plies=2)
    for chunk in (32, 1000):                                                               # 32 + 32 + 6, and one chunk larger than M
        act_c, q_c = ea.predict_lookahead(b, d, p["params"], return_q=True, plies=2, chunk=chunk)
        assert torch.equal(act, act_c) and torch.equal(bits(q), bits(q_c))
    assert torch.equal(ea.predict_lookahead(b, d, p["params"], plies=2), act)              # q NULL: the same actions
    assert torch.equal(ea.predict_lookahead(b, d, p["params"], plies=2, chunk=32), act)
    a1, q1 = ea.predict_lookahead(b, d, p["params"], return_q=True)
    assert torch.equal(ea.predict_lookahead(b, d, p["params"], return_q=True, plies=1, chunk=3)[1], q1)   # plies=1: today's call
    assert not torch.equal(bits(q), bits(q1))


@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    """the three launches of a two-move call through the C ABI, every buffer they write (and `leaf`, which the middle one writes and the
    last one reads) between 4 KB guard zones, the inputs at an odd address"""
    from ewn_gym_amd import _lib
    lib = _lib.load()
    M = 33
    p = pool(ea, S)
    alloc = GuardedAllocator()
    b = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards", offset=1)
    d = alloc.zeros((M,), dtype=torch.int8, tag="dice", offset=1)
    b.copy_(p["boards"][:M]); d.copy_(p["dice"][:M])
    lb = alloc.zeros((648 * M, S, S), dtype=torch.int8, tag="leaf_boards")
    ld = alloc.zeros((648 * M,), dtype=torch.int8, tag="leaf_dice")
    kind = alloc.zeros((M, 108), dtype=torch.int8, tag="kind")
    la = alloc.zeros((648 * M, 2), dtype=torch.int8, tag="leaf actions")
    leaf = alloc.zeros((648 * M, 6), dtype=torch.float32, tag="leaf")
    act = alloc.zeros((M, 2), dtype=torch.int8, tag="actions")
    q = alloc.zeros((M, 2, 3), dtype=torch.float32, tag="q")
    lb.fill_(9); ld.fill_(9); kind.fill_(9)                      # nothing has to be cleared: every row is written
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ewn_lookahead_expand(S, 3, M, ptr(b), ptr(d), ptr(lb), ptr(ld), ptr(kind), st) == 0
    assert lib.ewn_predict_lookahead(S, 3, 648 * M, ptr(lb), ptr(ld), ptr(p["params"]), 1.0, ptr(la), ptr(leaf), st) == 0
    assert lib.ewn_lookahead_reduce(S, 3, M, ptr(b), ptr(d), ptr(kind), ptr(leaf), 6, 1.0, ptr(act), ptr(q), st) == 0
    torch.cuda.synchronize()
    alloc.check("S=%d M=%d" % (S, M))
    ref = ea.predict_lookahead(p["boards"][:M], p["dice"][:M], p["params"], return_q=True, plies=2)
    assert torch.equal(act, ref[0]) and torch.equal(bits(q), bits(ref[1]))
    x = ea.lookahead_expand(p["boards"][:M], p["dice"][:M])
    assert torch.equal(lb.reshape(M, 648, S, S), x[0]) and torch.equal(ld.reshape(M, 648), x[1]) and torch.equal(kind, x[2])
    assert torch.equal(b, p["boards"][:M]) and torch.equal(d, p["dice"][:M])               # the inputs are only read
    # the width-1 reduce and the bindings' own outputs, guarded as well
    v = alloc.zeros((M, 648), dtype=torch.float32, tag="leaf values")
    v.copy_(ea.predict_policy(lb, ld, p["params"], return_value=True)[1].reshape(M, 648))
    with alloc.patch(tag="outputs"):            # lookahead_reduce's torch.zeros outputs come out of the guarded allocator
        a1, q1 = ea.lookahead_reduce(b, d, kind, v, return_q=True)
    assert alloc.owns(a1) and alloc.owns(q1)
    torch.cuda.synchronize()
    alloc.check("S=%d M=%d width 1" % (S, M))
    one = ea.predict_lookahead(p["boards"][:M], p["dice"][:M], p["params"], return_q=True)
    assert torch.equal(a1, one[0]) and torch.equal(bits(q1), bits(one[1]))


def test_value_search_agent_two_moves_on_the_drop_in_env(ea):
    from classical_policies import ValueSearchAgent
    from envs import EinsteinWuerfeltNichtEnv
    p = pool(ea, 5)
    agent = ValueSearchAgent(p["model"], board_size=5, plies=2)
    assert agent.plies == 2 and agent.terminal_value == 1.0
    env = EinsteinWuerfeltNichtEnv(board_size=5, seed=3)
    obs, _ = env.reset(seed=3)
    steps = 0
    for _ in range(60):
        action, state = agent.predict(obs)
        assert state is None and isinstance(action, np.ndarray) and action.shape == (2,)
        batch, q = agent.predict_batch(obs["board"].astype(np.int8)[None], [obs["dice_roll"]], return_q=True)
        assert np.array_equal(action, batch[0].cpu().numpy()) and q.shape == (1, 2, 3)
        assert np.isfinite(q[0, action[0], action[1]].item())           # the lookahead never plays a move that leaves the board
        obs, _, terminated, truncated, _ = env.step(action)
        steps += 1
        if terminated or truncated:
            break
    assert terminated or truncated                                       # one whole episode
    b, d = p["boards"][:70], p["dice"][:70]
    assert torch.equal(agent.policy_fn()(b, d, 5), ea.predict_lookahead(b, d, p["params"], plies=2))


def test_two_moves_in_the_tournament(ea):
    from ewn_gym_amd.tournament import evaluate
    m = pool(ea, 5)["model"]
    r1 = evaluate({"kind": "mlp_lookahead", "model": m, "plies": 2}, {"kind": "random"}, num=16)
    r2 = evaluate({"kind": "mlp_lookahead", "model": m, "plies": 2}, {"kind": "random"}, num=16)
    assert r1["engine"] == "ewn_step" and r1["episodes"] == 16 and int((r1["lengths"] > 0).sum()) == 16
    assert torch.equal(r1["scores"], r2["scores"]) and torch.equal(r1["lengths"], r2["lengths"])
    assert bool((r1["scores"] != 0).all())                                # every episode ended: no illegal-move stall
