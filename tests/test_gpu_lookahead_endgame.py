"""Exact endgame values at the leaves of the searches (ewn_predict_lookahead_eg, predict_lookahead / predict_puct(endgame_table=),
DESIGN.md 4p), against the float64 model of tests/test_gpu_predict_lookahead.py with a leaf's value replaced by terminal_value *
table.value(b2) where table.lookup covers b2.  Tables: (5, 2, 4) and (7, 2, 3), built once per session (tests/test_gpu_endgame.py's).
The tolerance is 4k's, unchanged: atol = 32 * 2^-24 * max(1, max |leaf value|, terminal_value) -- the substitution removes roundings
(a covered leaf is one product instead of a six-term mean) and adds none to the two means above it."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_endgame import board_of, covered_np, few_cube_lanes, make_env, sample, table  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, i8, tree  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402

KT = {5: (2, 4), 7: (2, 3)}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def tab(ea, S):
    return table(ea, S, *KT[S])


# ---------------------------------------------------------------- the model of the definition

def model_q(ea, t, boards, dice, params, tv):
    """(Q_model float64 [M, 2, 3], atol, stats): tree() of 4k's test; a leaf that t.lookup covers is worth tv * t.value(b2), any other
    the float64 mean of predict_policy's six values.  stats, counted on the host with covered_np: per row the number of leaf tuples
    the table values and the number the critic values (a tuple = a distinct reply of a searched root), and whether some (root, d1)
    reply set holds both kinds"""
    boards, dice = boards.cpu().numpy(), dice.cpu().numpy()
    M = boards.shape[0]
    K, T = t.max_cubes, t.max_total
    trees = [tree(boards[m], dice[m]) for m in range(M)]
    leaves, index = [], {}
    for tr in trees:
        for node in (tr or {}).values():
            if node == "win":
                continue
            for reps in node:
                for b2 in reps:
                    if not isinstance(b2, str) and b2.tobytes() not in index:
                        index[b2.tobytes()] = len(leaves)
                        leaves.append(b2)
    val, cov = np.zeros(0), np.zeros(0, bool)
    if leaves:
        lb = torch.as_tensor(np.stack(leaves)).to(torch.int8).cuda().contiguous()
        _, c, e = t.lookup(lb, torch.ones(len(leaves), dtype=torch.int8, device="cuda"), return_value=True)
        cov = c.cpu().numpy()
        assert np.array_equal(cov, covered_np(np.stack(leaves), K, T))          # lookup's coverage is the definition's
        V = ea.predict_policy(lb.repeat_interleave(6, 0).contiguous(), torch.arange(1, 7, dtype=torch.int8, device="cuda").repeat(len(leaves)),
                              params, return_value=True)[1].double().cpu().numpy().reshape(-1, 6)
        val = np.where(cov, tv * e.double().cpu().numpy(), V.mean(1))
    Q = np.full((M, 2, 3), -np.inf)
    for m, tr in enumerate(trees):
        for (f, r), node in (tr or {}).items():
            if node == "win":
                Q[m, f, r] = tv
            else:
                Q[m, f, r] = np.mean([min((-tv if isinstance(b2, str) else val[index[b2.tobytes()]]) for b2 in reps) for reps in node])
    atol = 32 * 2.0 ** -24 * max(1.0, float(np.abs(val).max()) if leaves else 0.0, tv)
    return Q, atol, host_counts(boards, dice, K, T, trees)


def host_counts(boards, dice, K, T, trees=None):
    """counted on the host alone (tree() and covered_np on numpy boards): n_exact / n_critic int64 [M], the leaf tuples of each row
    that a (S, K, T) table covers / does not cover; mixed_set bool [M], whether some (root, d1) reply set holds both kinds"""
    M = boards.shape[0]
    trees = trees if trees is not None else [tree(boards[m], dice[m]) for m in range(M)]
    n_exact, n_critic, mixed_set = np.zeros(M, np.int64), np.zeros(M, np.int64), np.zeros(M, bool)
    covered = lambda b2: bool(covered_np(b2[None], K, T)[0])   # noqa: E731
    for m, tr in enumerate(trees):
        same = tr is not None and same_cube(boards[m], dice[m])
        for (f, r), node in (tr or {}).items():
            if node == "win":
                continue
            for reps in node:
                mixed_set[m] |= len({covered(b2) for b2 in reps if not isinstance(b2, str)}) == 2
            if f == 1 and same:          # both flags name one cube: roots 3 .. 5 are roots 0 .. 2, whose tuples are counted once
                continue
            # the root's leaf tuples are its distinct replies: every cube of the other side is some dice's cube
            for b2 in {b2.tobytes(): b2 for reps in node for b2 in reps if not isinstance(b2, str)}.values():
                n_exact[m] += covered(b2)
                n_critic[m] += not covered(b2)
    return dict(n_exact=n_exact, n_critic=n_critic, mixed_set=mixed_set)


def same_cube(board, d):
    """both flags name one cube: the dice's cube is on the board, or there is a neighbour on one side only"""
    from tests.test_gpu_predict_lookahead import cubes_of, find_cube
    mine = cubes_of(board, 1)
    d = min(max(int(d), 1), 6)
    return find_cube(mine, d, True) == find_cube(mine, d, False)


def check(ea, t, boards, dice, params, tv, model=None, what=""):
    """the kernel's Q against the model's, the pick against both, leaf_counts against the host's; returns (act, q, counts, stats)"""
    act, q, counts = ea.predict_lookahead(boards, dice, params, terminal_value=tv, return_q=True, endgame_table=t, return_leaf_counts=True)
    M = boards.shape[0]
    assert act.shape == (M, 2) and act.dtype == torch.int8 and q.shape == (M, 2, 3) and q.dtype == torch.float32
    assert counts.shape == (M, 2) and counts.dtype == torch.int16
    Qm, atol, st = model if model is not None else model_q(ea, t, boards, dice, params, tv)
    a, qk = act.cpu().numpy().astype(np.int64), q.double().cpu().numpy()
    fin = np.isfinite(Qm)
    err = float(np.abs(qk[fin] - Qm[fin]).max()) if fin.any() else 0.0
    print("%s M=%d tv=%g: max |Q - Q_model| %.3g (atol %.3g); leaf tuples by the table %d, by the critic %d" % (
        what, M, tv, err, atol, st["n_exact"].sum(), st["n_critic"].sum()))
    assert np.array_equal(qk == -np.inf, ~fin) and not np.isnan(qk).any() and not (qk == np.inf).any()
    assert err <= atol, (err, atol)
    flat = a[:, 0] * 3 + a[:, 1]
    assert np.array_equal(flat, qk.reshape(M, 6).argmax(1))          # the first row-major maximum of the RETURNED Q, exactly
    chosen = Qm.reshape(M, 6)[np.arange(M), flat]
    assert (chosen >= Qm.reshape(M, 6).max(1) - 2 * atol).all()      # every row, none excluded
    ck = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(ck[:, 0], st["n_exact"]) and np.array_equal(ck[:, 1], st["n_critic"])
    return act, q, counts, st


def sample_counts(rng, S, ka, ko):
    """a live position with exactly ka cubes against ko: distinct random numbers and cells, no agent cube on C - 1, none of the other
    side's on 0 (sample() of tests/test_gpu_endgame.py with the counts fixed)"""
    C_ = S * S
    while True:
        cells = rng.sample(range(C_), ka + ko)
        agent = tuple(sorted(zip(rng.sample(range(1, 7), ka), cells[:ka])))
        opp = tuple(sorted(zip(rng.sample(range(1, 7), ko), cells[ka:])))
        if any(c == C_ - 1 for _, c in agent) or any(c == 0 for _, c in opp):
            continue
        return agent, opp


_MIXED = {}


def mixed(ea, S):
    """the 200 mixed rows of a board, their model at terminal_value 1 and 10: computed once and left unchanged.  5x5: 100 rows of
    three cubes against two and 100 of two against three; 7x7: 200 rows of two against two (a (7, 2, 3) table covers none of them)"""
    if S not in _MIXED:
        rng = random.Random(100 + S)
        shapes = [(3, 2)] * 100 + [(2, 3)] * 100 if S == 5 else [(2, 2)] * 200
        b = torch.as_tensor(np.stack([board_of(sample_counts(rng, S, ka, ko), S) for ka, ko in shapes])).cuda().contiguous()
        d = i8(*[rng.randint(1, 6) for _ in shapes])
        params, t = pool(ea, S)["params"], tab(ea, S)
        assert not bool(t.lookup(b, d)[1].any())                       # no root is covered: the leaves are the feature
        _MIXED[S] = dict(boards=b, dice=d, params=params, model={tv: model_q(ea, t, b, d, params, tv) for tv in (1.0, 10.0)})
    return _MIXED[S]


# ---------------------------------------------------------------- 1. covered roots equal the table

@pytest.mark.parametrize("S", [5, 7])
def test_covered_roots_equal_the_table(ea, S):
    """the covered set is closed under moves, so every leaf of a covered root is covered, and the fold of exact leaves is the table's
    own recurrence: negation, max and min are exact, both sides sum in dice order and multiply by fl(1/6), and a terminal value that
    is a power of two scales exactly.  Equality of values (torch.equal): where a sum is 0 the table holds -0.0 and the fold +0.0"""
    t, params = tab(ea, S), pool(ea, S)["params"]
    rng = random.Random(S)
    pos = [sample(rng, S, *KT[S]) for _ in range(200)]
    b = torch.as_tensor(np.stack([board_of(p, S) for p in pos for _ in range(6)])).cuda().contiguous()
    d = torch.arange(1, 7, dtype=torch.int8, device="cuda").repeat(len(pos))
    a_exact, cov, q_exact = t.lookup(b, d, return_q=True)
    assert bool(cov.all())
    for tv in (1.0, 0.5):
        act, q, counts = ea.predict_lookahead(b, d, params, terminal_value=tv, return_q=True, endgame_table=t, return_leaf_counts=True)
        assert torch.equal(q, tv * q_exact) and torch.equal(act, a_exact)
        assert int(counts[:, 1].sum()) == 0 and int(counts[:, 0].sum()) > 0                # the critic valued nothing
        act2, q2 = ea.predict_lookahead(b[:12], d[:12], params, terminal_value=tv, return_q=True, endgame_table=t, plies=2)
        assert torch.equal(q2, tv * q_exact[:12]) and torch.equal(act2, a_exact[:12])


# ---------------------------------------------------------------- 2. rows without a covered leaf are the plain kernel's

@pytest.mark.parametrize("S", [5, 7])
def test_rows_without_a_covered_leaf_are_the_plain_kernels(ea, S):
    """the first 300 rows of pool().  On 7x7 none of them has a covered leaf.  On 5x5 some do: ten plies of random play on the small
    board capture often enough to come within two moves of the (5, 2, 4) table (20 of the 300 rows, 130 leaf tuples).  The rows
    without a covered leaf are found on the host (tree() and covered_np); they are at least 280 of the 300, and it is they that must
    be the plain kernel's bit for bit.  On every row the counts are the host's."""
    p, t = pool(ea, S), tab(ea, S)
    b, d = p["boards"][:300], p["dice"][:300]
    st = host_counts(b.cpu().numpy(), d.cpu().numpy(), *KT[S])
    none = torch.as_tensor(st["n_exact"] == 0).cuda()
    print("S=%d: %d of 300 pool rows without a covered leaf; %d covered leaf tuples on the others" % (S, int(none.sum()), st["n_exact"].sum()))
    assert int(none.sum()) >= 280 and (S == 5 or bool(none.all()))
    act0, q0 = ea.predict_lookahead(b, d, p["params"], return_q=True)
    act, q, counts = ea.predict_lookahead(b, d, p["params"], return_q=True, endgame_table=t, return_leaf_counts=True)
    ck = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(ck[:, 0], st["n_exact"]) and np.array_equal(ck[:, 1], st["n_critic"]) and int(counts[none, 0].abs().sum()) == 0
    assert torch.equal(act[none], act0[none]) and torch.equal(bits(q[none]), bits(q0[none]))


# ---------------------------------------------------------------- 3. mixed rows against the float64 model

@pytest.mark.parametrize("S", [5, 7])
def test_the_mixed_rows_hold_both_kinds_of_leaf(ea, S):
    st = mixed(ea, S)["model"][1.0][2]
    both = (st["n_exact"] > 0) & (st["n_critic"] > 0)
    print("S=%d: %d of 200 rows have both kinds of leaf, %d a (root, d1) reply set with both" % (S, both.sum(), st["mixed_set"].sum()))
    assert both.sum() >= 40 and st["mixed_set"].sum() >= 25


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("tv", [1.0, 10.0])
def test_mixed_rows_against_the_model(ea, S, tv):
    mx = mixed(ea, S)
    st = mx["model"][tv][2]
    assert ((st["n_exact"] > 0) & (st["n_critic"] > 0)).sum() >= 40 and st["mixed_set"].sum() >= 25     # counted before it compares
    check(ea, tab(ea, S), mx["boards"], mx["dice"], mx["params"], tv, model=mx["model"][tv], what="S=%d mixed" % S)


# ---------------------------------------------------------------- 4. leaf_counts against the public calls

@pytest.mark.parametrize("S", [5, 7])
def test_leaf_counts_against_the_public_calls(ea, S):
    mx, t = mixed(ea, S), tab(ea, S)
    b, d, params = mx["boards"], mx["dice"], mx["params"]
    M = b.shape[0]
    act, q, counts = ea.predict_lookahead(b, d, params, return_q=True, endgame_table=t, return_leaf_counts=True)
    lb, ld, kind = ea.lookahead_expand(b, d)
    leaf = kind == 2
    assert torch.equal(counts.sum(1).long(), leaf.sum(1))
    first = lb.reshape(M, 108, 6, S, S)[:, :, 0].reshape(M * 108, S, S).contiguous()        # the tuple's board (under d2 = 1)
    cov = t.lookup(first, torch.ones(M * 108, dtype=torch.int8, device="cuda"))[1].reshape(M, 108)
    assert torch.equal(counts[:, 0].long(), (cov & leaf).sum(1))
    act1, q1 = ea.predict_lookahead(b, d, params, return_q=True, endgame_table=t)           # leaf_counts NULL: the same q
    assert torch.equal(act1, act) and torch.equal(bits(q1), bits(q))


# ---------------------------------------------------------------- 5. independence of the batch

@pytest.mark.parametrize("S", [5, 7])
def test_the_batch_does_not_matter(ea, S):
    mx, t = mixed(ea, S), tab(ea, S)
    b, d, params = mx["boards"], mx["dice"], mx["params"]
    call = lambda bb, dd, **kw: ea.predict_lookahead(bb, dd, params, endgame_table=t, **kw)   # noqa: E731
    act, q, counts = call(b, d, return_q=True, return_leaf_counts=True)
    parts = [call(b[i:j], d[i:j], return_q=True, return_leaf_counts=True) for i, j in ((0, 7), (7, 71), (71, 200))]
    for k, whole in enumerate((act, q, counts)):
        got = torch.cat([x[k] for x in parts])
        assert torch.equal(bits(whole), bits(got)) if whole.dtype == torch.float32 else torch.equal(whole, got)
    for M in (1, 31, 33):
        a, qq = call(b[:M], d[:M], return_q=True)
        assert torch.equal(a, act[:M]) and torch.equal(bits(qq), bits(q[:M]))
    assert torch.equal(call(b, d), act)                                                      # q NULL: the same actions
    assert torch.equal(call(b[0], d[:1]), act[:1])                                           # a single [S, S] board


@pytest.mark.parametrize("S", [5, 7])
def test_degenerate_rows_among_live_ones_and_dice_out_of_range(ea, S):
    mx, t = mixed(ea, S), tab(ea, S)
    M = 40
    b, d, params = mx["boards"][:M].clone(), mx["dice"][:M].clone(), mx["params"]
    call = lambda bb, dd: ea.predict_lookahead(bb, dd, params, return_q=True, endgame_table=t, return_leaf_counts=True)   # noqa: E731
    act0, q0, c0 = call(b, d)
    dead = boards_of(S, {(S - 1, S - 1): 3, (0, 1): -2}, {(0, 0): -1, (2, 2): 4}, {(2, 2): -3}, {(2, 2): 3}, {})
    rows = [0, 7, 31, 32, 39]       # agent on the far corner, opponent on (0, 0), no agent cube, no opposing cube, an empty board
    b[rows] = dead
    act, q, c = call(b, d)
    live = torch.ones(M, dtype=torch.bool, device="cuda")
    live[rows] = False
    assert torch.isneginf(q[rows]).all() and int(act[rows].abs().sum()) == 0 and int(c[rows].abs().sum()) == 0
    assert torch.equal(bits(q[live]), bits(q0[live])) and torch.equal(act[live], act0[live]) and torch.equal(c[live], c0[live])
    lo, hi = call(b, torch.zeros_like(d)), call(b, torch.full_like(d, 7))
    one, six = call(b, torch.ones_like(d)), call(b, torch.full_like(d, 6))
    assert torch.equal(lo[0], one[0]) and torch.equal(bits(lo[1]), bits(one[1])) and torch.equal(lo[2], one[2])
    assert torch.equal(hi[0], six[0]) and torch.equal(bits(hi[1]), bits(six[1])) and torch.equal(hi[2], six[2])
    assert not torch.equal(bits(one[1]), bits(six[1]))


# ---------------------------------------------------------------- 6. constructed positions

@pytest.mark.parametrize("S", [5, 7])
def test_constructed_positions(ea, S):
    t, params = tab(ea, S), pool(ea, S)["params"]
    E = S - 1
    if S == 5:      # K = 2, T = 4
        specs = [
            # 0 three against two, not covered; the moving cube 3 captures nothing, and every reply there is captures an agent cube:
            #   -1 on (0, 2) can only go left onto cube 1, -2 on (2, 0) only up onto cube 2: every leaf is two against two
            ({(0, 1): 1, (1, 0): 2, (2, 2): 3, (0, 2): -1, (2, 0): -2}, 3),
            # 1 three against one, nothing is captured: every leaf has K + 1 agent cubes (4 in all = T)
            ({(1, 1): 1, (1, 3): 2, (3, 1): 3, (E, E): -1}, 1),
            # 2 three against two, nothing is captured: every leaf has T + 1 cubes
            ({(1, 1): 1, (1, 3): 2, (3, 1): 3, (E, E): -1, (0, E): -2}, 1),
            # 3 two against three: -1 going left takes its own -2, and only those leaves are two against two
            ({(1, 1): 1, (0, 3): 2, (E, E): -1, (E, E - 1): -2, (2, E): -3}, 1),
            # 4 cube 1 twice on the agent's side (two against two otherwise): no position of the table's
            ({(1, 1): 1, (2, 2): 1, (E, E): -1, (E - 1, E): -2}, 1),
        ]
    else:           # K = 2, T = 3
        specs = [
            # 0 two against two, not covered; -1 on (0, 2) can only go left onto cube 1, -2 on (0, 3) only left onto its own -1
            ({(0, 1): 1, (2, 2): 3, (0, 2): -1, (0, 3): -2}, 3),
            # 1 three against one: K + 1 agent cubes
            ({(1, 1): 1, (1, 3): 2, (3, 1): 3, (E, E): -1}, 1),
            # 2 two against two, nothing is captured: T + 1 cubes with at most K a side
            ({(1, 1): 1, (1, 3): 2, (E, E): -1, (E, 2): -2}, 1),
            # 3 one against three: -1 going left takes its own -2, and only those leaves are one against two
            ({(1, 1): 1, (E, E): -1, (E, E - 1): -2, (2, E): -3}, 1),
            # 4 cube 1 twice on the agent's side (two against one otherwise): no position of the table's
            ({(1, 1): 1, (2, 2): 1, (E, E): -1}, 1),
        ]
    b = boards_of(S, *[s for s, _ in specs])
    d = i8(*[x for _, x in specs])
    assert not bool(t.lookup(b, d)[1].any())                              # no root is covered
    act0, q0 = ea.predict_lookahead(b, d, params, return_q=True)
    act, q, counts, st = check(ea, t, b[:4], d[:4], params, 1.0, what="S=%d constructed" % S)
    c = counts.cpu().numpy()
    assert c[0, 0] > 0 and c[0, 1] == 0                                   # every leaf by the table, none by the critic
    assert c[1, 0] == 0 and c[1, 1] > 0 and c[2, 0] == 0 and c[2, 1] > 0
    assert torch.equal(bits(q[1:3]), bits(q0[1:3])) and torch.equal(act[1:3], act0[1:3])
    assert c[3, 0] > 0 and c[3, 1] > 0
    act4, q4, c4 = ea.predict_lookahead(b[4:], d[4:], params, return_q=True, endgame_table=t, return_leaf_counts=True)
    assert int(c4[0, 0]) == 0 and int(c4[0, 1]) > 0
    assert torch.equal(bits(q4), bits(q0[4:])) and torch.equal(act4, act0[4:])


# ---------------------------------------------------------------- 7. guard zones

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    M = 33
    mx, t = mixed(ea, S), tab(ea, S)
    alloc = GuardedAllocator()
    b = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards", offset=1)
    d = alloc.zeros((M,), dtype=torch.int8, tag="dice", offset=1)
    params = alloc.zeros((mx["params"].numel(),), dtype=torch.float32, tag="params")
    tb = alloc.zeros((t.table.numel(),), dtype=torch.float32, tag="table", offset=4 if S == 5 else 0)   # once 4 bytes past a 16-byte boundary
    assert tb.data_ptr() % 16 == (4 if S == 5 else 0)
    b.copy_(mx["boards"][:M]); d.copy_(mx["dice"][:M]); params.copy_(mx["params"]); tb.copy_(t.table)
    guarded = ea.EndgameTable(S, t.max_cubes, t.max_total, tb)
    ref = ea.predict_lookahead(mx["boards"][:M], mx["dice"][:M], mx["params"], return_q=True, endgame_table=t, return_leaf_counts=True)
    with alloc.patch(tag="outputs"):            # predict_lookahead's torch.zeros outputs come out of the guarded allocator
        act, q, counts = ea.predict_lookahead(b, d, params, return_q=True, endgame_table=guarded, return_leaf_counts=True)
        act1 = ea.predict_lookahead(b, d, params, endgame_table=guarded)
    assert all(alloc.owns(x) for x in (act, q, counts, act1))
    torch.cuda.synchronize()
    alloc.check("S=%d M=%d" % (S, M))
    assert torch.equal(act, ref[0]) and torch.equal(bits(q), bits(ref[1])) and torch.equal(counts, ref[2]) and torch.equal(act1, ref[0])
    assert int(counts[:, 0].sum()) > 0 and int(counts[:, 1].sum()) > 0
    assert torch.equal(b, mx["boards"][:M]) and torch.equal(d, mx["dice"][:M]) and torch.equal(params, mx["params"])   # only read
    assert torch.equal(bits(tb), bits(t.table))


# ---------------------------------------------------------------- 8. compositions, bit for bit

@pytest.mark.parametrize("S", [5, 7])
def test_predict_puct_with_a_table_is_the_public_calls_composed(ea, S):
    mx, t = mixed(ea, S), tab(ea, S)
    M, sims, tv = 33, 16, 0.75
    rng = random.Random(50 + S)                 # 17 mixed rows, then 16 positions the table covers: their roots are replaced at once
    b = torch.cat([mx["boards"][:17], torch.as_tensor(np.stack([board_of(sample(rng, S, *KT[S]), S) for _ in range(16)])).cuda()]).contiguous()
    d, params = torch.cat([mx["dice"][:17], i8(*[rng.randint(1, 6) for _ in range(16)])]).contiguous(), mx["params"]
    got = ea.predict_puct(b, d, params, sims=sims, terminal_value=tv, return_visits=True, return_q=True, return_value=True, endgame_table=t)
    tree_, lb, ld = ea.puct_begin(b, d, sims)
    replaced = 0
    for _ in range(sims + 1):
        _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        _, cov, qe = t.lookup(lb, ld, return_q=True)
        replaced += int(cov.sum())
        value = torch.where(cov, tv * qe.reshape(M, 6).max(1).values, value)
        ea.puct_advance(tree_, logits, value, lb, ld, sims, terminal_value=tv)
    want = ea.puct_result(tree_, S, sims, return_visits=True, return_q=True, return_value=True)
    print("S=%d puct: %d of %d leaf evaluations by the table" % (S, replaced, M * (sims + 1)))
    assert replaced > 0
    for x, y in zip(got, want):
        assert torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)
    plain = ea.predict_puct(b, d, params, sims=sims, terminal_value=tv, return_q=True)
    assert not torch.equal(bits(plain[1]), bits(got[2]))                   # the table is read: the search is another one


@pytest.mark.parametrize("search", ["lookahead", "lookahead2", "puct"])
def test_one_distill_update_with_exact_leaves_is_the_public_calls_composed(ea, search):
    """the pattern of test_one_distill_update_with_the_table_is_the_public_calls_composed: every second lane goes on from a sampled
    few-cube position, so that the searches meet covered leaves (and covered roots, whose q is still replaced afterwards)"""
    from ewn_gym_amd._lib import EwnA2cHyper, check as rc_check
    from ewn_gym_amd.distill import SearchDistillTrainer
    from ewn_gym_amd.vec_env import _ptr, _stream
    S, N, K, tv = 5, 64, 2, 0.75
    t = tab(ea, S)
    kw = dict(search="puct", sims=8) if search == "puct" else dict(plies=2 if search == "lookahead2" else 1)
    tr = SearchDistillTrainer(make_env(ea, N, S), n_steps=K, seed=5, endgame_table=t, terminal_value=tv, endgame_leaves=True, **kw)
    params, sq = tr.params.clone(), torch.zeros_like(tr.params)
    few_cube_lanes(tr.env, 3, 5, 7)             # up to three cubes a side and five in all: around the (5, 2, 4) table's edge
    tr.collect_and_update()
    env = make_env(ea, N, S)
    few_cube_lanes(env, 3, 5, 7)
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, params, traj=traj, noise_key=tr.noise_key)
    assert torch.equal(traj["record"], tr.traj["record"])
    b = traj["obs_board"][:K].reshape(K * N, S, S).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    _, cov, qe = t.lookup(b, d, return_q=True)
    assert 0 < int(cov.sum()) < K * N
    if search == "puct":
        _, visits, q, value = ea.predict_puct(b, d, params, sims=8, terminal_value=tv, return_visits=True, return_q=True, return_value=True,
                                              endgame_table=t)
        from ewn_gym_amd.distill import puct_targets
        tp, tvv, w = puct_targets(visits, q, value, tv)
        e_pi, e_value, e_weight = ea.lookahead_targets(tv * qe, 0.0)
        tp = torch.where(cov[:, None], e_pi, tp)
        tvv, w = torch.where(cov, e_value, tvv), torch.where(cov, e_weight, w)
    else:
        _, q, counts = ea.predict_lookahead(b, d, params, terminal_value=tv, return_q=True, endgame_table=t, return_leaf_counts=True) \
            if search == "lookahead" else ea.predict_lookahead(b, d, params, terminal_value=tv, return_q=True, endgame_table=t, plies=2) + (None,)
        if counts is not None:
            assert int(counts[~cov, 0].sum()) > 0                             # rows off the table whose leaves are on it
        q = torch.where(cov[:, None, None], tv * qe, q)
        tp, tvv, w = ea.lookahead_targets(q, 0.0)
    grad = ea.sup_grad(b, d, tp, tvv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    norm = torch.zeros(1, device="cuda")
    rc_check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    assert torch.equal(bits(params), bits(tr.params)) and torch.equal(bits(sq), bits(tr.sq_avg))
    # without endgame_leaves the search does not see the table: another gradient on these lanes
    off = SearchDistillTrainer(make_env(ea, N, S), n_steps=K, seed=5, endgame_table=t, terminal_value=tv, **kw)
    few_cube_lanes(off.env, 3, 5, 7)
    off.collect_and_update()
    assert not torch.equal(bits(off.grad), bits(tr.grad))


def test_value_search_agent_with_a_table_on_the_drop_in_env(ea, tmp_path):
    from classical_policies import PuctAgent, ValueSearchAgent
    from envs import EinsteinWuerfeltNichtEnv
    p, t = pool(ea, 5), tab(ea, 5)
    agent = ValueSearchAgent(p["model"], board_size=5, endgame_table=t)
    assert agent.endgame_table is t and ValueSearchAgent(p["model"], board_size=5).endgame_table is None
    env = EinsteinWuerfeltNichtEnv(board_size=5, seed=3)
    rng = random.Random(9)
    for ep in range(4):
        obs, _ = env.reset(seed=ep)
        env.board[:] = board_of(sample_counts(rng, 5, 3, 2), 5)          # in place: obs["board"] is the env's board
        env._push_board()
        for _ in range(6):
            action, state = agent.predict(obs)
            assert state is None and isinstance(action, np.ndarray) and action.shape == (2,)
            bb, dd = obs["board"].astype(np.int8)[None], [obs["dice_roll"]]
            batch, q = agent.predict_batch(bb, dd, return_q=True)
            want = ea.predict_lookahead(torch.as_tensor(bb).cuda(), i8(int(dd[0])), p["params"], return_q=True, endgame_table=t)
            assert np.array_equal(action, batch[0].cpu().numpy()) and torch.equal(batch, want[0]) and torch.equal(bits(q), bits(want[1]))
            assert np.isfinite(q[0, action[0], action[1]].item())
            obs, _, terminated, truncated, _ = env.step(action)
            if terminated or truncated:
                break
    mx = mixed(ea, 5)
    b, d = mx["boards"], mx["dice"]
    assert torch.equal(agent.policy_fn()(b, d, 5), ea.predict_lookahead(b, d, p["params"], endgame_table=t))
    two = ValueSearchAgent(p["params"], board_size=5, terminal_value=0.5, plies=2, endgame_table=t)
    assert torch.equal(two.predict_batch(b[:8], d[:8]), ea.predict_lookahead(b[:8], d[:8], p["params"], terminal_value=0.5, plies=2, endgame_table=t))
    path, small = str(tmp_path / "eg.pt"), table(ea, 5, 1, 2)
    small.save(path)
    pu = PuctAgent(p["params"], board_size=5, sims=8, endgame_table=path)   # a path: loaded once
    assert torch.equal(bits(pu.endgame_table.table), bits(small.table))
    assert torch.equal(pu.predict_batch(b[:33], d[:33]), ea.predict_puct(b[:33], d[:33], p["params"], sims=8, endgame_table=small))
    with pytest.raises(ValueError, match="the table is for 7x7 boards, the agent plays 5x5"):
        ValueSearchAgent(p["params"], board_size=5, endgame_table=tab(ea, 7))
    with pytest.raises(ValueError, match="must be an EndgameTable or the path"):
        PuctAgent(p["params"], board_size=5, endgame_table=t.table)


def test_lookahead_with_exact_leaves_in_the_tournament(ea):
    from ewn_gym_amd.tournament import evaluate
    m, t = pool(ea, 5)["model"], tab(ea, 5)
    spec = {"kind": "mlp_lookahead", "model": m, "endgame_table": t}
    r1, r2 = evaluate(spec, {"kind": "random"}, num=64), evaluate(spec, {"kind": "random"}, num=64)
    assert r1["engine"] == "ewn_step" and r1["episodes"] == 64 and int((r1["lengths"] > 0).sum()) == 64
    assert torch.equal(r1["scores"], r2["scores"]) and torch.equal(r1["lengths"], r2["lengths"])
    assert bool((r1["scores"] != 0).all())                                # every episode ended: no illegal-move stall
    r3 = evaluate({"kind": "mlp_puct", "model": m, "sims": 4, "endgame_table": t}, {"kind": "random"}, num=16)
    assert r3["episodes"] == 16 and bool((r3["scores"] != 0).all())
    from ewn_gym_amd.tournament import evaluate_model
    rows = evaluate_model(m, names=("random",), num=64, lookahead=1, endgame_table=t, endgame_leaves=True)
    assert list(rows) == ["model vs random", "lookahead vs random", "lookahead + exact leaves vs random"]
    assert rows["lookahead + exact leaves vs random"]["wins"] == r1["wins"] and rows["lookahead + exact leaves vs random"]["episodes"] == 64
    assert list(evaluate_model(m, names=("random",), num=16, lookahead=1)) == ["model vs random", "lookahead vs random"]   # today's rows
