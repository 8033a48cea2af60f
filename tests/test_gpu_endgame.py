"""Exact endgame values (ewn_endgame_build / ewn_endgame_lookup, EndgameTable, EndgameAgent) against a memoised
Python model of the definition, written from the rules:
    E(b) = fl((m_1 + ... + m_6) * fl(1/6)),  m_d = max over the moves (f, r) that stay on the board of G,
    G = +1 where the move wins, else -E(flip(b1)).
The model carries every value twice: in float64, and in numpy float32 with exactly those operations.  The kernels must give the
float32 model bit for bit, and lie within 7 * 2^-24 * Phi(b) of the float64 one: a level costs at most five additions and one
multiply of fp32 rounding on operands of at most 6, scaled by 1/6; max and the mean do not amplify a child's error, and a position
is at most Phi(b) levels deep."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402

F32 = np.float32
SIXTH = F32(1.0) / F32(6.0)
NINF = float("-inf")


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


# ---------------------------------------------------------------- the model of the definition
# a position: (agent, opp), each a sorted tuple of (cube number, cell); the agent is TOP_LEFT and moves right, down, down-right

def find_cube(present, d, larger):
    """find_cube_to_move on the set of cube numbers a player has: the dice's cube, else the nearest in the asked direction, else the other"""
    if d in present:
        return d
    up = [k for k in range(d + 1, 7) if k in present]
    dn = [k for k in range(d - 1, 0, -1) if k in present]
    first, second = (up, dn) if larger else (dn, up)
    return (first or second)[0]


def moves_of(pos, S, k):
    """[(r, "win" | the position after the move, flipped: seen by the other side)] of the agent's cube k, the directions that stay on
    the board; the move captures whatever stands on the target"""
    agent, opp = pos
    C_ = S * S
    x, y = divmod(dict(agent)[k], S)
    out = []
    for r, (dx, dy) in enumerate(((0, 1), (1, 0), (1, 1))):
        nx, ny = x + dx, y + dy
        if nx >= S or ny >= S:
            continue
        dst = nx * S + ny
        a1 = tuple(sorted([(j, c) for j, c in agent if j != k and c != dst] + [(k, dst)]))
        o1 = tuple((j, c) for j, c in opp if c != dst)
        if dst == C_ - 1 or not o1:
            out.append((r, "win"))
        else:
            out.append((r, (tuple((j, C_ - 1 - c) for j, c in o1), tuple((j, C_ - 1 - c) for j, c in a1))))
    return out


class Model:
    def __init__(self, S):
        self.S, self.memo = S, {}

    def cube_best(self, pos, k):
        """{r: (G float64, G float32)} of cube k"""
        return {r: ((1.0, F32(1.0)) if nxt == "win" else tuple(-v for v in self.E(nxt))) for r, nxt in moves_of(pos, self.S, k)}

    def q(self, pos, d):
        """(q float64 [2, 3], q float32 [2, 3]) under the dice d, -inf where the move leaves the board"""
        mine = {k for k, _ in pos[0]}
        q64, q32 = np.full((2, 3), NINF), np.full((2, 3), NINF, F32)
        for f in (0, 1):
            for r, (g64, g32) in self.cube_best(pos, find_cube(mine, d, f == 1)).items():
                q64[f, r], q32[f, r] = g64, g32
        return q64, q32

    def E(self, pos):
        if pos not in self.memo:
            best = {k: self.cube_best(pos, k) for k, _ in pos[0]}
            b64 = {k: max(g[0] for g in v.values()) for k, v in best.items()}
            b32 = {k: max(g[1] for g in v.values()) for k, v in best.items()}
            mine = set(best)
            s64, s32 = 0.0, None
            for d in range(1, 7):
                k0, k1 = find_cube(mine, d, False), find_cube(mine, d, True)
                s64 += max(b64[k0], b64[k1])
                m = max(b32[k0], b32[k1])
                s32 = m if s32 is None else F32(s32 + m)
            self.memo[pos] = (s64 / 6.0, F32(s32 * SIXTH))
        return self.memo[pos]


_MODELS = {}


def model(S):
    return _MODELS.setdefault(S, Model(S))


def board_of(pos, S):
    b = np.zeros(S * S, np.int8)
    for k, c in pos[0]:
        b[c] = k
    for k, c in pos[1]:
        b[c] = -k
    return b.reshape(S, S)


def phi(pos, S):
    return sum(2 * (S - 1) - sum(divmod(c, S)) for _, c in pos[0]) + sum(sum(divmod(c, S)) for _, c in pos[1])


def sample(rng, S, K, T):
    """the issue's sampling: cube counts uniform in 1..K a side (redrawn over T in all), distinct random numbers and cells, rejected
    with an agent cube on C - 1 or an opposing cube on 0"""
    C_ = S * S
    while True:
        ka, ko = rng.randint(1, K), rng.randint(1, K)
        if ka + ko > T:
            continue
        cells = rng.sample(range(C_), ka + ko)
        agent = tuple(sorted(zip(rng.sample(range(1, 7), ka), cells[:ka])))
        opp = tuple(sorted(zip(rng.sample(range(1, 7), ko), cells[ka:])))
        if any(c == C_ - 1 for _, c in agent) or any(c == 0 for _, c in opp):
            continue
        return agent, opp


def covered_np(boards, K, T):
    """the definition's coverage test on int8 [M, S, S]"""
    b = boards.reshape(boards.shape[0], -1).astype(np.int64)
    ka, ko = (b > 0).sum(1), (b < 0).sum(1)
    live = (b[:, -1] <= 0) & (b[:, 0] >= 0) & (np.abs(b).max(1) <= 6)
    return live & (ka >= 1) & (ko >= 1) & (ka <= K) & (ko <= K) & (ka + ko <= T)


_TABLES = {}


def table(ea, S, K, T):
    """built once per module and left unchanged"""
    if (S, K, T) not in _TABLES:
        _TABLES[(S, K, T)] = ea.EndgameTable.build(S, K, T)
    return _TABLES[(S, K, T)]


def check_positions(ea, S, K, T, positions, what):
    """every dice of every position: value and q against both models, the action against the returned q"""
    t, mod = table(ea, S, K, T), model(S)
    b = torch.as_tensor(np.stack([board_of(p, S) for p in positions for _ in range(6)])).cuda()
    d = torch.arange(1, 7, dtype=torch.int8, device="cuda").repeat(len(positions))
    act, cov, q, val = t.lookup(b, d, return_q=True, return_value=True)
    M = 6 * len(positions)
    assert act.shape == (M, 2) and act.dtype == torch.int8 and cov.dtype == torch.bool and q.shape == (M, 2, 3) and val.shape == (M,)
    assert bool(cov.all())
    qk, vk, a = q.cpu().numpy(), val.cpu().numpy(), act.cpu().numpy().astype(np.int64)
    qs = [mod.q(p, dd) for p in positions for dd in range(1, 7)]
    q64, q32 = np.stack([x[0] for x in qs]), np.stack([x[1] for x in qs])
    v64 = np.repeat([mod.E(p)[0] for p in positions], 6)
    v32 = np.repeat(np.array([mod.E(p)[1] for p in positions], F32), 6)
    tol = 7 * 2.0 ** -24 * np.repeat([phi(p, S) for p in positions], 6)
    fin = np.isfinite(q64)
    err_v = np.abs(vk.astype(np.float64) - v64)
    err_q = np.where(fin, np.abs(np.where(fin, qk, 0).astype(np.float64) - np.where(fin, q64, 0)), 0.0)
    print("%s (%d, %d, %d): %d rows, max |value - f64| %.3g, max |q - f64| %.3g (smallest bound %.3g), f32 model against f64 %.3g" % (
        what, S, K, T, M, err_v.max(), err_q.max(), tol.min(), np.abs(v32.astype(np.float64) - v64).max()))
    assert np.array_equal(qk == NINF, ~fin) and not np.isnan(qk).any() and not np.isnan(vk).any()
    assert np.array_equal(vk.view(np.int32), v32.view(np.int32))                                  # bit for bit, every row
    assert np.array_equal(qk.view(np.int32), q32.view(np.int32))
    assert (err_v <= tol).all() and (err_q <= tol[:, None, None]).all()
    assert np.array_equal(a[:, 0] * 3 + a[:, 1], qk.reshape(M, 6).argmax(1))                      # the first maximum of the RETURNED q
    return b, d


# ---------------------------------------------------------------- 1. values and q against the model

def test_the_models_move_lists_agree_with_the_oracle():
    from oracle import pyoracle
    rng = random.Random(1)
    S = 5
    ps = [sample(rng, S, 3, 6) for _ in range(64)]
    b = np.stack([board_of(p, S) for p in ps])
    d = np.array([rng.randint(1, 6) for _ in ps], np.int8)
    acts, n, cs, cl, _ = pyoracle.legal_actions(b, d, player=1)
    for m, p in enumerate(ps):
        have = {k for k, _ in p[0]}
        cube = (find_cube(have, int(d[m]), False), find_cube(have, int(d[m]), True))
        assert cube == (abs(int(cs[m])), abs(int(cl[m])))
        mine = {(cube[f], r) for f in (0, 1) for r, _ in moves_of(p, S, cube[f])}
        assert mine == {(cube[int(x[0])], int(x[1])) for x in acts[m, :int(n[m])]}


@pytest.mark.parametrize("S,K,T,n", [(3, 2, 4, 2000), (3, 3, 4, 500), (4, 2, 4, 300), (5, 1, 2, 500)])
def test_values_and_q_against_the_model(ea, S, K, T, n):
    rng = random.Random(100 * S + 10 * K + T)
    check_positions(ea, S, K, T, [sample(rng, S, K, T) for _ in range(n)], "sampled")
    t = table(ea, S, K, T)
    assert (t.board_size, t.max_cubes, t.max_total, t.levels) == (S, K, T, 2 * T * (S - 1))
    assert t.table.dtype == torch.float32 and t.table.numel() * 4 == ea.EndgameTable.table_bytes(S, K, T)


# ---------------------------------------------------------------- 2. the 5x5 table every 5x5 test below uses

def mixed_rows(ea, M):
    """M observations of a RandomAgent rollout with auto-reset; every 7th replaced by a sampled covered position, every 97th by a
    finished one"""
    p = pool(ea, 5)
    b, d = p["boards"][:M].clone(), p["dice"][:M].clone()
    rng = random.Random(7)
    for m in range(0, M, 7):
        b[m] = torch.as_tensor(board_of(sample(rng, 5, 2, 4), 5)).cuda()
    done = np.zeros((5, 5), np.int8)
    done[4, 4], done[0, 1] = 3, -2
    for m in range(0, M, 97):
        b[m] = torch.as_tensor(done).cuda()
    return b.contiguous(), d.contiguous()


def test_5x5_sampled_against_the_model(ea):
    rng = random.Random(524)
    check_positions(ea, 5, 2, 4, [sample(rng, 5, 2, 4) for _ in range(60)], "sampled")


@pytest.mark.parametrize("M", [1, 31, 33, 300])
def test_5x5_rollout_rows(ea, M):
    t = table(ea, 5, 2, 4)
    b, d = mixed_rows(ea, M)
    act, cov, q, val = t.lookup(b, d, return_q=True, return_value=True)
    want = covered_np(b.cpu().numpy(), 2, 4)
    assert np.array_equal(cov.cpu().numpy(), want)
    if M >= 31:
        assert want.any() and not want.all()
    un = ~cov
    assert bool(torch.isneginf(q[un]).all()) and int(act[un].abs().sum()) == 0 and int(bits(val[un]).abs().sum()) == 0
    assert bool(torch.isfinite(val[cov]).all()) and bool((val[cov].abs() <= 1).all())
    qf = q.reshape(M, 6)
    assert torch.equal(act[:, 0].long() * 3 + act[:, 1].long(), qf.argmax(1))
    # the covered rows against the model
    mod = model(5)
    for m in np.nonzero(want)[0][:40]:
        bb = b[m].cpu().numpy().reshape(-1)
        pos = (tuple(sorted((int(v), c) for c, v in enumerate(bb) if v > 0)), tuple(sorted((int(-v), c) for c, v in enumerate(bb) if v < 0)))
        assert np.array_equal(q[m].cpu().numpy().view(np.int32), mod.q(pos, int(d[m]))[1].view(np.int32))
        assert val[m].cpu().numpy().view(np.int32) == mod.E(pos)[1].view(np.int32)
    if M == 300:
        parts = [t.lookup(b[i:j], d[i:j], return_q=True, return_value=True) for i, j in ((0, 7), (7, 71), (71, 300))]
        for k, whole in enumerate((act, cov, q, val)):
            cat = torch.cat([x[k] for x in parts])
            assert torch.equal(whole, cat) if whole.dtype != torch.float32 else torch.equal(bits(whole), bits(cat))
        a0, c0 = t.lookup(b, d)                                                                  # q, value NULL: the same actions
        assert torch.equal(a0, act) and torch.equal(c0, cov)
        assert torch.equal(bits(t.value(b)), bits(val))
        a1 = torch.zeros((M, 2), dtype=torch.int8, device="cuda")                                 # covered NULL too
        from ewn_gym_amd._lib import check, load
        from ewn_gym_amd.vec_env import _ptr, _stream
        check(load().ewn_endgame_lookup(5, 2, 4, _ptr(t.table), M, _ptr(b), _ptr(d), _ptr(a1), None, None, None, _stream()), "lookup")
        assert torch.equal(a1, act)


# ---------------------------------------------------------------- 3. constructed positions

def boards_of(S, *specs):
    out = np.zeros((len(specs), S, S), np.int8)
    for i, s in enumerate(specs):
        for (x, y), v in s.items():
            out[i, x, y] = v
    return torch.as_tensor(out).cuda()


def i8(*v):
    return torch.tensor(v, dtype=torch.int8, device="cuda")


@pytest.mark.parametrize("S", [5, 3])
def test_a_step_from_the_corner(ea, S):
    t = table(ea, S, 2, 4)
    E_ = S - 1
    b = boards_of(S, {(E_ - 1, E_ - 1): 3, (0, E_): -2}, {(E_, E_ - 1): 1, (0, 1): -4}, {(E_ - 1, E_): 6, (1, 0): -1})
    act, cov, q, val = t.lookup(b, i8(3, 5, 2), return_q=True, return_value=True)
    assert bool(cov.all()) and bool((val == 1.0).all())
    q = q.cpu().numpy()
    assert q[0, 0, 2] == 1.0 and q[0, 1, 2] == 1.0 and q[0].max() == 1.0
    assert q[1, 0, 0] == 1.0 and np.isneginf(q[1, :, 1:]).all() and tuple(act[1].tolist()) == (0, 0)
    assert q[2, 0, 1] == 1.0 and np.isneginf(q[2, :, [0, 2]]).all() and tuple(act[2].tolist()) == (0, 1)


def test_constructed_5x5(ea):
    t = table(ea, 5, 2, 4)
    specs = [
        ({(1, 1): 3, (2, 2): -4}, 6),                              # 0 the diagonal captures the last opposing cube: it wins
        ({(0, 0): 1, (0, 1): 2, (1, 0): -3}, 1),                   # 1 cube 1: down takes the last opposing cube; right takes the own cube 2
        ({(0, 0): 1, (0, 1): 2, (1, 2): -3, (2, 1): -5}, 1),       # 2 cube 1's right captures the own cube 2
        ({(0, 2): 4, (2, 0): 5, (3, 4): -1}, 2),                   # 3 dice 2, cubes 4 and 5: both flags name cube 4
        ({(0, 2): 2, (2, 0): 5, (3, 4): -1}, 3),                   # 4 dice 3, cubes 2 and 5: the flags differ
    ]
    b, d = boards_of(5, *[s for s, _ in specs]), i8(*[x for _, x in specs])
    act, cov, q, val = t.lookup(b, d, return_q=True, return_value=True)
    assert bool(cov.all())
    qn = q.cpu().numpy()
    assert qn[0, 0, 2] == 1.0 and tuple(act[0].tolist()) == (0, 2)
    assert qn[1, 0, 1] == 1.0 and tuple(act[1].tolist()) == (0, 1) and np.isfinite(qn[1, 0, 0]) and qn[1, 0, 0] < 1.0
    assert np.isfinite(qn[2]).all()
    assert torch.equal(bits(q[3, 0]), bits(q[3, 1])) and int(act[3, 0]) == 0                      # one cube under both flags; the first wins
    assert not np.array_equal(qn[4, 0], qn[4, 1])
    # an own capture as the only move at all: cube 1 on the last row next to its own cube 2
    only = boards_of(5, {(4, 2): 1, (4, 3): 2, (0, 1): -1})
    a, c, qq, v = t.lookup(only, i8(1), return_q=True, return_value=True)
    assert np.array_equal(qq[0].cpu().numpy().view(np.int32), model(5).q((((1, 22), (2, 23)), ((1, 1),)), 1)[1].view(np.int32))
    assert np.isneginf(qq[0, :, 1:].cpu().numpy()).all() and tuple(a[0].tolist()) == (0, 0)
    # dice 0 and 7 are dice 1 and 6
    bb, _ = mixed_rows(ea, 64)
    for lo, ref in ((0, 1), (7, 6), (-5, 1), (100, 6)):
        x, y = t.lookup(bb, torch.full((64,), lo, dtype=torch.int8, device="cuda"), return_q=True), t.lookup(bb, torch.full((64,), ref, dtype=torch.int8, device="cuda"), return_q=True)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(bits(x[2]), bits(y[2]))


def test_the_only_move_that_keeps_the_win_captures_an_own_cube(ea):
    """Cube 1 on (2, 2), its own cube 6 on (3, 3), the last opposing cube two moves from (0, 0), dice 1.  The diagonal takes the own
    cube: cube 1 is then alone, one step from the corner, and moves whatever the next dice is: q = +1.  Right or down keep cube 6, and
    a next dice of 1 then moves cube 1 (two steps from the corner) while the opponent arrives: q = 5/6 - 1/6.  (A position whose other
    moves all have q = -1 was looked for among 12 000 sampled positions of 3x3, 4x4 and 5x5 with the model and not found: an own
    capture only changes which cube the dice selects, and where that matters the other moves keep a chance.)"""
    pos = (((1, 12), (6, 18)), ((3, 2),))
    q64, q32 = model(5).q(pos, 1)
    assert q64[0, 2] == 1.0 and (q64[0, :2] < 0.7).all() and np.array_equal(q64[0], q64[1])
    act, cov, q, val = table(ea, 5, 2, 4).lookup(torch.as_tensor(board_of(pos, 5)[None]).cuda(), i8(1), return_q=True, return_value=True)
    assert bool(cov[0]) and tuple(act[0].tolist()) == (0, 2)
    assert np.array_equal(q[0].cpu().numpy().view(np.int32), q32.view(np.int32))
    assert val[0].cpu().numpy().view(np.int32) == model(5).E(pos)[1].view(np.int32)


def test_not_covered(ea):
    t = table(ea, 5, 2, 4)
    t3 = table(ea, 3, 3, 4)
    b5 = boards_of(5, {(0, 0): 1, (0, 1): 2, (0, 2): 3, (3, 3): -1},            # K + 1 cubes on the agent's side
                   {(0, 0): 1, (3, 3): -1, (3, 4): -2, (4, 3): -3},             # ... on the other side
                   {(0, 0): 1, (3, 3): -1},                                     # covered
                   {(0, 0): 7, (3, 3): -1},                                     # a cell outside -6..6
                   {(0, 0): 1}, {(3, 3): -1}, {},                               # a side missing
                   {(4, 4): 1, (3, 3): -1}, {(1, 1): 1, (0, 0): -1})            # finished
    act, cov, q, val = t.lookup(b5, i8(*[1] * 9), return_q=True, return_value=True)
    assert cov.tolist() == [False, False, True, False, False, False, False, False, False]
    un = ~cov
    assert bool(torch.isneginf(q[un]).all()) and int(act[un].abs().sum()) == 0 and int(bits(val[un]).abs().sum()) == 0
    b3 = boards_of(3, {(0, 0): 1, (0, 1): 2, (0, 2): 3, (2, 1): -1, (1, 2): -2},  # 3 + 2: one over T = 4 in all
                   {(0, 0): 1, (0, 1): 2, (0, 2): 3, (2, 1): -1},                 # 3 + 1: covered
                   {(0, 0): 1, (0, 1): 2, (2, 1): -1, (1, 2): -2})                # 2 + 2: covered
    assert t3.lookup(b3, i8(1, 1, 1))[1].tolist() == [False, True, True]


@pytest.mark.parametrize("S,K,T", [(5, 2, 4), (3, 3, 4), (3, 3, 6)])
def test_the_recurrence_through_the_public_calls(ea, S, K, T):
    """value recomputed in float32 from lookup's q under the six dice: the maxima summed in dice order, one multiply"""
    t = table(ea, S, K, T)
    rng = random.Random(S + K)
    ps = [sample(rng, S, K, T) for _ in range(200)]
    b = torch.as_tensor(np.stack([board_of(p, S) for p in ps for _ in range(6)])).cuda()
    d = torch.arange(1, 7, dtype=torch.int8, device="cuda").repeat(200)
    _, cov, q, val = t.lookup(b, d, return_q=True, return_value=True)
    assert bool(cov.all())
    m = q.reshape(200, 6, 6).max(2).values.cpu().numpy()
    s = m[:, 0].copy()
    for dd in range(1, 6):
        s = (s + m[:, dd]).astype(F32)
    e = (s * SIXTH).astype(F32)
    v = val.reshape(200, 6).cpu().numpy()
    assert all(np.array_equal(v[:, dd].view(np.int32), e.view(np.int32)) for dd in range(6))


# ---------------------------------------------------------------- 4. two builds, guard zones, alignment

def test_two_builds_give_the_same_bits_and_stay_inside(ea):
    """into a zeroed buffer and into one of NaN bit patterns: every slot is written, so ALL slots are compared; 4 KB guards around it"""
    S, K, T = 3, 2, 4
    n = ea.EndgameTable.table_bytes(S, K, T) // 4
    alloc = GuardedAllocator()
    z = alloc.zeros((n,), dtype=torch.float32, tag="table (zeros)")
    nan = alloc.zeros((n,), dtype=torch.float32, tag="table (NaN)")
    nan.view(torch.int32).fill_(0x7FC00123)
    ea.EndgameTable.build(S, K, T, out=z)
    ea.EndgameTable.build(S, K, T, out=nan)
    torch.cuda.synchronize()
    alloc.check("build (3, 2, 4)")
    assert torch.equal(bits(z), bits(nan)) and torch.equal(bits(z), bits(table(ea, S, K, T).table))
    assert not bool(torch.isnan(z).any()) and bool((z.abs() <= 1).all()) and int((z != 0).sum()) > n // 8


def test_lookup_guard_zones_and_a_table_off_the_16_byte_boundary(ea):
    M, S = 33, 5
    t = table(ea, S, 2, 4)
    b0, d0 = mixed_rows(ea, M)
    ref = t.lookup(b0, d0, return_q=True, return_value=True)
    alloc = GuardedAllocator()
    b = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards", offset=1)
    d = alloc.zeros((M,), dtype=torch.int8, tag="dice", offset=1)
    b.copy_(b0); d.copy_(d0)
    with alloc.patch(tag="outputs"):            # lookup's torch.zeros outputs come out of the guarded allocator
        out = t.lookup(b, d, return_q=True, return_value=True)
    assert all(alloc.owns(x) for x in out)
    torch.cuda.synchronize()
    alloc.check("lookup M=%d" % M)
    for x, y in zip(out, ref):
        assert torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(bits(x), bits(y))
    assert torch.equal(b, b0) and torch.equal(d, d0)
    # a (3, 2, 4) table 4 bytes past a 16-byte boundary: built there and read there
    n = ea.EndgameTable.table_bytes(3, 2, 4) // 4
    off = alloc.zeros((n,), dtype=torch.float32, tag="table at +4", offset=4)
    assert off.data_ptr() % 16 == 4
    t3 = ea.EndgameTable.build(3, 2, 4, out=off)
    rng = random.Random(3)
    bb = torch.as_tensor(np.stack([board_of(sample(rng, 3, 2, 4), 3) for _ in range(50)])).cuda()
    dd = i8(*[rng.randint(1, 6) for _ in range(50)])
    x, y = t3.lookup(bb, dd, return_q=True, return_value=True), table(ea, 3, 2, 4).lookup(bb, dd, return_q=True, return_value=True)
    torch.cuda.synchronize()
    alloc.check("table at +4")
    assert torch.equal(bits(off), bits(table(ea, 3, 2, 4).table))
    assert torch.equal(x[0], y[0]) and torch.equal(bits(x[2]), bits(y[2])) and torch.equal(bits(x[3]), bits(y[3]))


# ---------------------------------------------------------------- 5. the Python layers

def test_save_and_load(ea, tmp_path):
    t = table(ea, 3, 2, 4)
    path = str(tmp_path / "eg.pt")
    t.save(path)
    u = ea.EndgameTable.load(path)
    assert (u.board_size, u.max_cubes, u.max_total, u.levels) == (3, 2, 4, 16) and torch.equal(bits(u.table), bits(t.table)) and u.table.is_cuda
    sd = torch.load(path, weights_only=True)
    torch.save(dict(sd, endgame_layout=sd["endgame_layout"] + 1), path)
    with pytest.raises(ValueError, match="layout"):
        ea.EndgameTable.load(path)
    torch.save(dict(sd, max_cubes=3, max_total=4), path)           # the table does not fit the parameters
    with pytest.raises(ValueError, match="float32 tensor of"):
        ea.EndgameTable.load(path)
    torch.save({"params": torch.zeros(3)}, path)
    with pytest.raises(ValueError, match="not an endgame table"):
        ea.EndgameTable.load(path)


@pytest.mark.parametrize("S,K,T,episodes", [(5, 2, 4, 64), (7, 2, 3, 16)])
def test_endgame_agent_on_the_drop_in_env(ea, S, K, T, episodes):
    """every ply of every episode: the agent's action is lookup's where covered and the fallback's elsewhere.  On 7x7 random play from
    the opening does not reach the table within the test, so every second episode starts from a sampled position the table covers:
    the covered plies come from the inputs"""
    from classical_policies import EndgameAgent, RandomAgent
    from envs import EinsteinWuerfeltNichtEnv
    t = table(ea, S, K, T)
    env = EinsteinWuerfeltNichtEnv(board_size=S, seed=3)
    fallback = RandomAgent(env)
    agent = EndgameAgent(t, fallback)
    plies = exact = 0
    rng = random.Random(S)
    for ep in range(episodes):
        obs, _ = env.reset(seed=ep)
        if S != 5 and ep % 2 == 0:
            env.board[:] = board_of(sample(rng, S, K, T), S)     # in place: obs["board"] is the env's board
            env._push_board()
        for _ in range(200):
            action, state = agent.predict(obs)
            assert state is None and isinstance(action, np.ndarray) and action.shape == (2,)
            b, d = obs["board"].astype(np.int8)[None], [obs["dice_roll"]]
            a_exact, cov = t.lookup(b, d)
            hand = a_exact[0] if bool(cov[0]) else fallback.predict_batch(b, d)[0]
            both, c2 = agent.predict_batch(b, d, return_covered=True)
            assert np.array_equal(action, hand.cpu().numpy()) and torch.equal(both[0], hand) and bool(c2[0]) == bool(cov[0])
            plies += 1
            exact += int(cov[0])
            obs, _, terminated, truncated, _ = env.step(action)
            if terminated or truncated:
                break
        assert terminated or truncated
    print("EndgameAgent %dx%d: %d plies, %d covered" % (S, S, plies, exact))
    assert exact > 0 and exact < plies
    if S == 5:
        bb, dd = mixed_rows(ea, 300)
    else:
        p = pool(ea, S)
        bb, dd = p["boards"][:300].clone(), p["dice"][:300].clone()
        bb[::3] = torch.as_tensor(np.stack([board_of(sample(rng, S, K, T), S) for _ in range(100)])).cuda()
    assert torch.equal(agent.policy_fn()(bb, dd, 3), agent.predict_batch(bb, dd))


def test_the_endgame_kind_in_the_tournament(ea, tmp_path):
    from ewn_gym_amd.tournament import evaluate
    t = table(ea, 5, 2, 4)
    m = pool(ea, 5)["model"]
    spec = {"kind": "endgame", "table": t, "fallback": {"kind": "mlp_lookahead", "model": m}}
    r1, r2 = evaluate(spec, {"kind": "random"}, num=64), evaluate(spec, {"kind": "random"}, num=64)
    assert r1["engine"] == "ewn_step" and r1["episodes"] == 64 and int((r1["lengths"] > 0).sum()) == 64
    assert torch.equal(r1["scores"], r2["scores"]) and torch.equal(r1["lengths"], r2["lengths"])
    assert bool((r1["scores"] != 0).all())                                # every episode ended: no illegal-move stall
    r3 = evaluate({"kind": "endgame", "table": t, "fallback": {"kind": "random"}}, {"kind": "random"}, num=64)
    assert r3["episodes"] == 64 and bool((r3["scores"] != 0).all())


def make_env(ea, N, S=5, key=77):
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=5,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=key)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 11).astype(np.uint32))
    return env


def few_cube_lanes(env, K, T, seed):
    """every second lane of the env goes on from a sampled position that the (S, K, T) table covers, under the dice it has"""
    rng = random.Random(seed)
    b = env.board.clone().reshape(env.N, env.S, env.S)
    b[::2] = torch.as_tensor(np.stack([board_of(sample(rng, env.S, K, T), env.S) for _ in range(0, env.N, 2)])).cuda()
    env.set_obs(b, env.dice.clone())


@pytest.mark.parametrize("S", [5, 7])
def test_one_distill_update_with_the_table_is_the_public_calls_composed(ea, S):
    """on 7x7 with the (7, 2, 3) table a rollout does not reach a covered position within the test: every second lane is put on one"""
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.distill import SearchDistillTrainer
    from ewn_gym_amd.vec_env import _ptr, _stream
    N, K = 256, 5
    t = table(ea, 5, 2, 4) if S == 5 else table(ea, 7, 2, 3)
    tr = SearchDistillTrainer(make_env(ea, N, S), n_steps=K, seed=5, endgame_table=t, terminal_value=0.75)
    params, sq = tr.params.clone(), torch.zeros_like(tr.params)
    tr.env.rollout_policy(14, params, noise_key=1)     # past the openings: a rollout from the reset holds no position with few cubes
    if S == 7:
        few_cube_lanes(tr.env, 2, 3, 7)
    tr.collect_and_update()
    env = make_env(ea, N, S)
    env.rollout_policy(14, params, noise_key=1)
    if S == 7:
        few_cube_lanes(env, 2, 3, 7)
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, params, traj=traj, noise_key=tr.noise_key)
    assert torch.equal(traj["record"], tr.traj["record"])
    b = traj["obs_board"][:K].reshape(K * N, S, S).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    _, q = ea.predict_lookahead(b, d, params, terminal_value=0.75, return_q=True)
    _, cov, qe = t.lookup(b, d, return_q=True)
    print("distill update %dx%d: %d of %d rows covered" % (S, S, int(cov.sum()), K * N))
    assert 0 < int(cov.sum()) < K * N
    if S == 7:
        assert int(cov[:N].sum()) >= N // 2                                # the lanes that were put on covered positions
    assert torch.equal(torch.isneginf(q[cov]), torch.isneginf(qe[cov]))   # -inf in the same places, by construction
    q = torch.where(cov[:, None, None], 0.75 * qe, q)
    tp, tv, w = ea.lookahead_targets(q, 0.0)
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    norm = torch.zeros(1, device="cuda")
    check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    assert torch.equal(bits(params), bits(tr.params)) and torch.equal(bits(sq), bits(tr.sq_avg))


def test_distill_without_a_table_is_unchanged(ea):
    from ewn_gym_amd.distill import SearchDistillTrainer
    N, K = 64, 3
    a, b = SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=5, endgame_table=None), SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=5)
    for _ in range(2):
        a.collect_and_update(); b.collect_and_update()
    assert torch.equal(bits(a.grad), bits(b.grad)) and torch.equal(bits(a.params), bits(b.params)) and torch.equal(bits(a.sq_avg), bits(b.sq_avg))
