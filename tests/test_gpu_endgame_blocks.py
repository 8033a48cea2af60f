"""The endgame table with three cubes a side and five or six in all: the (ka, ko) blocks (2, 3), (3, 2) and (3, 3),
which hold almost all of a three-cube table's bytes, on 3x3, 4x4 and the 5x5 table of 24 GB whose entry index passes 2^31 and 2^32.
0. entry_index: the documented layout (version 1) written again in plain Python from the comment at the top of ewn_endgame.hip; its
   block sizes against EndgameTable.table_bytes, and table[entry_index(p)] against the value lookup returns, in every case below.
1. value, q, action and covered of sampled positions with five or six cubes under all six dice, through test_gpu_endgame's
   check_positions: the float32 model bit for bit, float64 within 7 * 2^-24 * Phi.  No new tolerance.
2. A block's values depend on neither K nor T: the blocks two tables share are equal by bit pattern, all of them.
3. Every slot of (2, 3), (3, 2) and (3, 3) on 3x3 that is not a live position is +0.0.
4. Coverage at ka + ko = T and at K + 1 cubes a side, with live rows around the uncovered ones.
5. Two builds of (3, 3, 5) inside guard zones."""
import itertools
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_endgame import (_TABLES, Model, bits, board_of, check_positions, covered_np, model, moves_of, phi, sample,  # noqa: E402
                                    table)

assert model(3).__class__ is Model                 # the module's memoised models, one per board size, are test_gpu_endgame's

NEW = ((2, 3), (3, 2), (3, 3))                     # the blocks no table of at most four cubes has
CASES = ((3, 3, 5), (3, 3, 6), (4, 3, 5), (5, 3, 5), (3, 3, 4), (3, 2, 4), (4, 2, 4), (5, 2, 4))
GIB = 1 << 30


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.fixture(scope="module", autouse=True)
def free_the_4x4_table():
    yield
    if _TABLES.pop((4, 3, 5), None) is not None:           # 2.6 GB
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 0. the layout, from its description

MASKS = {k: [m for m in range(64) if bin(m).count("1") == k] for k in (1, 2, 3)}     # bit j - 1: cube number j; ascending


def n_side(S, k):
    return math.comb(6, k) * (S * S) ** k


def blocks(S, K, T):
    """{(ka, ko): (first entry, entries)}, ka-major over ka + ko <= T"""
    out, off = {}, 0
    for ka in range(1, K + 1):
        for ko in range(1, K + 1):
            if ka + ko <= T:
                out[(ka, ko)] = (off, n_side(S, ka) * n_side(S, ko))
                off += out[(ka, ko)][1]
    return out


def side_index(side, S):
    """side: ((cube number, cell), ...) sorted by number"""
    v = MASKS[len(side)].index(sum(1 << (k - 1) for k, _ in side))
    for _, c in sorted(side):
        v = v * S * S + c
    return v


def entry_index(pos, S, K, T):
    agent, opp = pos
    return blocks(S, K, T)[(len(agent), len(opp))][0] + side_index(agent, S) * n_side(S, len(opp)) + side_index(opp, S)


def block_of(t, ka, ko):
    """the block's slots as int32 bit patterns, a view of the table"""
    off, n = blocks(t.board_size, t.max_cubes, t.max_total)[(ka, ko)]
    return bits(t.table[off:off + n])


def slots_hold_the_values(t, positions):
    """table[entry_index(p)] has the bits of the value lookup returns for p"""
    S, K, T = t.board_size, t.max_cubes, t.max_total
    idx = torch.tensor([entry_index(p, S, K, T) for p in positions], dtype=torch.int64, device="cuda")
    assert int(idx.min()) >= 0 and int(idx.max()) < t.table.numel()
    val = t.value(torch.as_tensor(np.stack([board_of(p, S) for p in positions])).cuda())
    assert torch.equal(bits(t.table[idx]), bits(val))
    return idx


def draw(seed, S, K, T, n, keep):
    rng, out = random.Random(seed), []
    while len(out) < n:
        p = sample(rng, S, K, T)
        if keep(p):
            out.append(p)
    return out


def cubes(p):
    return len(p[0]) + len(p[1])


def per_block(ps):
    return {b: sum(1 for p in ps if (len(p[0]), len(p[1])) == b) for b in NEW}


def test_the_mirror_adds_up_to_table_bytes(ea):
    for S, K, T in CASES:
        bl = blocks(S, K, T)
        assert 4 * sum(n for _, n in bl.values()) == ea.EndgameTable.table_bytes(S, K, T), (S, K, T)
        offs = [o for o, _ in bl.values()]
        assert offs == sorted(offs) and offs[0] == 0
    assert list(blocks(3, 3, 5)) == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2)]
    assert [ea.EndgameTable.table_bytes(*c) for c in CASES[:4]] == [154457604, 1004763204, 2641465344, 24175402500]
    assert 4 * blocks(5, 3, 5)[(2, 3)][0] < 2 ** 32 < 4 * sum(blocks(5, 3, 5)[(2, 3)])     # the byte offset passes 2^32 inside (2, 3)
    # a side index by hand: cubes 2 and 5 on cells 7 and 1 of 3x3; masks of two cubes below 0b010010: 3, 5, 6, 9, 10, 12, 17
    assert side_index(((2, 7), (5, 1)), 3) == 7 * 81 + 7 * 9 + 1


# ---------------------------------------------------------------- 1. values and q against the model

def a_move_captures_into_a_smaller_block(p, S):
    return any(nxt != "win" and cubes(nxt) < cubes(p) for k, _ in p[0] for _, nxt in moves_of(p, S, k))


# 3x3, every cube as far from its corner as distinct cells allow: Phi = 4 + 3 + 3 a side of three, 4 + 3 a side of two
FARTHEST = {5: [(((1, 0), (2, 1), (3, 3)), ((4, 8), (5, 7))), (((1, 0), (2, 1)), ((3, 8), (4, 7), (5, 5)))],
            6: [(((1, 0), (2, 1), (3, 3)), ((4, 8), (5, 7), (6, 5)))]}


@pytest.mark.parametrize("T", [5, 6])
def test_3x3_five_and_six_cubes_against_the_model(ea, T):
    """no cap on Phi: it passes 16, the highest level a four-cube position of 3x3 can have.  Five cubes reach 17 and the 200 sampled
    positions stop at 16, so the positions of the highest level are added to them by hand"""
    S, K = 3, 3
    ps = draw(100 * S + 10 * K + T, S, K, T, 200, lambda p: cubes(p) >= 5)
    assert len(ps) == 200 and [phi(p, S) for p in FARTHEST[T]] == {5: [17, 17], 6: [20]}[T]
    ps += FARTHEST[T]
    hit = per_block(ps)
    print("(3, 3, %d): positions per block %s, max Phi %d" % (T, hit, max(phi(p, S) for p in ps)))
    if T == 6:
        assert min(hit.values()) >= 40
        assert max(phi(p, S) for p in ps) >= 20
    else:
        assert hit[(2, 3)] >= 40 and hit[(3, 2)] >= 40 and hit[(3, 3)] == 0
    assert any(a_move_captures_into_a_smaller_block(p, S) for p in ps)
    check_positions(ea, S, K, T, ps, "five cubes and more")
    t = table(ea, S, K, T)
    assert (t.board_size, t.max_cubes, t.max_total, t.levels) == (S, K, T, 2 * T * (S - 1))
    slots_hold_the_values(t, ps)


def test_4x4_five_cubes_against_the_model(ea):
    """Phi <= 16 only keeps the Python model to a second"""
    S, K, T = 4, 3, 5
    ps = draw(435, S, K, T, 40, lambda p: cubes(p) >= 5 and phi(p, S) <= 16)
    hit = per_block(ps)
    print("(4, 3, 5): positions per block %s" % (hit,))
    assert hit[(2, 3)] >= 1 and hit[(3, 2)] >= 1
    check_positions(ea, S, K, T, ps, "five cubes, Phi <= 16")
    slots_hold_the_values(table(ea, S, K, T), ps)


def positions_5x5():
    return draw(535, 5, 3, 5, 40, lambda p: cubes(p) == 5 and phi(p, 5) <= 16)


def ranges_5x5(ps):
    idx = [entry_index(p, 5, 3, 5) for p in ps]
    return (sum(1 for i in idx if i < 2 ** 31), sum(1 for i in idx if 2 ** 31 <= i < 2 ** 32), sum(1 for i in idx if i >= 2 ** 32))


def test_the_5x5_sample_lies_on_both_sides_of_2_31_and_2_32():
    """on the sample and the mirror alone: needs no GPU"""
    lo, mid, hi = ranges_5x5(positions_5x5())
    print("(5, 3, 5): %d entries below 2^31, %d in [2^31, 2^32), %d at or past 2^32" % (lo, mid, hi))
    assert min(lo, mid, hi) >= 5 and lo + mid + hi == 40


def test_5x5_five_cubes_the_24_GB_table(ea):
    """the table the README gives: 6 043 850 625 entries.  Built here and freed here.  This test found the build launching levels
    of 23 866 975 workgroups in one grid, of which 7 089 759 ran: blocks (3, 1), (3, 2) and 43 % of (2, 3) stayed 0"""
    S, K, T = 5, 3, 5
    free = torch.cuda.mem_get_info()[0]
    if free < 32 * GIB:
        pytest.skip("the (5, 3, 5) table is 24 GB and %.1f GiB of device memory are free: below 32 GiB" % (free / GIB))
    ps = positions_5x5()
    assert min(ranges_5x5(ps)) >= 5
    small = table(ea, 5, 2, 4)
    try:
        t = table(ea, S, K, T)
        assert t.table.numel() == 6043850625
        check_positions(ea, S, K, T, ps, "five cubes, Phi <= 16")
        idx = slots_hold_the_values(t, ps)
        assert int((idx >= 2 ** 32).sum()) >= 5
        for b in ((1, 1), (1, 2), (2, 1), (2, 2)):
            same_block(t, small, *b)
        del t, idx
    finally:
        _TABLES.pop((S, K, T), None)
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 2. shared blocks

def same_block(a, b, ka, ko):
    """block (ka, ko) of the tables a and b (b the smaller one), every slot"""
    S = a.board_size
    x, y = block_of(a, ka, ko), block_of(b, ka, ko)
    assert x.numel() == y.numel() and torch.equal(x, y), (ka, ko)
    assert int((x != 0).sum()) > 0
    # ... and it is block (ka, ko), not another of its size: blocks (ka, ko) and (ko, ka) are as long, so two tables laid out ko-major
    # would pass the comparison above.  a's slots against the values that b looks up
    ps = draw(10 * ka + ko, S, max(ka, ko), ka + ko, 16, lambda p: (len(p[0]), len(p[1])) == (ka, ko))
    local = torch.tensor([side_index(p[0], S) * n_side(S, ko) + side_index(p[1], S) for p in ps], device="cuda")
    val = b.value(torch.as_tensor(np.stack([board_of(p, S) for p in ps])).cuda())
    assert torch.equal(x[local], bits(val)), (ka, ko)


@pytest.mark.parametrize("big,smaller", [((3, 3, 6), (3, 3, 5)), ((3, 3, 6), (3, 3, 4)), ((3, 3, 6), (3, 2, 4)), ((4, 3, 5), (4, 2, 4))])
def test_shared_blocks_are_equal_by_bits(ea, big, smaller):
    a, b = table(ea, *big), table(ea, *smaller)
    shared = [k for k in blocks(*smaller) if k in blocks(*big)]
    assert shared == list(blocks(*smaller))                        # the smaller table's blocks are all in the larger one
    for ka, ko in shared:
        same_block(a, b, ka, ko)


# ---------------------------------------------------------------- 3. slots that are not positions

def sides(S, k, agent):
    """of every side index of k cubes: (valid on its own bool [n_k], the occupied cells as a bit mask int32 [n_k]), on the GPU"""
    C_ = S * S
    rem = torch.arange(n_side(S, k), dtype=torch.int64, device="cuda") % C_ ** k
    ok = torch.ones_like(rem, dtype=torch.bool)
    occ = torch.zeros_like(rem)
    for _ in range(k):
        bit = 1 << (rem % C_)
        ok &= (occ & bit) == 0
        occ |= bit
        rem = rem // C_
    ok &= (occ & (1 << (C_ - 1) if agent else 1)) == 0             # an agent cube on C - 1, an opposing cube on 0
    return ok, occ.to(torch.int32)


def live_count(S, ka, ko):
    """by enumeration of the cells, not of indices"""
    C_ = S * S
    n = sum(1 for c in itertools.permutations(range(C_), ka + ko) if C_ - 1 not in c[:ka] and 0 not in c[ka:])
    return n * math.comb(6, ka) * math.comb(6, ko)


@pytest.mark.parametrize("T,ka,ko", [(5, 2, 3), (5, 3, 2), (6, 3, 3)])
def test_slots_that_are_not_positions_are_plus_zero(ea, T, ka, ko):
    S = 3
    blk = block_of(table(ea, S, 3, T), ka, ko).reshape(n_side(S, ka), n_side(S, ko))
    ok_a, occ_a = sides(S, ka, True)
    ok_o, occ_o = sides(S, ko, False)
    rows = max(1, (1 << 26) // n_side(S, ko))                      # 2^26 slots a chunk: 256 MB of int32, 64 MB of bool
    live_n = dead_nonzero = live_nonzero = 0
    for i in range(0, n_side(S, ka), rows):
        live = (ok_a[i:i + rows, None] & ok_o[None, :]) & ((occ_a[i:i + rows, None] & occ_o[None, :]) == 0)
        nz = blk[i:i + rows] != 0                                   # by bit pattern: -0.0 is not +0.0
        live_n += int(live.sum())
        dead_nonzero += int((nz & ~live).sum())
        live_nonzero += int((nz & live).sum())
        del live, nz
    print("(3, 3, %d) block (%d, %d): %d slots, %d live, %d of them nonzero" % (T, ka, ko, blk.numel(), live_n, live_nonzero))
    assert live_n == live_count(S, ka, ko)                         # the decode above finds the live slots, all of them
    assert dead_nonzero == 0
    assert live_nonzero > live_n // 2                              # not of each live slot: the model has live positions of value 0 here


# ---------------------------------------------------------------- 4. coverage at the new boundary

A3, O3 = ((1, 0), (2, 1), (3, 2)), ((1, 6), (2, 7), (3, 8))
ROWS = [
    (A3, O3),                                                      # 0  3 + 3
    (A3, O3[:2]),                                                  # 1  3 + 2
    (A3[:2], O3),                                                  # 2  2 + 3
    (A3 + ((4, 3),), O3[:1]),                                      # 3  four cubes on the agent's side
    (A3[:1], O3 + ((4, 5),)),                                      # 4  ... on the other side
    (((2, 4), (5, 1)), ((1, 3), (4, 5), (6, 8))),                  # 5  2 + 3
    (((6, 3), (4, 7), (1, 2)), ((3, 1), (5, 8), (2, 4))),          # 6  3 + 3
    (((6, 3), (4, 7), (1, 2)), ((3, 1), (5, 8))),                  # 7  3 + 2
]


def norm(p):
    return tuple(sorted(p[0])), tuple(sorted(p[1]))


@pytest.mark.parametrize("T", [5, 6])
def test_coverage_at_five_and_six_cubes(ea, T):
    S, K = 3, 3
    t = table(ea, S, K, T)
    ps = [norm(p) for p in ROWS]
    b = torch.as_tensor(np.stack([board_of(p, S) for p in ps])).cuda()
    d = torch.tensor([1, 2, 3, 4, 5, 6, 1, 2], dtype=torch.int8, device="cuda")
    act, cov, q, val = t.lookup(b, d, return_q=True, return_value=True)
    want = covered_np(b.cpu().numpy(), K, T)
    assert want.tolist() == [T == 6, True, True, False, False, True, T == 6, True]
    assert np.array_equal(cov.cpu().numpy(), want)
    un = ~cov
    assert bool(torch.isneginf(q[un]).all()) and int(act[un].abs().sum()) == 0 and int(bits(val[un]).abs().sum()) == 0
    # the live rows alone give the same bits, and they are the model's
    keep = torch.as_tensor(want).cuda()
    a1, c1, q1, v1 = t.lookup(b[keep].contiguous(), d[keep].contiguous(), return_q=True, return_value=True)
    assert bool(c1.all()) and torch.equal(a1, act[keep]) and torch.equal(bits(q1), bits(q[keep])) and torch.equal(bits(v1), bits(val[keep]))
    mod = model(S)
    for m in np.nonzero(want)[0]:
        assert np.array_equal(q[m].cpu().numpy().view(np.int32), mod.q(ps[m], int(d[m]))[1].view(np.int32)), m
        assert val[m].cpu().numpy().view(np.int32) == mod.E(ps[m])[1].view(np.int32), m
    slots_hold_the_values(t, [ps[m] for m in np.nonzero(want)[0]])


# ---------------------------------------------------------------- 5. the build inside guard zones

def test_two_builds_of_3_3_5_give_the_same_bits_and_stay_inside(ea):
    """the last block, (3, 2), ends where the buffer ends"""
    S, K, T = 3, 3, 5
    n = ea.EndgameTable.table_bytes(S, K, T) // 4
    assert sum(blocks(S, K, T)[(3, 2)]) == n
    alloc = GuardedAllocator()
    z = alloc.zeros((n,), dtype=torch.float32, tag="table (zeros)")
    nan = alloc.zeros((n,), dtype=torch.float32, tag="table (NaN)")
    nan.view(torch.int32).fill_(0x7FC00123)
    ea.EndgameTable.build(S, K, T, out=z)
    ea.EndgameTable.build(S, K, T, out=nan)
    torch.cuda.synchronize()
    alloc.check("build (3, 3, 5)")
    assert torch.equal(bits(z), bits(nan)) and torch.equal(bits(z), bits(table(ea, S, K, T).table))
    assert not bool(torch.isnan(z).any()) and bool((z.abs() <= 1).all())
