"""The endgame table on every board size it is instantiated for, and past the 64th cell.
A. S = 3 .. 11, one cube a side: the WHOLE table of (S, 1, 2), all 36 C^2 slots, against test_gpu_endgame's model.  The slot of
   (agent number ka on cell ca; opposing number ko on cell co) is ((ka - 1) C + ca) 6 C + (ko - 1) C + co.  Live slots equal the float32
   model by bit pattern and lie within 7 * 2^-24 * Phi of the float64 one; every other slot is +0.0; and because the model has no live
   1v1 position of value 0 (asserted first), nonzero means live: a position the build dropped shows.  At 9x9 and 11x11, where the
   occupancy mask of eg_decode takes its second 64-bit word, lookup on every live pair under all six dice.
B. Two cubes a side on 7x7 and 9x9, (S, 2, 3): sampled positions with Phi <= 24 (the bound only keeps the Python model to seconds)
   and constructed 9x9 positions on both sides of cell 64.
No new tolerance: test_gpu_endgame's check_positions and its bounds, unchanged."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_endgame import (F32, _TABLES, board_of, check_positions, model, moves_of, phi, sample, table)  # noqa: E402
from tests.test_gpu_predict_policy import bits  # noqa: E402

PHI_MAX = 24
SEEDS = {7: 3, 9: 10}                   # of the sampled positions; chosen so that the 9x9 sample meets the bounds asserted on it


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.fixture(scope="module", autouse=True)
def free_the_9x9_table():
    yield
    if _TABLES.pop((9, 2, 3), None) is not None:           # 383 MB
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- A. one cube a side, the whole table

_ONE = {}


def one_cube_model(S):
    """(live bool [C, C], E float32 [C, C], E float64 [C, C], Phi [C, C]) over (agent cell, opposing cell), cube number 1 on both
    sides; zeros where the pair is not live.  Computed once per size and left unchanged"""
    if S not in _ONE:
        C_ = S * S
        mod = model(S)
        live = np.zeros((C_, C_), bool)
        e32, e64, ph = np.zeros((C_, C_), F32), np.zeros((C_, C_)), np.zeros((C_, C_))
        for ca in range(C_ - 1):
            for co in range(1, C_):
                if ca == co:
                    continue
                pos = (((1, ca),), ((1, co),))
                live[ca, co] = True
                e64[ca, co], e32[ca, co] = mod.E(pos)
                ph[ca, co] = phi(pos, S)
        _ONE[S] = (live, e32, e64, ph)
    return _ONE[S]


def live_pairs(S):
    live = one_cube_model(S)[0]
    return [(((1, int(ca)),), ((1, int(co)),)) for ca, co in np.argwhere(live)]


LIVE_PAIRS = {3: 57, 4: 211, 5: 553, 6: 1191, 7: 2257, 8: 3907, 9: 6321, 10: 9703, 11: 14281}     # (C - 1)^2 - (C - 2)


@pytest.mark.parametrize("S", range(3, 12))
def test_the_model_has_no_live_1v1_position_of_value_zero(S):
    """what makes `nonzero means live` a test of the table: needs no GPU"""
    live, e32, e64, _ = one_cube_model(S)
    assert int(live.sum()) == LIVE_PAIRS[S]
    assert (e32[live] != 0).all() and (e64[live] != 0).all() and not e32[~live].any()


@pytest.mark.parametrize("S", range(3, 12))
def test_the_whole_table_one_cube_a_side(ea, S):
    C_ = S * S
    live, e32, e64, ph = one_cube_model(S)
    assert (e32[live] != 0).all()                                                   # the property of the model, first
    t = table(ea, S, 1, 2)
    assert t.table.numel() == 36 * C_ * C_ and ea.EndgameTable.table_bytes(S, 1, 2) == 4 * 36 * C_ * C_
    tab = t.table.cpu().numpy().reshape(6, C_, 6, C_).transpose(0, 2, 1, 3)         # [ka - 1, ko - 1, ca, co]: the documented slot
    want = np.where(live, e32, F32(0.0)).astype(F32)                                # +0.0 wherever the pair is not live
    err = np.abs(tab.astype(np.float64) - e64)[:, :, live]
    tol = 7 * 2.0 ** -24 * ph[live]
    print("(%d, 1, 2): %d slots, %d live pairs x 36 numberings, max |E - f64| %.3g (smallest bound %.3g), %d nonzero slots" % (
        S, tab.size, int(live.sum()), err.max(), tol.min(), int((tab != 0).sum())))
    for ka in range(6):
        for ko in range(6):
            assert np.array_equal(tab[ka, ko].view(np.int32), want.view(np.int32)), (S, ka + 1, ko + 1)   # live: the model's bits; else +0.0
            assert np.array_equal(tab[ka, ko].view(np.int32), tab[0, 0].view(np.int32))                   # the number cannot matter
    assert (err <= tol).all()
    assert np.array_equal(tab != 0, np.broadcast_to(live, tab.shape))               # nonzero means live: nothing dropped, nothing extra
    assert not np.isnan(tab).any() and (np.abs(tab) <= 1).all()


@pytest.mark.parametrize("S", [9, 11])
def test_lookup_on_every_live_pair_past_the_64th_cell(ea, S):
    C_ = S * S
    ps = live_pairs(S)
    assert len(ps) == LIVE_PAIRS[S] and sum(1 for p in ps if p[0][0][1] >= 64 and p[1][0][1] >= 64) > 100
    check_positions(ea, S, 1, 2, ps, "every live pair")
    # not live: an agent cube on C - 1, an opposing cube on 0, a cube number 7 (next to live rows, which stay covered)
    b = np.zeros((6, C_), np.int8)
    b[0, C_ - 1], b[0, 70] = 1, -1
    b[1, 70], b[1, 0] = 1, -1
    b[2, 6], b[2, 70] = 7, -1
    b[3, 6], b[3, 70] = 1, -7
    b[4, 6], b[4, 70] = 1, -1
    b[5, 70], b[5, 6] = 1, -1
    act, cov, q, val = table(ea, S, 1, 2).lookup(torch.as_tensor(b.reshape(6, S, S)).cuda(), torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int8).cuda(),
                                                 return_q=True, return_value=True)
    assert cov.tolist() == [False, False, False, False, True, True]
    un = ~cov
    assert bool(torch.isneginf(q[un]).all()) and int(act[un].abs().sum()) == 0 and int(bits(val[un]).abs().sum()) == 0
    assert bool((val[cov] != 0).all())


# ---------------------------------------------------------------- B. two cubes a side on 7x7 and 9x9

def high(pos):
    """(an agent cube on a cell >= 64, an opposing one)"""
    return any(c >= 64 for _, c in pos[0]), any(c >= 64 for _, c in pos[1])


_SAMPLES = {}


def sampled(S, n=100):
    """the first n draws of sample(rng, S, 2, 3) with Phi <= PHI_MAX, a fixed seed per board"""
    if S not in _SAMPLES:
        rng, out, draws = random.Random(SEEDS[S]), [], 0
        while len(out) < n:
            p = sample(rng, S, 2, 3)
            draws += 1
            if phi(p, S) <= PHI_MAX:
                out.append(p)
        _SAMPLES[S] = (out, draws)
    return _SAMPLES[S]


def test_the_9x9_sample_reaches_the_second_occupancy_word():
    """on the sample itself: needs no GPU"""
    ps, draws = sampled(9)
    either = sum(1 for p in ps if any(high(p)))
    both = sum(1 for p in ps if all(high(p)))
    print("9x9: %d positions of %d draws, %d with a cube on a cell >= 64, %d with one on both sides" % (len(ps), draws, either, both))
    assert len(ps) == 100 and either >= 30 and both >= 5
    assert any(len(p[0]) == 2 for p in ps) and any(len(p[1]) == 2 for p in ps)


@pytest.mark.parametrize("S", [7, 9])
def test_sampled_positions_two_cubes_a_side(ea, S):
    ps, draws = sampled(S)
    if S == 9:
        assert sum(1 for p in ps if any(high(p))) >= 30 and sum(1 for p in ps if all(high(p))) >= 5
    check_positions(ea, S, 2, 3, ps, "sampled, Phi <= %d (%d draws)" % (PHI_MAX, draws))
    print("(%d, 2, 3): the model holds %d states" % (S, len(model(S).memo)))
    t = table(ea, S, 2, 3)
    assert (t.board_size, t.max_cubes, t.max_total, t.levels) == (S, 2, 3, 6 * (S - 1))
    assert t.table.numel() * 4 == ea.EndgameTable.table_bytes(S, 2, 3)


# 9x9: cell 63 is (7, 0), 64 is (7, 1), 72 is (8, 0), 80 the agent's goal.  name -> (agent, opponent), each ((number, cell), ...)
CONSTRUCTED_9 = {
    "two agent cubes on c and c + 64": (((1, 6), (2, 70)), ((3, 40),)),
    "two opposing cubes on c and c + 64": (((3, 40),), ((1, 6), (2, 70))),
    "agent on c, opponent on c + 64": (((1, 6),), ((1, 70),)),
    "agent on c + 64, opponent on c": (((1, 70),), ((1, 6),)),
    "takes an opposing cube on a cell >= 64": (((1, 64),), ((1, 65), (2, 20))),
    "takes its own cube on a cell >= 64": (((1, 64), (2, 65)), ((1, 20),)),
    "from 63 right, down and diagonally over the word boundary": (((1, 63),), ((1, 30),)),
    "... with a second agent cube next to it": (((1, 63), (4, 62)), ((2, 30),)),
    "a step from 80 against a step from 0": (((1, 79),), ((1, 1),)),
    "... on the other edges": (((1, 71),), ((1, 9),)),
    "2v1: the best move takes the last opposing cube": (((1, 9), (2, 64)), ((1, 10),)),
    "1v2: every reply can take the agent's last cube": (((1, 66),), ((1, 76), (2, 77))),
}


def takes_the_last_cube(pos, S):
    """a move of the side to move lands on the only cube of the other side"""
    (_, last), = pos[1]
    return any(n == "win" and c + (1, S, S + 1)[r] == last for k, c in pos[0] for r, n in moves_of(pos, S, k))


def test_the_constructed_9x9_positions_are_what_their_names_say():
    """on the model and the rules alone: needs no GPU"""
    S, mod, P = 9, model(9), CONSTRUCTED_9
    for name, pos in P.items():
        assert mod.E(pos)[1] != 0 and mod.E(pos)[0] != 0, name                      # a zeroed slot cannot pass
        for d in range(1, 7):
            assert np.isfinite(mod.q(pos, d)[1].max()), (name, d)
    a, o = P["two agent cubes on c and c + 64"]
    assert a[1][1] - a[0][1] == 64 and P["two opposing cubes on c and c + 64"] == (o, a)
    for name in ("agent on c, opponent on c + 64", "agent on c + 64, opponent on c"):
        a, o = P[name]
        assert abs(a[0][1] - o[0][1]) == 64
    # the captures: the child of the move holds one cube less on the side that lost it (the child is seen by the other side)
    a, o = P["takes an opposing cube on a cell >= 64"]
    nxt = dict(moves_of((a, o), S, 1))[0]
    assert o[0][1] == a[0][1] + 1 >= 64 and len(nxt[0]) == 1 and len(nxt[1]) == 1
    a, o = P["takes its own cube on a cell >= 64"]
    nxt = dict(moves_of((a, o), S, 1))[0]
    assert a[1][1] == a[0][1] + 1 >= 64 and len(nxt[0]) == 1 and nxt[1] == ((1, 80 - 65),)
    a, o = P["from 63 right, down and diagonally over the word boundary"]
    assert sorted(80 - n[1][0][1] for _, n in moves_of((a, o), S, 1)) == [64, 72, 73]
    q = mod.q(P["a step from 80 against a step from 0"], 3)[1]
    assert q[0, 0] == 1.0 and np.isneginf(q[0, 1:]).all()
    q = mod.q(P["... on the other edges"], 3)[1]
    assert q[0, 1] == 1.0 and np.isneginf(q[0, [0, 2]]).all()                       # (7, 8): only down stays on the board
    pos = P["2v1: the best move takes the last opposing cube"]
    assert takes_the_last_cube(pos, S) and mod.q(pos, 1)[1][0, 0] == 1.0 and mod.E(pos)[1] < 1.0
    pos = P["1v2: every reply can take the agent's last cube"]
    assert len(moves_of(pos, S, 1)) == 3
    for _, nxt in moves_of(pos, S, 1):                                              # after each move, seen by the side that replies
        assert len(nxt[1]) == 1 and nxt[1][0][1] != 80 and takes_the_last_cube(nxt, S)


def test_constructed_9x9_positions_on_both_sides_of_cell_64(ea):
    mod = model(9)
    ps = list(CONSTRUCTED_9.values())
    for name, pos in CONSTRUCTED_9.items():
        assert mod.E(pos)[1] != 0 and all(np.isfinite(mod.q(pos, d)[1].max()) for d in range(1, 7)), name
    b, d = check_positions(ea, 9, 2, 3, ps, "constructed")
    val = table(ea, 9, 2, 3).value(b)
    assert bool((val != 0).all())
