"""The tree and lookahead kernels past one trip of their capped grids (ewn_puct.hip, ewn_lookahead_stages.hip: a wave per row, four waves
a block, at most 1 024 blocks, so a wave's second row is 4 096 rows after its first and reuses the wave's LDS slice).  M = 4 097 (one
wave alone takes a second trip), 4 096 + 70 and 8 192 + 33 (a third trip), on 5x5 and 7x7, small budgets.  Everything here is
deterministic and row-independent, so the oracle is byte equality: one big call against calls on slices of at most 1 024 rows (the size
the lock-step tests anchor to the numpy model), and the late rows of the big call against the numpy models of tests/test_gpu_puct.py and
tests/test_gpu_puct_selfplay.py directly.  The only inexact step is the prior check of those models (P_TOL / NOISE_TOL, unchanged).
Planted rows: wave w of block b serves rows 4 b + w + 4 096 trip; degenerate rows before and after live ones on the same wave, a row
whose two flags name one cube before and after one where they do not, dice outside 1..6 on late rows.
(a) the PUCT stages; (b) the late rows against the models; (c) puct_play; (d) the lookahead stages; (e) the drivers with a chunk larger
than one trip; (f) guard zones."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_lookahead_plies import check_expand  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct import F, P_TOL, Model, check_result, compare, degenerate, edges, host_views, lockstep  # noqa: E402
from tests.test_gpu_puct_selfplay import (KEYS, NOISE_TOL, ROWS, NoiseModel, check_play, check_rules, noise_rows, reset_positions,  # noqa: E402
                                          same_records)

TRIP = 4096                                         # rows in one trip of advance, result, play, expand and reduce (begin: 1 024)
SLICE = 1024
LATE = TRIP + 70                                    # the batch whose late rows go through the numpy models
CASES = [(S, M) for S in (5, 7) for M in (TRIP + 1, LATE, 2 * TRIP + 33)]
SIMS = 7
EPS = 0.25


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def cuts(M):
    return [(i, min(i + SLICE, M)) for i in range(0, M, SLICE)]


def u8(t):
    return t.contiguous().view(torch.uint8)


def dead_boards(S):
    """the degenerate boards of the existing tests: mover on the far corner, no mover cube, no opposing cube, empty, opponent on (0, 0)"""
    e = S - 1
    return boards_of(S, {(e, e): 2, (0, 1): -1}, {(2, 2): -4}, {(1, 1): 2}, {}, {(0, 0): -3, (2, 2): 1}).cpu().numpy()


def flag_boards(S):
    """(both flags name cube 4 under dice 2, the flags name cubes 2 and 5 under dice 3)"""
    e = S - 1
    b = boards_of(S, {(0, 2): 4, (2, 0): 5, (e, e - 1): -1, (e - 1, e): -4},
                  {(0, 2): 2, (2, 0): 5, (e, e - 1): -1, (e - 1, e): -4, (e - 2, e - 2): -6}).cpu().numpy()
    return (b[0], 2), (b[1], 3)


def dead_mask(boards):
    return torch.as_tensor([degenerate(x) for x in boards.cpu().numpy()]).cuda()


_ROWS = {}


def rows(ea, S, M):
    """M rows of the pool (repeated with the rows rolled by an odd count if it were shorter) with the planted rows written over them,
    computed once per shape and left unchanged -> (boards, dice, plan); plan names the planted rows: dead_then_live, live_then_dead,
    one_then_two, two_then_one (first rows r of pairs r, r + 4 096), odd_dice (rows)"""
    if (S, M) in _ROWS:
        return _ROWS[(S, M)]
    p = pool(ea, S)
    n, off, spare_n = p["boards"].shape[0], 9000 + 100 * S, 256
    i = off + np.arange(M + spare_n)
    idx = torch.as_tensor((i % n + (i // n) * 1237) % n).cuda()
    hb, hd = p["boards"][idx].cpu().numpy(), p["dice"][idx].cpu().numpy()
    spare = iter([k for k in range(M, M + spare_n) if not degenerate(hb[k])])

    def put_live(r):
        if degenerate(hb[r]):
            k = next(spare)
            hb[r], hd[r] = hb[k], hd[k]

    dead, (one, two) = dead_boards(S), flag_boards(S)
    plan = dict(dead_then_live=[r for r in (0, 5, 18, 33, 69) if r + TRIP < M], live_then_dead=[r for r in (1, 6, 34, 68) if r + TRIP < M],
                one_then_two=[r for r in (10,) if r + TRIP < M], two_then_one=[r for r in (11,) if r + TRIP < M], odd_dice=[])
    for k, r in enumerate(plan["dead_then_live"]):
        hb[r] = dead[k % 5]
        put_live(r + TRIP)
        if r == 5 and r + 2 * TRIP < M:
            hb[r + 2 * TRIP] = dead[(k + 1) % 5]               # dead, live, dead on one wave
    for k, r in enumerate(plan["live_then_dead"]):
        put_live(r)
        hb[r + TRIP] = dead[(k + 2) % 5]
        if r + 2 * TRIP < M:
            put_live(r + 2 * TRIP)                             # live, dead, live
    for r in plan["one_then_two"]:
        (hb[r], hd[r]), (hb[r + TRIP], hd[r + TRIP]) = one, two
    for r in plan["two_then_one"]:
        (hb[r], hd[r]), (hb[r + TRIP], hd[r + TRIP]) = two, one
        if r + 2 * TRIP < M:
            hb[r + 2 * TRIP], hd[r + 2 * TRIP] = two
    for r, v in ((TRIP + 20, 0), (TRIP + 21, 9), (2 * TRIP + 7, 0)) if M > TRIP + 21 else ((M - 1, 9),):
        if r < M:
            put_live(r)
            hd[r] = v
            plan["odd_dice"].append(r)
    for r in range(M - TRIP):                                  # the same wave must not see the same row twice: the pool holds the
        while np.array_equal(hb[r], hb[r + TRIP]) and hd[r] == hd[r + TRIP]:   # start position under each dice about 900 times
            k = next(spare)
            hb[r + TRIP], hd[r + TRIP] = hb[k], hd[k]
    _ROWS[(S, M)] = (torch.as_tensor(hb[:M].copy()).cuda(), torch.as_tensor(hd[:M].copy()).cuda(), plan)
    return _ROWS[(S, M)]


@pytest.mark.parametrize("S,M", CASES)
def test_the_planted_rows_are_what_they_are_named_for(ea, S, M):
    b, d, plan = rows(ea, S, M)
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    assert hb.shape == (M, S, S) and hd.shape == (M,)
    same = (hb[:-TRIP] == hb[TRIP:]).all((1, 2)) & (hd[:-TRIP] == hd[TRIP:])
    assert not same.any(), np.nonzero(same)[0][:8]             # a row and the row 4 096 later are never equal
    dead = lambda r: Model(hb[r], hd[r], 1).degenerate         # noqa: E731
    one = lambda r: bool(edges(hb[r], min(max(int(hd[r]), 1), 6))[2])   # noqa: E731
    assert plan["dead_then_live"] and (M == TRIP + 1 or (plan["live_then_dead"] and plan["one_then_two"] and plan["two_then_one"]))
    for r in plan["dead_then_live"]:
        assert dead(r) and not dead(r + TRIP), r
    for r in plan["live_then_dead"]:
        assert not dead(r) and dead(r + TRIP), r
    for r in plan["one_then_two"]:
        assert not dead(r) and not dead(r + TRIP) and one(r) and not one(r + TRIP), r
    for r in plan["two_then_one"]:
        assert not dead(r) and not dead(r + TRIP) and not one(r) and one(r + TRIP), r
    assert plan["odd_dice"] and all(r >= TRIP and not dead(r) and not 1 <= hd[r] <= 6 for r in plan["odd_dice"])
    if M > 2 * TRIP:                                           # the third trip: dead, live, dead and live, dead, live; two, one, two
        assert dead(5 + 2 * TRIP) and not dead(1 + 2 * TRIP) and not dead(6 + 2 * TRIP) and not one(11 + 2 * TRIP)
        assert hd[2 * TRIP + 7] == 0
    n_dead = sum(dead(r) for r in range(M))
    assert 0 < n_dead < M // 8                                 # the batch is live play with a few degenerate rows in it


# ---------------------------------------------------------------- (a), (b) the PUCT stages

_RUNS = {}


def stages(ea, S, M, sims, noisy):
    """begin, sims + 1 rounds of predict_policy and advance and the result, once on all M rows and once on slices of at most 1 024,
    equal byte for byte after every call.  With M = 4 096 + 70 the rows from 4 096 on are the numpy models' as well: the plain run
    through lockstep (its own calls on those 70 rows), the run with noise round by round beside the big call.  Computed once per
    shape -> dict(tree, lb, ld, b, d, result, models)"""
    key = (S, M, sims, noisy)
    if key in _RUNS:
        return _RUNS[key]
    p = pool(ea, S)
    b, d, _ = rows(ea, S, M)
    params, cs = p["params"], cuts(M)
    eta = noise_rows(b.cpu().numpy(), d.cpu().numpy(), 7 * S + M) if noisy else None
    noise = torch.as_tensor(eta).cuda() if noisy else None
    kw = lambda i, j: dict(root_noise=noise[i:j], noise_eps=EPS) if noisy else {}   # noqa: E731

    def same(where):
        for k, name in enumerate(("tree", "leaf_boards", "leaf_dice")):
            assert torch.equal(big[k], torch.cat([x[k] for x in parts])), (where, name)

    big = ea.puct_begin(b, d, sims)
    parts = [ea.puct_begin(b[i:j], d[i:j], sims) for i, j in cs]
    same("begin")
    models = None
    if M == LATE and noisy:
        hb, hd = b[TRIP:].cpu().numpy(), d[TRIP:].cpu().numpy()
        models = [NoiseModel(hb[m], hd[m], sims, eta[TRIP + m], EPS) for m in range(M - TRIP)]
        compare(ea, big[0][TRIP:], big[1][TRIP:], big[2][TRIP:], models, S, sims, "begin")
    for rnd in range(sims + 1):
        _, logits, value = ea.predict_policy(big[1], big[2], params, return_logits=True, return_value=True)
        ea.puct_advance(big[0], logits, value, big[1], big[2], sims, **kw(0, M))
        for (i, j), x in zip(cs, parts):
            _, lg, v = ea.predict_policy(x[1], x[2], params, return_logits=True, return_value=True)
            ea.puct_advance(x[0], lg, v, x[1], x[2], sims, **kw(i, j))
        same("round %d" % rnd)
        if models is not None:                                 # noise_run's round, on the big call's late rows
            gp = host_views(ea, big[0][TRIP:], S, sims)["p"]
            hl, hv = logits[TRIP:].cpu().numpy(), value[TRIP:].cpu().numpy()
            for m, mod in enumerate(models):
                ev = mod.advance(hl[m], hv[m], F(1.5), F(1), gp[m])
                if ev is not None:
                    err = float(np.abs(gp[m, ev[0]].astype(np.float64) - ev[1]).max())
                    assert err <= (NOISE_TOL if ev[0] == 0 else P_TOL), (rnd, m, ev[0], err)
            compare(ea, big[0][TRIP:], big[1][TRIP:], big[2][TRIP:], models, S, sims, "round %d" % rnd)
    if M == LATE and not noisy:
        t70, models, _ = lockstep(ea, S, b[TRIP:], d[TRIP:], params, sims)
        assert torch.equal(t70, big[0][TRIP:])
        compare(ea, big[0][TRIP:], big[1][TRIP:], big[2][TRIP:], models, S, sims, "the late rows of the big call")
    res = ea.puct_result(big[0], S, sims, return_visits=True, return_q=True, return_value=True)
    res_parts = [ea.puct_result(x[0], S, sims, return_visits=True, return_q=True, return_value=True) for x in parts]
    for k, name in enumerate(("actions", "visits", "q", "value")):
        assert torch.equal(u8(res[k]), u8(torch.cat([x[k] for x in res_parts]))), name
    assert torch.equal(ea.puct_result(big[0], S, sims), res[0])                       # the optional outputs NULL: the same actions
    _RUNS[key] = dict(tree=big[0], lb=big[1], ld=big[2], b=b, d=d, result=res, models=models)
    return _RUNS[key]


def check_roots(ea, r, S, M, sims):
    """what the planted rows must show in the results, whatever the slices say"""
    _, _, plan = rows(ea, S, M)
    act, visits, q, value = r["result"]
    dead = dead_mask(r["b"])
    assert not visits[dead].any() and not act[dead].any() and bool((q[dead] == float("-inf")).all()) and not value[dead].any()
    assert bool((visits[~dead].sum((1, 2)) == sims).all())     # every live row was searched to its budget, in every trip
    for r0 in [x + TRIP for x in plan["two_then_one"]] + plan["one_then_two"]:
        assert bool((q[r0, 1] == float("-inf")).all()) and not visits[r0, 1].any()     # one cube: edges 3 .. 5 are no actions
    for r0 in [x + TRIP for x in plan["one_then_two"]] + plan["two_then_one"]:
        assert bool(torch.isfinite(q[r0, 1]).any())
    assert not r["lb"].any() and bool((r["ld"] == 1).all())    # no leaf is pending after sims + 1 rounds


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("S,M", CASES)
def test_one_big_call_equals_many_small_ones(ea, S, M, noisy):
    r = stages(ea, S, M, SIMS, noisy)
    check_roots(ea, r, S, M, SIMS)
    plain = stages(ea, S, M, SIMS, False)
    if noisy:
        assert not torch.equal(r["tree"][TRIP:], plain["tree"][TRIP:])                # the noise reached the late rows


@pytest.mark.parametrize("S", [5, 7])
def test_one_simulation(ea, S):
    check_roots(ea, stages(ea, S, LATE, 1, False), S, LATE, 1)


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("S", [5, 7])
def test_the_late_rows_against_the_model(ea, S, noisy):
    r = stages(ea, S, LATE, SIMS, noisy)
    models = r["models"]
    assert len(models) == 70 and any(m.degenerate for m in models) and sum(not m.degenerate for m in models) > 60
    check_result(ea, r["tree"][TRIP:], models, S, SIMS)
    got = [x[TRIP:] for x in r["result"]]
    want = ea.puct_result(r["tree"][TRIP:], S, SIMS, return_visits=True, return_q=True, return_value=True)
    for x, y in zip(got, want):
        assert torch.equal(u8(x), u8(y))


# ---------------------------------------------------------------- (c) the move

@pytest.mark.parametrize("S,M", CASES)
def test_play_past_one_trip(ea, S, M):
    r = stages(ea, S, M, SIMS, True)
    tree, b, d, models = r["tree"], r["b"], r["d"], r["models"]
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    game[:, 0] = torch.arange(M, device="cuda") % 6            # plies 0 .. 5: below, at and above temp_plies = 3
    over = [x for x in (5, 8, TRIP + 5, TRIP + 8, 2 * TRIP + 8) if x < M and M > TRIP + 8]
    for x in over:                                             # games that are over, in every trip there is
        game[x, 1], game[x, 2] = 1, -1 if x % 2 else 0
    n_drawn, moved = 0, {}
    for temp_plies in (0, 3, 100):
        for key, off in (KEYS[1], KEYS[2]):                    # KEYS[2]: game numbers above 2^32
            bb, dd, gg = b.clone(), d.clone(), game.clone()
            out = ea.puct_play(tree, bb, dd, gg, S, SIMS, temp_plies=temp_plies, key=key, game_offset=off)
            assert sorted(out) == sorted(ROWS)
            small = []
            for i, j in cuts(M):
                x = (b[i:j].clone(), d[i:j].clone(), game[i:j].clone())
                o = ea.puct_play(tree[i:j], *x, S, SIMS, temp_plies=temp_plies, key=key, game_offset=off + i)
                small.append(x + tuple(o[k] for k in ROWS))
            for k, whole in enumerate((bb, dd, gg) + tuple(out[k] for k in ROWS)):
                assert torch.equal(u8(whole), u8(torch.cat([x[k] for x in small]))), (temp_plies, key, k)
            for x in over:
                assert int(out["live"][x]) == 0 and gg[x].tolist() == game[x].tolist() and torch.equal(bb[x], b[x])
            moved[(temp_plies, key)] = out["action"][TRIP:].clone()
            assert int(out["live"][TRIP:].sum()) > (M - TRIP) // 2
            if models is not None:                             # the 70 late rows against play_model, every byte
                o70, g70, drawn = check_play(ea, tree[TRIP:], models, S, SIMS, b[TRIP:], d[TRIP:], game[TRIP:], temp_plies, key, off + TRIP)
                for k in ROWS:
                    assert torch.equal(u8(o70[k]), u8(out[k][TRIP:])), k
                assert torch.equal(g70, gg[TRIP:])
                n_drawn += len(drawn)
                assert temp_plies > 0 or not drawn
    if models is not None:
        assert n_drawn > 0                                     # some late row was drawn from the visits
    if M - TRIP >= 33:                                         # ... and the draw moved a late row somewhere
        assert any(not torch.equal(moved[(0, k)], moved[(100, k)]) for k in (KEYS[1][0], KEYS[2][0]))


# ---------------------------------------------------------------- (d) the lookahead stages

def lookahead_stages(ea, S, M):
    p = pool(ea, S)
    b, d, plan = rows(ea, S, M)
    params, cs = p["params"], cuts(M)
    lb, ld, kind = ea.lookahead_expand(b, d)
    assert lb.shape == (M, 648, S, S) and ld.shape == (M, 648) and kind.shape == (M, 108)
    for i, j in cs:
        for x, y in zip((lb, ld, kind), ea.lookahead_expand(b[i:j], d[i:j])):
            assert torch.equal(x[i:j], y), (i, j)
    dead = dead_mask(b)
    assert not kind[dead].any() and not lb[dead].any() and bool(kind[~dead].any())
    for r0 in [x + TRIP for x in plan["two_then_one"]] + plan["one_then_two"]:
        assert not kind[r0, 54:].any() and bool(kind[r0, :54].any())                  # one cube: roots 3 .. 5 are roots 0 .. 2
    for r0 in [x + TRIP for x in plan["one_then_two"]] + plan["two_then_one"]:
        assert bool(kind[r0, 54:].any())
    rb, rd = lb.reshape(-1, S, S), ld.reshape(-1)
    v = ea.predict_policy(rb, rd, params, return_value=True)[1].reshape(M, 648)
    lq = ea.predict_lookahead(rb, rd, params, return_q=True)[1].reshape(M, 648, 6)    # as the two-move call chains them
    one = ea.predict_lookahead(b, d, params, return_q=True)                           # the other implementation of width 1
    for leaf in (v, lq):
        act, q = ea.lookahead_reduce(b, d, kind, leaf, return_q=True)
        for i, j in cs:
            a, qq = ea.lookahead_reduce(b[i:j], d[i:j], kind[i:j], leaf[i:j], return_q=True)
            assert torch.equal(act[i:j], a) and torch.equal(bits(q[i:j]), bits(qq)), (leaf.dim(), i, j)
        assert torch.equal(ea.lookahead_reduce(b, d, kind, leaf), act)                # q NULL: the same actions
        assert bool(torch.isneginf(q[dead]).all()) and not act[dead].any() and bool(torch.isfinite(q[~dead]).any(2).any(1).all())
        if leaf is v:
            assert torch.equal(act, one[0]) and torch.equal(bits(q), bits(one[1]))
        else:
            assert not torch.equal(bits(q), bits(one[1]))
    if M == LATE:                                              # the late rows against the rules
        check_expand(ea, b[TRIP:], d[TRIP:])


@pytest.mark.parametrize("S,M", CASES)
def test_lookahead_stages_past_one_trip(ea, S, M):
    try:
        lookahead_stages(ea, S, M)
    except torch.cuda.OutOfMemoryError:
        if (S, M) != (7, 2 * TRIP + 33):
            raise
        torch.cuda.empty_cache()
        lookahead_stages(ea, S, TRIP + 1)
        pytest.skip("7x7, M = 8 225: the 260 MB of leaf boards did not fit on this GPU; the same checks passed at M = 4 097 instead")


# ---------------------------------------------------------------- (e) the drivers with a chunk larger than one trip

@pytest.mark.parametrize("S,M", CASES)
def test_predict_puct_in_one_chunk(ea, S, M):
    p = pool(ea, S)
    b, d, _ = rows(ea, S, M)
    kw = dict(sims=SIMS, return_visits=True, return_q=True, return_value=True)
    got = ea.predict_puct(b, d, p["params"], chunk=M, **kw)
    want = ea.predict_puct(b, d, p["params"], chunk=SLICE, **kw)
    for x, y, z in zip(got, want, stages(ea, S, M, SIMS, False)["result"]):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(u8(x), u8(y)) and torch.equal(u8(x), u8(z))                # ... and both are the stages driven by hand


@pytest.mark.parametrize("S,M", CASES)
def test_predict_lookahead_two_moves_in_one_chunk(ea, S, M):
    p = pool(ea, S)
    b, d, _ = rows(ea, S, M)
    try:
        act, q = ea.predict_lookahead(b, d, p["params"], plies=2, chunk=M, return_q=True)
    except torch.cuda.OutOfMemoryError:
        if (S, M) != (7, 2 * TRIP + 33):
            raise
        torch.cuda.empty_cache()
        b, d = b[:TRIP + 1], d[:TRIP + 1]
        act, q = ea.predict_lookahead(b, d, p["params"], plies=2, chunk=TRIP + 1, return_q=True)
        M = 0
    want = ea.predict_lookahead(b, d, p["params"], plies=2, chunk=SLICE, return_q=True)
    assert torch.equal(act, want[0]) and torch.equal(bits(q), bits(want[1]))
    if M == 0:
        pytest.skip("7x7, M = 8 225: the scratch of one chunk did not fit on this GPU; the same check passed at M = 4 097 instead")


@pytest.mark.parametrize("S", [5, 7])
def test_selfplay_in_one_chunk(ea, S):
    from ewn_gym_amd.vec_env import SELFPLAY_MAX_PLIES
    p, M, T = pool(ea, S), LATE, SELFPLAY_MAX_PLIES[S]
    b, d = reset_positions(ea, S, n=M)
    d[TRIP:] = d[:M - TRIP] % 6 + 1                            # one opening position for all: a late game starts under another dice than its wave's first
    assert not bool(((b[:-TRIP] == b[TRIP:]).all(2).all(1) & (d[:-TRIP] == d[TRIP:])).any())
    kw = dict(sims=4, key=11, game_offset=2 ** 32 + 5)
    got = ea.selfplay_puct(b, d, p["params"], chunk=M, **kw)
    same_records(got, ea.selfplay_puct(b, d, p["params"], chunk=SLICE, **kw))
    late = {k: (x[TRIP:] if k in ("winner", "plies") else x[:, TRIP:]) for k, x in got.items()}
    h = check_rules(late, S, T)
    print("%dx%d: the 70 late games have %d .. %d plies (mean %.1f)" % (S, S, h["plies"].min(), h["plies"].max(), h["plies"].mean()))
    assert bool((got["winner"] != 0).all()) and int(got["plies"].min()) >= 1


# ---------------------------------------------------------------- (f) guard zones

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    """a wrong row index in a late trip writes out of bounds before it writes wrong values: every buffer the four kernels write ends
    where its last row ends"""
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib, M, sims = pool(ea, S), ea._lib.load(), TRIP + 1, SIMS
    b, d, _ = rows(ea, S, M)
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    alloc = GuardedAllocator()
    z = lambda shape, dtype, tag: alloc.zeros(shape, dtype=dtype, tag=tag)  # noqa: E731
    tree, lb, ld = z((M, nb), torch.uint8, "tree"), z((M, S, S), torch.int8, "leaf_boards"), z((M,), torch.int8, "leaf_dice")
    logits, value, noise = z((M, 5), torch.float32, "logits"), z((M,), torch.float32, "value"), z((M, 6), torch.float32, "root_noise")
    cb, cd, game = z((M, S, S), torch.int8, "boards"), z((M,), torch.int8, "dice"), z((M, 4), torch.int32, "game")
    act, visits = z((M, 2), torch.int8, "actions"), z((M, 6), torch.int32, "visits")
    q, val = z((M, 6), torch.float32, "q"), z((M,), torch.float32, "result value")
    rec = dict(board=z((M, S, S), torch.int8, "rec_board"), dice=z((M,), torch.int8, "rec_dice"), visits=z((M, 6), torch.int32, "rec_visits"),
               value=z((M,), torch.float32, "rec_value"), action=z((M, 2), torch.int8, "rec_action"), live=z((M,), torch.int8, "rec_live"))
    noise.copy_(ea.selfplay_noise(M, 1.0, 3, 0, 0))
    cb.copy_(b)
    cd.copy_(d)
    assert lib.ewn_puct_begin(S, 3, M, sims, _ptr(cb), _ptr(cd), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("begin, M=%d" % M)
    for rnd in range(sims + 1):
        _, lg, v = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
        logits.copy_(lg)
        value.copy_(v)
        assert lib.ewn_puct_advance_noise(S, 3, M, sims, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(logits), _ptr(value), _ptr(noise),
                                          C.c_float(EPS), _ptr(lb), _ptr(ld), _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("advance_noise, M=%d sims=%d" % (M, sims))
    assert lib.ewn_puct_result(S, 3, M, _ptr(tree), _ptr(act), _ptr(visits), _ptr(q), _ptr(val), _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("result, M=%d" % M)
    assert lib.ewn_puct_play(S, 3, M, _ptr(tree), _ptr(cb), _ptr(cd), _ptr(game), 8, C.c_uint64(9), C.c_int64(2 ** 40),
                             *[_ptr(rec[k]) for k in ROWS], _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("play, M=%d" % M)
    live = rec["live"] == 1
    assert bool(live[TRIP]) and not bool(live[0]) and int(live.sum()) > M // 2         # the planted pair: a dead row, then a live one
    assert bool((game[:, 0] == live.to(torch.int32)).all()) and int(rec["visits"].sum()) == sims * int(live.sum())
    assert int(visits[TRIP].sum()) == sims and torch.equal(rec["visits"], visits) and not torch.equal(cb, b)
