"""PUCT self-play: root noise (ewn_puct_advance_noise), the move of a game (ewn_puct_play), the driver selfplay_puct and
the trainer, against test_gpu_puct's numpy model of the search and a numpy model of the move written here.
1. noise_eps = 0 is the plain call, byte for byte.  2. Lock step with noise: the model is subclassed with the mixing at node 0.  The
root's mixed priors lie within NOISE_TOL of the float64 evaluation of the same formula on the same fp32 inputs; the model then adopts
the GPU's bits as test_gpu_puct's lock step does.  NOISE_TOL = P_TOL + 16 * 2^-24: the unmixed prior is within P_TOL (the factor
keep <= 1 does not enlarge that), and the mixing adds ten fp32 roundings on values of at most 1 -- five additions in es, the division
eta / es, the product with eps, keep = 1 - eps itself, the product keep * P and the final sum -- each of at most 2^-24 absolute;
ten is rounded up to sixteen as test_gpu_puct rounds its count up.  Derived, not tuned.  3. ewn_puct_play against the model, bit for
bit.  4. the driver is the stages, and its records obey the rules of the game; with endgame_table= it is the stages with the table's
exact values written over the covered leaves' (DESIGN.md 4p).  5. guard zones.  6. the trainer, without and with a table."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle  # noqa: E402
from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, cube_moves, cubes_of, find_cube, i8  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct import F, P_TOL, Model, compare, edges, flip, host_views, lockstep  # noqa: E402

NOISE_TOL = P_TOL + 16 * 2.0 ** -24
ROWS = ("board", "dice", "visits", "value", "action", "live")


def row_shapes(S):
    """a record row's (shape per game, dtype) by name, in the order of ROWS: ewn_puct_play's rec_* arguments"""
    return dict(board=((S, S), torch.int8), dice=((), torch.int8), visits=((2, 3), torch.int32), value=((), torch.float32),
                action=((2,), torch.int8), live=((), torch.int8))


KEYS = ((0, 0), (0xDEADBEEFCAFEF00D, 7), (5, 2 ** 32 + 3), (2 ** 64 - 1, 2 ** 40 + 1))


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


# ---------------------------------------------------------------- the model: the mixing at node 0, and the move

def mix64(prior, kind, eta, eps):
    """the definition's formula in float64 on the fp32 inputs the kernel gets (eps and keep = fl(1 - eps) are fp32 numbers)"""
    e = np.where((kind != 0) & np.isfinite(eta) & (eta > 0), eta, F(0)).astype(np.float64)
    es = e.sum()
    if not es > 0:
        return prior
    keep = float(F(F(1) - F(eps)))
    return np.where(kind != 0, keep * prior + float(F(eps)) * (e / es), 0.0)


class NoiseModel(Model):
    def __init__(self, board, dice, sims, eta, eps):
        super().__init__(board, dice, sims)
        self.eta, self.eps = np.asarray(eta, F), eps

    def advance(self, logits, V, c, inv_tv, gpu_p):
        root = self.pending == 0
        out = super().advance(logits, V, c, inv_tv, gpu_p)
        if root and out is not None:
            out = (0, mix64(out[1], self.t["kind"][0], self.eta, self.eps))
        return out


def after(board, d, a):
    """the board after edge a = 3 f + r of the node (board, d)"""
    cube = find_cube(cubes_of(board, 1), int(d), a // 3 == 1)
    return next(nb for r, nb in cube_moves(board, cube, 1) if r == a % 3)


def philox_words(ply, g, key):
    return pyoracle.philox([ply & 0xFFFFFFFF, g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, 0x50555350], [key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF])


def play_model(mod, board, dice, game, temp_plies, key, g):
    """ewn_puct_play of one game on the model's tree -> (record row dict, board, dice, game, whether the edge was drawn from the visits)"""
    S = board.shape[0]
    rec = dict(board=np.zeros((S, S), np.int8), dice=np.int8(0), visits=np.zeros(6, np.int32), value=F(0), action=np.zeros(2, np.int8),
               live=np.int8(0))
    game = game.copy()
    ply, over = int(game[0]), int(game[1])
    kind, n = mod.t["kind"][0], mod.t["n"][0]
    if over != 0 or mod.degenerate or not kind.any():
        if over == 0:
            game[1] = 1
        return rec, board, dice, game, False
    o = philox_words(ply, g, key)
    wins, drawn = [a for a in range(6) if kind[a] == 1], False
    if wins:
        a = wins[0]
    else:
        tn = int(n[kind == 2].sum())
        if ply < temp_plies and tn > 0:
            r, run, drawn = (int(o[0]) * tn) >> 32, 0, True
            for a in range(6):
                if kind[a] == 2:
                    run += int(n[a])
                    if run > r:
                        break
        else:
            f, r = mod.result()[0]
            a = 3 * f + r
    root, d = mod.t["board"][0], int(mod.t["dice"][0])
    rec = dict(board=root.copy(), dice=np.int8(d), visits=n.copy(), value=mod.result()[3], action=np.array([a // 3, a % 3], np.int8),
               live=np.int8(1))
    game[0] = ply + 1
    if kind[a] == 1:
        game[1], game[2] = 1, 1 if ply % 2 == 0 else -1
    return rec, flip(after(root, d, a)), np.int8(1 + ((int(o[1]) * 6) >> 32)), game, drawn


def check_play(ea, tree, models, S, sims, boards, dice, game, temp_plies, key, off):
    """puct_play on clones of (boards, dice, game) against play_model, every byte; -> (record, game after, rows drawn from the visits)"""
    M = len(models)
    b, d, g = boards.clone(), dice.clone(), game.clone()
    out = ea.puct_play(tree, b, d, g, S, sims, temp_plies=temp_plies, key=key, game_offset=off)
    assert sorted(out) == sorted(ROWS)
    hb, hd, hg = boards.cpu().numpy(), dice.cpu().numpy(), game.cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    gb, gd, gg = b.cpu().numpy(), d.cpu().numpy(), g.cpu().numpy()
    drawn = []
    for m, mod in enumerate(models):
        rec, nb, nd, ng, dr = play_model(mod, hb[m], hd[m], hg[m], temp_plies, key, off + m)
        where = (m, temp_plies, key, off)
        assert np.array_equal(gb[m], nb) and int(gd[m]) == int(nd) and np.array_equal(gg[m], ng), (where, gg[m], ng)
        assert np.array_equal(got["board"][m], rec["board"]) and int(got["dice"][m]) == int(rec["dice"]), where
        assert np.array_equal(got["visits"][m].reshape(6), rec["visits"]) and np.array_equal(got["action"][m], rec["action"]), where
        assert got["value"][m].view(np.int32) == np.asarray(rec["value"], F).view(np.int32) and int(got["live"][m]) == int(rec["live"]), where
        if dr:
            a = 3 * int(rec["action"][0]) + int(rec["action"][1])
            assert mod.t["kind"][0, a] == 2 and mod.t["n"][0, a] > 0, where
            drawn.append(m)
    return out, g, drawn


def noise_rows(hb, hd, seed):
    """float32 [M, 6] per root: gamma variates; every fourth row all zeros; zeros on some legal edges; large numbers, inf, nan and
    negative numbers on the edges that are no actions"""
    M = hb.shape[0]
    eta = np.random.default_rng(seed).gamma(1.0, size=(M, 6)).astype(F) + F(1e-3)
    junk = np.array([1e30, np.inf, np.nan, -1.0, 3.0e38, -np.inf], F)
    for m in range(M):
        dead = hb[m][0, 0] < 0 or hb[m][-1, -1] > 0 or not (hb[m] > 0).any() or not (hb[m] < 0).any()
        kind = np.zeros(6, np.int8) if dead else edges(hb[m], min(max(int(hd[m]), 1), 6))[0]
        if m % 4 == 1:
            eta[m] = 0
        if m % 4 == 2:
            eta[m, np.nonzero(kind)[0][::2]] = 0                # the first, third .. legal edge: with one legal edge the sum is zero
        if m % 4 == 3 or M == 1:
            eta[m, kind == 0] = np.roll(junk, m)[kind == 0]
    return eta


_RUNS = {}


def noise_run(ea, S, M, sims, eps=0.25):
    """lock step with the noise entry point in every round, computed once per shape -> (tree, models, views, boards, dice)"""
    if (S, M, sims) in _RUNS:
        return _RUNS[(S, M, sims)]
    p = pool(ea, S)
    off = 100 * sims + 7
    b, d = p["boards"][off:off + M].clone(), p["dice"][off:off + M].clone()
    if M > 2:
        b[2] = boards_of(S, {(S - 1, S - 1): 2, (0, 1): -1})[0]  # a degenerate tree among live ones
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    eta = noise_rows(hb, hd, 1000 * S + 10 * M + sims)
    noise = torch.as_tensor(eta).cuda()
    tree, lb, ld = ea.puct_begin(b, d, sims)
    plain = [x.clone() for x in (tree, lb, ld)]
    models = [NoiseModel(hb[m], hd[m], sims, eta[m], eps) for m in range(M)]
    compare(ea, tree, lb, ld, models, S, sims, "begin")
    c, inv_tv, worst, worst_other, unchanged = F(1.5), F(1), 0.0, 0.0, 0
    for rnd in range(sims + 1):
        _, logits, value = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
        if rnd == 0:
            ea.puct_advance(plain[0], logits, value, plain[1], plain[2], sims)
            p_plain = host_views(ea, plain[0], S, sims)["p"][:, 0]
        out = ea.puct_advance(tree, logits.reshape(M, 5), value, lb, ld, sims, root_noise=noise.reshape(M, 2, 3), noise_eps=eps)
        assert out[0] is tree and out[1] is lb and out[2] is ld
        gp = host_views(ea, tree, S, sims)["p"]
        hl, hv = logits.cpu().numpy(), value.cpu().numpy()
        for m, mod in enumerate(models):
            ev = mod.advance(hl[m], hv[m], c, inv_tv, gp[m])
            if ev is None:
                continue
            err = float(np.abs(gp[m, ev[0]].astype(np.float64) - ev[1]).max())
            if ev[0] == 0:
                assert rnd == 0 and err <= NOISE_TOL, (m, gp[m, 0], ev[1])
                worst = max(worst, err)
                kind = mod.t["kind"][0]
                if not ((kind != 0) & np.isfinite(eta[m]) & (eta[m] > 0)).any():          # no weight: the plain priors, bit for bit
                    assert np.array_equal(gp[m, 0].view(np.int32), p_plain[m].view(np.int32)), m
                    unchanged += 1
            else:                                                                       # every other node: the plain priors' bound
                assert err <= P_TOL, (rnd, m, ev[0])
                worst_other = max(worst_other, err)
        v = compare(ea, tree, lb, ld, models, S, sims, "round %d" % rnd)
    print("S=%d M=%d sims=%d eps=%g: max |P_root - P_float64| %.3g (bound %.3g), other nodes %.3g (bound %.3g), %d roots without a weight" % (
        S, M, sims, eps, worst, NOISE_TOL, worst_other, P_TOL, unchanged))
    assert M < 4 or unchanged > 0
    _RUNS[(S, M, sims)] = (tree, models, v, b, d)
    return _RUNS[(S, M, sims)]


# ---------------------------------------------------------------- 1. noise_eps = 0 is the plain call

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 33, 70])
@pytest.mark.parametrize("sims", [1, 7, 40])
def test_zero_eps_is_the_plain_call(ea, S, M, sims):
    p = pool(ea, S)
    off = 100 * sims + 7
    b, d = p["boards"][off:off + M], p["dice"][off:off + M]
    noise = torch.as_tensor(noise_rows(b.cpu().numpy(), d.cpu().numpy(), 5)).cuda()
    x, y = ea.puct_begin(b, d, sims), ea.puct_begin(b, d, sims)
    for rnd in range(sims + 1):
        _, logits, value = ea.predict_policy(x[1], x[2], p["params"], return_logits=True, return_value=True)
        ea.puct_advance(x[0], logits, value, x[1], x[2], sims)
        ea.puct_advance(y[0], logits, value, y[1], y[2], sims, root_noise=noise, noise_eps=0.0)
        for s, t in zip(x, y):
            assert torch.equal(s, t), (rnd,)                     # all tree bytes and the leaf rows
    assert int(ea.puct_tree_views(y[0], S, sims)["count"].max()) > 1 or sims == 1


# ---------------------------------------------------------------- 2. lock step with noise

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 33, 70])
@pytest.mark.parametrize("sims", [1, 7, 40])
def test_lock_step_with_noise(ea, S, M, sims):
    tree, models, v, _, _ = noise_run(ea, S, M, sims)
    assert any(not m.degenerate for m in models) and (M <= 2 or models[2].degenerate)
    live = v["degenerate"] == 0
    assert np.array_equal(v["n"][:, 0].sum(1)[live], np.full(int(live.sum()), sims))


def test_the_noise_moves_the_search(ea):
    """eps = 1 with all the weight on one legal edge: the root's prior is that edge, and the first simulation takes it"""
    S, sims = 5, 1
    p = pool(ea, S)
    b, d = p["boards"][:64], p["dice"][:64]
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    eta, want = np.zeros((64, 6), F), np.full(64, -1)
    for m in range(64):
        if not Model(hb[m], hd[m], 1).degenerate:
            legal = np.nonzero(edges(hb[m], int(hd[m]))[0])[0]
            want[m] = legal[-1]
            eta[m, want[m]] = 2.5
    tree, lb, ld = ea.puct_begin(b, d, sims)
    _, logits, value = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
    ea.puct_advance(tree, logits, value, lb, ld, sims, root_noise=torch.as_tensor(eta).cuda(), noise_eps=1.0)
    v = host_views(ea, tree, S, sims)
    assert (want >= 0).sum() > 32
    for m in np.nonzero(want >= 0)[0]:
        assert v["p"][m, 0, want[m]] == 1.0 and v["p"][m, 0].sum() == 1.0
        if v["kind"][m, 0, want[m]] == 2:
            assert v["child"][m, 0, want[m]].max() == 1            # the one simulation went down that edge


# ---------------------------------------------------------------- 3. the move

@pytest.mark.parametrize("S,M,sims", [(5, 70, 40), (7, 70, 40), (5, 33, 7), (7, 33, 7), (7, 1, 1), (5, 1, 1)])
def test_play_against_the_model(ea, S, M, sims):
    tree, models, _, b, d = noise_run(ea, S, M, sims)
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    game[:, 0] = torch.arange(M, device="cuda") % 6               # plies 0 .. 5: below, at and above temp_plies = 3
    if M > 8:
        game[5, 1], game[5, 2] = 1, -1                            # a game that is over keeps its winner
        game[8, 1] = 1
    result = ea.puct_result(tree, S, sims).cpu().numpy()
    n_drawn = 0
    for temp_plies in (0, 3, 100):
        for key, off in KEYS:
            out, g, drawn = check_play(ea, tree, models, S, sims, b, d, game, temp_plies, key, off)
            n_drawn += len(drawn)
            live = out["live"].cpu().numpy() == 1
            if temp_plies == 0:
                assert not drawn and np.array_equal(out["action"].cpu().numpy()[live], result[live])
            else:
                assert all(int(game[m, 0]) < temp_plies for m in drawn)
            if M > 8:
                assert not live[5] and not live[8] and not live[2]
                assert g[5].tolist() == [5, 1, -1, 0] and g[8].tolist() == [2, 1, 0, 0]
                assert g[2].tolist() == [2, 1, 0, 0]                # the degenerate tree: over, without a winner
    assert n_drawn > 0 or M == 1
    # the draw follows the key and the game's number: other words, other moves somewhere
    if M == 70:
        acts = [ea.puct_play(tree, b.clone(), d.clone(), game.clone(), S, sims, temp_plies=100, key=k, game_offset=o)["action"] for k, o in KEYS]
        assert any(not torch.equal(acts[0], a) for a in acts[1:])


def constructed(ea, S):
    e = S - 1
    b = boards_of(S,
                  {(e - 1, e - 1): 1, (0, 0): 3, (1, e): -2},            # dice 2: flag 0 moves cube 1, whose diagonal reaches the corner
                  {(1, 1): 3, (0, 2): 5, (1, 2): -4},                    # dice 4: flag 0 moves cube 3, to the right it takes the last opposing cube
                  {(e - 1, e - 1): 6, (0, 1): 2, (2, 2): -1},            # dice 4: flag 1 moves cube 6 onto the corner
                  {(e, 1): 5, (0, e): -1, (1, e): -3},                   # one cube on the last row: it can only go right
                  {(e, e): 2, (0, 1): -1},                               # already won: degenerate
                  {(2, 2): -4})                                          # no cube of the mover's: degenerate
    return b, i8(2, 4, 4, 3, 1, 2)


@pytest.mark.parametrize("S", [5, 7])
def test_constructed_positions(ea, S):
    p = pool(ea, S)
    b, d = constructed(ea, S)
    sims = 12
    tree, models, v = lockstep(ea, S, b, d, p["params"], sims)
    for ply, winner in ((4, 1), (7, -1)):
        for temp_plies in (0, 100):
            game = torch.zeros((6, 4), dtype=torch.int32, device="cuda")
            game[:, 0] = ply
            out, g, drawn = check_play(ea, tree, models, S, sims, b, d, game, temp_plies, 99, 3)
            assert out["action"][:3].tolist() == [[0, 2], [0, 0], [1, 2]]                 # the win is played, whatever the visits
            assert g[:3].tolist() == [[ply + 1, 1, winner, 0]] * 3
            assert out["action"][3].tolist() == [0, 0] and g[3].tolist() == [ply + 1, 0, 0, 0]
            assert out["visits"][3].reshape(6).tolist() == [sims, 0, 0, 0, 0, 0] and (temp_plies == 0 or drawn == [3])
            assert out["live"].tolist() == [1, 1, 1, 1, 0, 0] and g[4:].tolist() == [[ply, 1, 0, 0]] * 2
    # a game that is over, and a degenerate tree: boards, dice and ply stay byte for byte, whatever they hold
    game = torch.tensor([[3, 1, 1, 0]] * 4 + [[9, 0, 0, 0]] * 2, dtype=torch.int32, device="cuda")
    fb = torch.full((6, S, S), 0x5A, dtype=torch.int8, device="cuda")
    fd = torch.full((6,), 0x5A, dtype=torch.int8, device="cuda")
    out = ea.puct_play(tree, fb, fd, game, S, sims, temp_plies=5, key=1)
    assert bool((fb == 0x5A).all()) and bool((fd == 0x5A).all()) and not out["live"].any()
    assert game.tolist() == [[3, 1, 1, 0]] * 4 + [[9, 1, 0, 0]] * 2
    for name in ROWS:
        assert not out[name].any()


@pytest.mark.parametrize("S", [5, 7])
def test_null_record_pointers_one_by_one(ea, S):
    tree, models, _, b, d = noise_run(ea, S, 33, 7)
    game = torch.zeros((33, 4), dtype=torch.int32, device="cuda")
    args = dict(temp_plies=4, key=77, game_offset=2 ** 33)
    b0, d0, g0 = b.clone(), d.clone(), game.clone()
    full = ea.puct_play(tree, b0, d0, g0, S, 7, **args)
    for skip in ROWS + (None,):
        out = {k: torch.full_like(full[k], 0x33) for k in ROWS if k != skip}
        if skip is not None and skip != "board":
            out[skip] = None                                      # None and a missing name both mean NULL
        b1, d1, g1 = b.clone(), d.clone(), game.clone()
        assert ea.puct_play(tree, b1, d1, g1, S, 7, out=out, **args) is out
        assert torch.equal(b1, b0) and torch.equal(d1, d0) and torch.equal(g1, g0)
        for k in ROWS:
            if k != skip:
                assert torch.equal(out[k].view(torch.uint8), full[k].view(torch.uint8)), (skip, k)
    only_state = ea.puct_play(tree, b.clone(), d.clone(), game.clone(), S, 7, out={}, **args)
    assert only_state == {}


# ---------------------------------------------------------------- 4. the driver

def reset_positions(ea, S, n=33):
    env = ea.VecEWN(n, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=n, philox_key=5)
    b, d = env.reset(seeds=(np.arange(n, dtype=np.uint64) + 21).astype(np.uint32))
    return b.clone(), d.clone()


def by_hand(ea, S, b, d, params, sims, T, key, off, eps=0.25, alpha=1.0, temp_plies=8, table=None, terminal_value=1.0):
    """selfplay_puct written out in the public calls, without the early exit.  table (an EndgameTable): a pending leaf that it covers is
    worth terminal_value * max_a q_exact instead of the value head's output, the substitution that
    test_gpu_lookahead_endgame.py::test_predict_puct_with_a_table_is_the_public_calls_composed writes out"""
    M = b.shape[0]
    cb, cd = b.clone(), d.clone()
    game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    rec = {k: torch.zeros((T, M) + s, dtype=dt, device="cuda") for k, (s, dt) in row_shapes(S).items()}
    for t in range(T):
        noise = ea.selfplay_noise(M, alpha, key, off, t)
        tree, lb, ld = ea.puct_begin(cb, cd, sims)
        for rnd in range(sims + 1):
            _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
            if table is not None:
                _, covered, q_exact = table.lookup(lb, ld, return_q=True)
                value = torch.where(covered, terminal_value * q_exact.reshape(M, 6).max(1).values, value)
            ea.puct_advance(tree, logits, value, lb, ld, sims, terminal_value=terminal_value, root_noise=noise if rnd == 0 else None,
                            noise_eps=eps)
        ea.puct_play(tree, cb, cd, game, S, sims, temp_plies=temp_plies, key=key, game_offset=off, out={k: rec[k][t] for k in rec})
    rec["live"] = rec["live"].view(torch.bool)
    rec["winner"], rec["plies"] = game[:, 2].contiguous(), game[:, 0].contiguous()
    rec["z"], rec["weight"] = ea.selfplay_outcomes(rec["winner"], rec["live"])
    return rec


def same_records(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, k
        assert torch.equal(x[k].contiguous().view(torch.uint8), y[k].contiguous().view(torch.uint8)), k


def check_rules(rec, S, T):
    """the records are games of EinStein wuerfelt nicht: every move by the numpy move model, every game won within the bound"""
    h = {k: v.cpu().numpy() for k, v in rec.items()}
    M = h["winner"].shape[0]
    assert h["board"].shape == (T, M, S, S) and h["visits"].shape == (T, M, 2, 3) and h["action"].shape == (T, M, 2)
    assert h["live"].dtype == np.bool_ and h["z"].shape == h["weight"].shape == h["live"].shape == (T, M)
    for m in range(M):
        n = int(h["plies"][m])
        assert 1 <= n <= (69 if S == 5 else 117)
        assert h["live"][:n, m].all() and not h["live"][n:, m].any()
        for k in ("board", "dice", "visits", "value", "action", "z", "weight"):
            assert not h[k][n:, m].any(), (k, m)
        for t in range(n):
            a = 3 * int(h["action"][t, m, 0]) + int(h["action"][t, m, 1])
            b1 = after(h["board"][t, m], h["dice"][t, m], a)
            won = b1[-1, -1] > 0 or not (b1 < 0).any()
            assert won == (t == n - 1), (m, t)
            if t + 1 < n:
                assert np.array_equal(h["board"][t + 1, m], flip(b1)) and 1 <= h["dice"][t + 1, m] <= 6
        assert h["winner"][m] == (1 if (n - 1) % 2 == 0 else -1)                          # the side that made the last move
        z = h["z"][:n, m]
        assert z[n - 1] == 1.0 and np.array_equal(z, np.where((np.arange(n) - (n - 1)) % 2 == 0, 1.0, -1.0).astype(F))
        assert (h["weight"][:n, m] == 1.0).all()
    return h


@pytest.mark.parametrize("S,T", [(5, 80), (7, 128)])
def test_the_driver_is_the_stages(ea, S, T):
    p = pool(ea, S)
    b, d = reset_positions(ea, S)
    kw = dict(sims=8, max_plies=T, key=11, game_offset=2 ** 32 + 5)
    got = ea.selfplay_puct(b, d, p["params"], **kw)
    same_records(got, by_hand(ea, S, b, d, p["params"], 8, T, 11, 2 ** 32 + 5))
    h = check_rules(got, S, T)
    print("%dx%d: 33 games of %d .. %d plies (mean %.1f), first mover wins %d" % (
        S, S, h["plies"].min(), h["plies"].max(), h["plies"].mean(), int((h["winner"] == 1).sum())))
    if S == 5:
        same_records(got, ea.selfplay_puct(b, d, p["params"], **kw))                      # the same key: the same bytes
        same_records(got, ea.selfplay_puct(b, d, p["params"], chunk=16, **kw))            # chunks of 16, 16 and 1
        same_records(got, ea.selfplay_puct(b, d, p["params"], check_every=1, **kw))
        other = ea.selfplay_puct(b, d, p["params"], **dict(kw, key=12))
        assert not torch.equal(other["action"], got["action"])
        check_rules(other, S, T)
        assert got["board"].data_ptr() != b.data_ptr() and torch.equal(b, reset_positions(ea, S)[0])   # the inputs are not changed


def table_openings(ea):
    """the (5, 2, 4) table, and 64 openings: the 33 of reset_positions, then 31 sampled positions with one or two cubes a side, neither
    side already won, under varied dice, which the table covers from ply 0"""
    import random
    from tests.test_gpu_endgame import board_of, sample
    from tests.test_gpu_lookahead_endgame import tab
    t, rng = tab(ea, 5), random.Random(64)
    b, d = reset_positions(ea, 5)
    fb = torch.as_tensor(np.stack([board_of(sample(rng, 5, t.max_cubes, t.max_total), 5) for _ in range(31)])).cuda()
    fd = torch.tensor([1 + i % 6 for i in range(31)], dtype=torch.int8, device="cuda")
    assert bool(t.lookup(fb, fd)[1].all()) and not bool(t.lookup(b, d)[1].any())
    assert len({int((x != 0).sum()) for x in fb}) > 1              # two, three and four cubes in all
    return t, torch.cat([b, fb]).contiguous(), torch.cat([d, fd]).contiguous()


def covered_roots(t, rec):
    """bool [T, M]: the recorded roots that the table covers (rows past a game's end are zero boards: not covered)"""
    T, M, S = rec["board"].shape[:3]
    cov = t.lookup(rec["board"].reshape(T * M, S, S), rec["dice"].reshape(T * M).clamp(min=1))[1].reshape(T, M)
    assert not bool((cov & ~rec["live"]).any())
    return cov


@pytest.mark.parametrize("tv", [1.0, 0.75])
def test_the_driver_with_a_table_is_the_stages(ea, tv):
    """selfplay_puct(endgame_table=) is by_hand(table=): late in a game most leaves are covered, and the overwritten leaf values meet
    the noise round and ewn_puct_play.  That the table is read is checked on the host: recorded roots that lookup covers"""
    S, T = 5, 80
    params = pool(ea, S)["params"]
    t, b, d = table_openings(ea)
    # key 15: of the keys 11 .. 20 the one whose by-hand games reach the most covered roots under both terminal values (key 11, the
    # plain test's, reaches 11 of them at terminal_value 1 and none at 0.75)
    kw = dict(sims=8, max_plies=T, key=15, game_offset=2 ** 32 + 5, terminal_value=tv)
    got = ea.selfplay_puct(b, d, params, endgame_table=t, **kw)
    want = by_hand(ea, S, b, d, params, 8, T, 15, 2 ** 32 + 5, table=t, terminal_value=tv)
    cov = covered_roots(t, want)                                         # counted on the by-hand run, before it is compared
    n_reset, n_few = int(cov[:, :33].sum()), int(cov[:, 33:].sum())
    print("tv=%g: %d recorded roots of the 33 reset games are covered (in %d of the games), %d of the 31 few-cube games; %d roots in all" % (
        tv, n_reset, int(cov[:, :33].any(0).sum()), n_few, int(want["live"].sum())))
    assert bool(cov[0, 33:].all()) and not bool(cov[0, :33].any())
    assert n_reset > 0                                                   # among the reset games' later plies
    same_records(got, want)
    check_rules(got, S, T)
    plain = ea.selfplay_puct(b, d, params, **kw)
    check_rules(plain, S, T)
    assert any(not torch.equal(plain[k], got[k]) for k in ("visits", "value", "action"))   # the table is read: other searches
    if tv == 1.0:                                                        # chunks of 16 and a host read every ply: the same bytes
        same_records(got, ea.selfplay_puct(b, d, params, endgame_table=t, chunk=16, **kw))
        same_records(got, ea.selfplay_puct(b, d, params, endgame_table=t, check_every=1, **kw))
        same_records(got, ea.selfplay_puct(b, d, params, endgame_table=t, chunk=16, check_every=1, **kw))


# ---------------------------------------------------------------- 5. guard zones

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib, M, sims = pool(ea, S), ea._lib.load(), 70, 40
    b, d = p["boards"][300:300 + M].contiguous(), p["dice"][300:300 + M].contiguous()
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    alloc = GuardedAllocator()
    z = lambda shape, dtype, tag: alloc.zeros(shape, dtype=dtype, tag=tag)  # noqa: E731
    tree, lb, ld = z((M, nb), torch.uint8, "tree"), z((M, S, S), torch.int8, "leaf_boards"), z((M,), torch.int8, "leaf_dice")
    logits, value, noise = z((M, 5), torch.float32, "logits"), z((M,), torch.float32, "value"), z((M, 6), torch.float32, "root_noise")
    cb, cd, game = z((M, S, S), torch.int8, "boards"), z((M,), torch.int8, "dice"), z((M, 4), torch.int32, "game")
    rec = dict(board=z((M, S, S), torch.int8, "rec_board"), dice=z((M,), torch.int8, "rec_dice"), visits=z((M, 6), torch.int32, "rec_visits"),
               value=z((M,), torch.float32, "rec_value"), action=z((M, 2), torch.int8, "rec_action"), live=z((M,), torch.int8, "rec_live"))
    noise.copy_(ea.selfplay_noise(M, 1.0, 3, 0, 0))
    cb.copy_(b)
    cd.copy_(d)
    assert lib.ewn_puct_begin(S, 3, M, sims, _ptr(cb), _ptr(cd), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) == 0
    for rnd in range(sims + 1):
        _, lg, val = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
        logits.copy_(lg)
        value.copy_(val)
        assert lib.ewn_puct_advance_noise(S, 3, M, sims, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(logits), _ptr(value), _ptr(noise),
                                          C.c_float(0.25), _ptr(lb), _ptr(ld), _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("advance_noise, M=70 sims=40")
    assert lib.ewn_puct_play(S, 3, M, _ptr(tree), _ptr(cb), _ptr(cd), _ptr(game), 8, C.c_uint64(9), C.c_int64(2 ** 40),
                             *[_ptr(rec[k]) for k in ROWS], _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("play, M=70 sims=40")
    live = rec["live"] == 1
    assert int(live.sum()) > 35 and bool((game[:, 0] == live.to(torch.int32)).all())
    assert int(rec["visits"].sum()) == sims * int(live.sum()) and not torch.equal(cb, b)


# ---------------------------------------------------------------- 6. the trainer

def selfplay_trainer(ea, **kw):
    from ewn_gym_amd.distill import PuctSelfPlayTrainer
    from tests.test_gpu_distill_trainer import make_env
    return PuctSelfPlayTrainer(make_env(ea, 64), **dict(dict(sims=6, seed=5, temp_plies=4, max_plies=16), **kw))


def targets_by_hand(rec, terminal_value=1.0):
    """the trainer's target arithmetic on selfplay_puct's records, written out -> (boards [R, S, S], dice [R], target_pi [R, 5],
    target_value [R], weight [R], one bool [R]: a recorded root whose two flags name one cube), R = T * M"""
    T, M, S = rec["board"].shape[:3]
    R = T * M
    b, d = rec["board"].reshape(R, S, S), rec["dice"].reshape(R).clamp(min=1)
    vis = rec["visits"].reshape(R, 2, 3).float()
    tot = vis.sum((1, 2))
    den = torch.where(tot > 0, tot, torch.ones_like(tot))[:, None]
    flag, direction = vis.sum(2) / den, vis.sum(1) / den
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    one = torch.tensor([bool(tot[i] > 0) and find_cube(cubes_of(hb[i], 1), int(hd[i]), False) == find_cube(cubes_of(hb[i], 1), int(hd[i]), True)
                        for i in range(R)], device="cuda")
    flag = torch.where(one[:, None], torch.full_like(flag, 0.5), flag)
    tp = (torch.cat([flag, direction], 1) * (tot > 0)[:, None]).contiguous()
    tv = (terminal_value * rec["z"]).reshape(R).contiguous()
    return b, d, tp, tv, rec["weight"].reshape(R).contiguous(), one


def test_one_update_with_a_table_is_the_public_calls_composed(ea, monkeypatch):
    """test_one_update_is_the_public_calls_composed with endgame_table=: the records are selfplay_puct's with the table, the gradient
    sup_grad's on them; the parts that the table does not change (the apply, the counters, the statistics) are tested there"""
    from tests.test_gpu_distill_trainer import make_env
    from tests.test_gpu_lookahead_endgame import tab
    N, T, t = 64, 16, tab(ea, 5)
    tr = selfplay_trainer(ea, endgame_table=t)
    assert tr.endgame_table is t and selfplay_trainer(ea).endgame_table is None
    params = tr.params.clone()
    lookups, lookup = [], t.lookup
    monkeypatch.setattr(t, "lookup", lambda *a, **kw: (lookups.append(a[0].shape[0]), lookup(*a, **kw))[1])
    tr.collect_and_update()
    monkeypatch.undo()
    assert lookups and len(lookups) % 7 == 0 and set(lookups) == {N}     # the search asked the table: sims + 1 rounds per ply, 64 leaf rows
    env = make_env(ea, N)
    b0, d0 = env.reset(seeds=(5 + np.arange(N, dtype=np.uint64)).astype(np.uint32))
    rec = ea.selfplay_puct(b0, d0, params, sims=6, max_plies=T, temp_plies=4, key=tr.noise_key, game_offset=0, endgame_table=t)
    same_records(rec, tr.records)
    b, d, tp, tv, w, one = targets_by_hand(rec)
    assert bool(one.any()) and 0 < float(w.sum()) < T * N
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    assert tr.num_timesteps == int(rec["live"].sum()) and tr.seed_counter == 1


def test_one_update_is_the_public_calls_composed(ea):
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    from tests.test_gpu_distill_trainer import make_env
    N, T = 64, 16                                                        # 16 plies: some games end within them, some do not
    tr = selfplay_trainer(ea)
    assert (tr.algorithm, tr.sims, tr.c_puct, tr.noise_eps, tr.noise_alpha, tr.temp_plies, tr.max_plies) == ("SELFPLAY", 6, 1.5, 0.25, 1.0, 4, 16)
    params = tr.params.clone()
    sq = torch.zeros_like(params)
    tr.collect_and_update()
    env = make_env(ea, N)                                                # by hand, on a second env: the first update's seeds are seed + lane
    b0, d0 = env.reset(seeds=(5 + np.arange(N, dtype=np.uint64)).astype(np.uint32))
    rec = ea.selfplay_puct(b0, d0, params, sims=6, max_plies=T, temp_plies=4, key=tr.noise_key, game_offset=0)
    same_records(rec, tr.records)
    R = T * N
    b, d, tp, tv, w, one = targets_by_hand(rec)
    live = rec["live"].reshape(R)
    unfinished = live & (w == 0)
    assert bool(one.any()) and bool(unfinished.any()) and 0 < float(w.sum()) < float(live.sum()) < R
    assert bool(((tp[:, :2].sum(1) - 1).abs() < 1e-6)[w > 0].all()) and bool((tv[w > 0].abs() == 1).all())
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    # rows that weigh nothing do not move the gradient, whatever their targets hold
    tp2, tv2 = tp.clone(), tv.clone()
    tp2[w == 0], tv2[w == 0] = float("nan"), 1e30
    tp2[unfinished] = 0.2
    assert torch.equal(bits(ea.sup_grad(b, d, tp2, tv2, params, weight=w, pi_coef=1.0, vf_coef=0.5)), bits(grad))
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    norm = torch.zeros(1, device="cuda")
    check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    assert torch.equal(bits(params), bits(tr.params)) and torch.equal(bits(sq), bits(tr.sq_avg))
    assert tr.num_timesteps == int(live.sum()) and tr.seed_counter == 1
    st = tr.stats_dict()
    assert abs(st["mean_game_length"] - float(rec["plies"].float().mean())) < 1e-4
    assert abs(st["finished_fraction"] - float((rec["winner"] != 0).float().mean())) < 1e-6 and 0 <= st["first_mover_win_fraction"] <= 1
    assert st["grad_norm"] > 0 and abs(st["live_fraction"] - float(w.sum()) / R) < 1e-6
    tr.collect_and_update()                                              # the second update plays other games
    assert not torch.equal(tr.records["dice"][0], rec["dice"][0]) and tr.seed_counter == 2       # other seeds: other first dice


def test_the_checkpoint_round_trips_and_resumes(ea, tmp_path):
    from ewn_gym_amd import tournament
    tr = selfplay_trainer(ea, c_puct=2.0, noise_eps=0.5, noise_alpha=0.75)
    tr.collect_and_update()
    path = str(tmp_path / "selfplay.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["fused"], sd["sims"], sd["c_puct"], sd["noise_eps"], sd["noise_alpha"], sd["temp_plies"], sd["seed_counter"]) == (
        "SELFPLAY", True, 6, 2.0, 0.5, 0.75, 4, 1)
    other = selfplay_trainer(ea, sims=3, temp_plies=0)
    other.load(path)
    assert (other.sims, other.c_puct, other.noise_eps, other.noise_alpha, other.temp_plies, other.seed_counter, other.num_timesteps) == (
        6, 2.0, 0.5, 0.75, 4, 1, tr.num_timesteps)
    assert torch.equal(bits(other.params), bits(tr.params)) and torch.equal(bits(other.sq_avg), bits(tr.sq_avg))
    tr.collect_and_update()
    other.collect_and_update()                                           # ... and goes on with the update the first one makes next
    same_records(other.records, tr.records)
    assert torch.equal(bits(other.params), bits(tr.params)) and torch.equal(bits(other.grad), bits(tr.grad))
    model = tournament.load_policy(path)                                 # read as the other fused checkpoints are
    assert torch.equal(bits(model.flat_parameters()), bits(sd["params"].cuda()))
    from ewn_gym_amd.distill import SearchDistillTrainer
    from tests.test_gpu_distill_trainer import make_env
    with pytest.raises(ValueError, match="not written by"):
        SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4).load(path)


def test_train_a2c_selfplay_end_to_end(ea, tmp_path):
    """one epoch of SELFPLAY with tiny numbers, in a fresh child process: the command line is what this test is about"""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SELFPLAY", "--num_envs", "64", "--sims", "4", "--epoch_num", "1",
                        "--timesteps_per_epoch", "300", "--eval_episode_num", "16", "--eval_opponent", "random", "--save_dir", str(tmp_path)],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert any(x.get("trainer") == "PuctSelfPlayTrainer" for x in lines)
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 1 and 300 <= ep[0]["timesteps"] <= 64 * 69 and math.isfinite(ep[0]["policy_loss"])
    assert 6 <= ep[0]["mean_game_length"] <= 69 and ep[0]["finished_fraction"] == 1.0
    sd = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["sims"], sd["noise_eps"], sd["temp_plies"], sd["seed_counter"]) == ("SELFPLAY", 4, 0.25, 8, 1)


def test_every_rank_counts_the_same_positions(ea, monkeypatch):
    """learn() loops on num_timesteps and every update ends in a collective: the count a rank adds must not depend on the lengths of
    its own games.  Two ranks are rehearsed on one trainer: the counters' all-reduce adds another rank's counts, whichever is larger"""
    from ewn_gym_amd import distill
    added = []
    for other in ([1000, 900, 60, 31], [5, 5, 1, 0]):                    # the other rank's live rows, plies, finished games, first-mover wins
        tr = selfplay_trainer(ea)
        tr.world = 2
        tr.hyper.world_size = 2
        monkeypatch.setattr(tr, "_all_reduce_grad", lambda: None)
        monkeypatch.setattr(distill, "all_reduce_counters", lambda c, other=other: c + torch.tensor(other, device=c.device))
        tr.collect_and_update()
        own = int(tr.records["live"].sum())
        assert tr.num_timesteps == (own + other[0]) // 2                 # what the other rank adds as well: half the sum
        st = tr.stats_dict()
        assert abs(st["mean_game_length"] - (float(tr.records["plies"].sum()) + other[1]) / 128) < 1e-9
        assert abs(st["finished_fraction"] - (int((tr.records["winner"] != 0).sum()) + other[2]) / 128) < 1e-9
        added.append(tr.num_timesteps)
    assert added[0] != added[1]
