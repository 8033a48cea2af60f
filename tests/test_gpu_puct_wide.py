"""The PUCT search in one launch with several leaves per tree and round (ewn_puct_search_wide, puct_search_wide, leaves=).
With leaves = 1 the yardstick is puct_search: all bytes of all trees.  With more leaves there is no other implementation to compare
with, and the yardstick is the definition as a numpy model (tests/test_puct_wide_cpu.py's WideModel, the extension of
tests/test_gpu_puct.py's Model): it takes its logits and values from predict_policy on its own leaf rows round by round, and every
section of every tree is compared, W and P by bit pattern.  As in the lock-step test of test_gpu_puct.py the priors are the one
tolerance: the kernel's P of a node lies within P_TOL of the float64 softmax product, and the model then adopts the kernel's bits.
1. leaves = 1.  2. the model.  3. geometry.  4. what the buffers held.  5. guard zones.  6. degenerate rows, dice.  7. the stream
contract.  8. the users."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_playout_search import sleep_cycles  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct import FIELDS, P_TOL, F, host_views  # noqa: E402
from tests.test_gpu_puct_fused import planted, rows, same  # noqa: E402
from tests.test_gpu_puct_selfplay import noise_rows, same_records, selfplay_trainer  # noqa: E402
from tests.test_puct_wide_cpu import WideModel  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def raw(ea, S, b, d, params, sims, leaves, tree, scratch, noise=None, eps=0.25, tile=0, blocks=0, c_puct=1.5, tv=1.0):
    """the entry itself, on the caller's buffers and the current stream"""
    from ewn_gym_amd.vec_env import _ptr, _stream
    rc = ea._lib.load().ewn_puct_search_wide(S, 3, b.shape[0], sims, leaves, C.c_float(c_puct), C.c_float(tv), _ptr(b), _ptr(d), _ptr(params),
                                             _ptr(noise), C.c_float(eps), tile, blocks, _ptr(tree), _ptr(scratch), _stream())
    assert rc == 0, rc
    return tree


def buffers(ea, S, M, sims, fill=0):
    lib = ea._lib.load()
    return (torch.full((M, lib.ewn_puct_tree_bytes(S, 3, sims)), fill, dtype=torch.uint8, device="cuda"),
            torch.full((lib.ewn_puct_search_wide_scratch_bytes(S, 3, M, sims),), fill, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- 1. leaves = 1 is puct_search

@pytest.mark.parametrize("S,M,sims", [(5, 9, 6), (5, 70, 17), (7, 33, 12)])
def test_one_leaf_is_puct_search(ea, S, M, sims):
    p = pool(ea, S)
    b, d = rows(ea, S, M, sims)
    eta = torch.as_tensor(noise_rows(b.cpu().numpy(), d.clamp(1, 6).cpu().numpy(), 100 * S + M)).cuda()
    want = ea.puct_search(b, d, p["params"], sims)
    same(ea.puct_search_wide(b, d, p["params"], sims, 1), want, "without noise")
    noisy = ea.puct_search(b, d, p["params"], sims, root_noise=eta, noise_eps=0.25)
    assert not torch.equal(noisy, want)
    same(ea.puct_search_wide(b, d, p["params"], sims, 1, root_noise=eta.reshape(M, 2, 3), noise_eps=0.25), noisy, "with noise")
    same(ea.puct_search_wide(b, d, p["params"], sims, 1, root_noise=eta, noise_eps=0.0), want, "eps 0 is the plain call")
    same(ea.puct_search_wide(b, d, p["params"], sims, 1, noise_eps=float("nan")), want, "without noise the weight is not read")
    same(ea.puct_search_wide(b, d, p["params"], sims, 1, c_puct=0.5, terminal_value=2.0, tile=3, blocks=2),
         ea.puct_search(b, d, p["params"], sims, c_puct=0.5, terminal_value=2.0), "other constants, another geometry")


# ---------------------------------------------------------------- 2. more leaves: the model

_STATS = {}


def against_the_model(ea, S, b, d, params, sims, L, got, c_puct=1.5, tv=1.0, where=""):
    """WideModel beside the kernel's finished trees `got` -> the models.  Round by round the models' pending rows go through one
    predict_policy call; a model adopts the kernel's final P of the node it evaluates, held to P_TOL against the float64 softmax"""
    hb, hd = b.cpu().numpy(), d.cpu().numpy()
    M = hb.shape[0]
    v = host_views(ea, got, S, sims)
    models = [WideModel(hb[m], hd[m], sims, L) for m in range(M)]
    c, inv_tv, pmax = F(c_puct), F(F(1) / F(tv)), 0.0
    for _ in range(sims + 1):                                      # at most sims + 1 rounds
        busy = [m for m in range(M) if models[m].busy()]
        if not busy:
            break
        obs = [r for m in busy for r in models[m].rows()]
        hl, hv = np.zeros((0, 5), F), np.zeros(0, F)
        if obs:
            lb = torch.as_tensor(np.stack([r[0] for r in obs])).cuda()
            ld = torch.as_tensor(np.array([r[1] for r in obs], np.int8)).cuda()
            _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
            hl, hv = logits.cpu().numpy(), value.cpu().numpy()
        k = 0
        for m in busy:
            n = len(models[m].pend)
            for j, p64 in models[m].round([(hl[k + i], hv[k + i]) for i in range(n)], c, inv_tv, v["p"][m]):
                err = float(np.abs(v["p"][m, j].astype(np.float64) - p64).max())
                pmax = max(pmax, err)
                assert err <= P_TOL, (where, m, j, v["p"][m, j], p64)
            k += n
    assert not any(mod.busy() for mod in models), where
    print("%s S=%d M=%d sims=%d L=%d: max |P - P_float64| %.3g (bound %.3g); rounds at most %d, wide rounds %d, collisions %d" % (
        where, S, M, sims, L, pmax, P_TOL, max(mod.rounds for mod in models), sum(mod.wide_rounds for mod in models),
        sum(mod.collisions for mod in models)))
    for name in ("count", "done", "pending", "degenerate"):
        want = np.array([int(getattr(mod, name)) for mod in models], np.int32)
        assert np.array_equal(v[name], want), (where, name, v[name], want)
    for name in FIELDS:
        want = np.stack([mod.t[name] for mod in models])
        assert np.array_equal(v[name], want), (where, name, np.argwhere(v[name] != want)[:4])
    for name in ("w", "p"):                                        # by bit pattern
        want = np.stack([mod.t[name] for mod in models])
        assert np.array_equal(v[name].view(np.int32), want.view(np.int32)), (where, name, np.argwhere(v[name] != want)[:4])
    for mod in models:
        assert not mod.vn.any() and not mod.vcn.any() and (mod.degenerate or mod.done == sims)
    return models


CASES = [(5, 9, 12, 4, None), (5, 33, 40, 8, None), (7, 9, 20, 32, None), (5, 5, 5, 32, None), (7, 70, 17, 3, 1)]


@pytest.mark.parametrize("S,M,sims,L,blocks", CASES)
def test_more_leaves_against_the_model(ea, S, M, sims, L, blocks):
    p = pool(ea, S)
    b, d = rows(ea, S, M, sims)
    got = ea.puct_search_wide(b, d, p["params"], sims, L, blocks=blocks)
    models = against_the_model(ea, S, b, d, p["params"], sims, L, got, where="case")
    assert sum(mod.wide_rounds for mod in models) > 0                # rounds that collected at least two leaves
    assert max(mod.rounds for mod in models) < sims + 1              # ... and so fewer rounds than simulations
    _STATS[(S, M, sims, L)] = sum(mod.collisions for mod in models)
    if blocks is not None:
        same(ea.puct_search_wide(b, d, p["params"], sims, L), got, "the default grid")


def test_the_collision_rule_fires_at_32_leaves(ea):
    for S, M, sims, L, blocks in CASES:
        if L == 32 and (S, M, sims, L) not in _STATS:                # run alone: the cases are searched here
            p = pool(ea, S)
            b, d = rows(ea, S, M, sims)
            models = against_the_model(ea, S, b, d, p["params"], sims, L, ea.puct_search_wide(b, d, p["params"], sims, L), where="again")
            _STATS[(S, M, sims, L)] = sum(mod.collisions for mod in models)
    assert sum(n for (S, M, sims, L), n in _STATS.items() if L == 32) > 0


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("sims", [0, 1])
def test_no_and_one_simulation(ea, S, sims):
    p = pool(ea, S)
    b, d = rows(ea, S, 33, 7)
    for L in (4, 32):
        got = ea.puct_search_wide(b, d, p["params"], sims, L)
        against_the_model(ea, S, b, d, p["params"], sims, L, got, where="sims %d" % sims)
        same(got, ea.puct_search(b, d, p["params"], sims), "one leaf at a time: puct_search")   # a budget of 0 or 1 never has two leaves


@pytest.mark.parametrize("S", [5, 7])
def test_other_constants_and_the_planted_rows(ea, S):
    from tests.test_gpu_puct import biased_params
    pb, pd, dead = planted(S)
    params = biased_params(S, 4)                                   # the winning direction gets a prior of about e^-12
    for sims, L, c_puct, tv in ((12, 4, 1.5, 1.0), (9, 8, 0.0, 10.0), (7, 2, 2.5, 0.75)):
        got = ea.puct_search_wide(pb, pd, params, sims, L, c_puct=c_puct, terminal_value=tv)
        models = against_the_model(ea, S, pb, pd, params, sims, L, got, c_puct=c_puct, tv=tv, where="planted")
        assert [mod.degenerate for mod in models] == dead


# ---------------------------------------------------------------- 3. geometry

@pytest.mark.parametrize("S,M,sims,L", [(5, 33, 12, 4), (7, 9, 8, 16), (5, 70, 7, 3)])
def test_tile_and_blocks_change_no_byte(ea, S, M, sims, L):
    p = pool(ea, S)
    b, d = rows(ea, S, M, sims)
    want = ea.puct_search_wide(b, d, p["params"], sims, L)
    for tile in sorted({1, 2, 32 // L}):
        for blocks in (1, None):
            same(ea.puct_search_wide(b, d, p["params"], sims, L, tile=tile, blocks=blocks), want, "tile %d, blocks %s" % (tile, blocks))
    same(ea.puct_search_wide(b[:M - 4], d[:M - 4], p["params"], sims, L), want[:M - 4], "a tree does not depend on its neighbours")


# ---------------------------------------------------------------- 4. what the buffers held does not matter

@pytest.mark.parametrize("S", [5, 7])
def test_what_the_buffers_held_does_not_matter(ea, S):
    p, M, sims, L = pool(ea, S), 33, 12, 4
    b, d = rows(ea, S, M, sims)
    want = ea.puct_search_wide(b, d, p["params"], sims, L)
    for fill in (0x00, 0xFF, 0x7F):                                # zeros; a NaN in every float and -1 in every count; huge numbers
        tree, scratch = buffers(ea, S, M, sims, fill)
        same(raw(ea, S, b, d, p["params"], sims, L, tree, scratch), want, "fill %#x" % fill)
        same(raw(ea, S, b, d, p["params"], sims, L, tree, scratch, tile=2, blocks=3), want, "and again on what the last call left")
        out = torch.full_like(tree, fill)
        assert ea.puct_search_wide(b, d, p["params"], sims, L, out=out) is out
        same(out, want, "out=, fill %#x" % fill)


# ---------------------------------------------------------------- 5. guard zones

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    p, M, sims = pool(ea, S), 33, 12
    lib = ea._lib.load()
    b, d = rows(ea, S, M, sims)
    nb, ns = lib.ewn_puct_tree_bytes(S, 3, sims), lib.ewn_puct_search_wide_scratch_bytes(S, 3, M, sims)
    alloc = GuardedAllocator()
    gb = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards")
    gd = alloc.zeros((M,), dtype=torch.int8, tag="dice")
    gp = alloc.zeros((p["params"].numel(),), dtype=torch.float32, tag="params")
    gn = alloc.zeros((M, 6), dtype=torch.float32, tag="noise")
    gb.copy_(b)
    gd.copy_(d)
    gp.copy_(p["params"])
    gn.fill_(1.0)
    for L, tile, blocks in ((4, 0, 0), (32, 0, 0), (3, 10, 1)):
        want = ea.puct_search_wide(b, d, p["params"], sims, L, root_noise=gn.clone(), noise_eps=0.25)
        tree = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree, L %d" % L, offset=4)          # 4 bytes past a 16-byte boundary
        scratch = alloc.zeros((ns,), dtype=torch.uint8, tag="scratch, L %d" % L, offset=4)
        assert tree.data_ptr() % 16 == 4 and scratch.data_ptr() % 16 == 4
        raw(ea, S, gb, gd, gp, sims, L, tree, scratch, noise=gn, tile=tile, blocks=blocks)
        alloc.check("search, L %d" % L)
        same(tree, want, "in guarded buffers")
        plain = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree without noise, L %d" % L, offset=4)
        raw(ea, S, gb, gd, gp, sims, L, plain, scratch, tile=tile, blocks=blocks)
        alloc.check("search without noise, L %d" % L)
        same(plain, ea.puct_search_wide(b, d, p["params"], sims, L), "without noise")


# ---------------------------------------------------------------- 6. degenerate and already-won rows; dice

@pytest.mark.parametrize("S", [5, 7])
def test_degenerate_rows_among_live_ones_and_dice_outside_the_range(ea, S):
    p, sims, L = pool(ea, S), 10, 4
    pb, pd, dead = planted(S)
    live = p["boards"][:14]
    b = torch.stack([pb, live], 1).reshape(28, S, S).contiguous()  # a degenerate or constructed row, a row of play, ...
    d = torch.stack([pd, p["dice"][:14]], 1).reshape(28).contiguous()
    got = ea.puct_search_wide(b, d, p["params"], sims, L)
    models = against_the_model(ea, S, b, d, p["params"], sims, L, got, where="degenerate rows")
    v = host_views(ea, got, S, sims)
    is_dead = np.array([x for flag in dead for x in (flag, False)])
    assert np.array_equal(v["degenerate"] == 1, is_dead) and [mod.degenerate for mod in models] == is_dead.tolist()
    assert (v["count"][is_dead] == 1).all() and (v["done"][is_dead] == 0).all() and (v["pending"] == -1).all()
    assert (v["done"][~is_dead] == sims).all()
    same(ea.puct_search_wide(live, p["dice"][:14], p["params"], sims, L), got[1::2], "... without disturbing their neighbours")
    act, visits = ea.predict_puct(b, d, p["params"], sims=sims, leaves=L, return_visits=True)
    assert not act[torch.as_tensor(is_dead).cuda()].any() and not visits[torch.as_tensor(is_dead).cuda()].any()
    for bad, good in ((0, 1), (7, 6), (-128, 1), (127, 6)):
        x = ea.puct_search_wide(live, torch.full((14,), bad, dtype=torch.int8, device="cuda"), p["params"], sims, L)
        y = ea.puct_search_wide(live, torch.full((14,), good, dtype=torch.int8, device="cuda"), p["params"], sims, L)
        same(x, y, "dice %d is dice %d" % (bad, good))
    assert host_views(ea, x, S, sims)["dice"][:, 0].tolist() == [6] * 14


# ---------------------------------------------------------------- 7. the stream contract

STREAM_SHAPES = [(5, 9, 12, 4), (7, 33, 8, 32)]


@pytest.mark.parametrize("S,M,sims,L", STREAM_SHAPES)
def test_a_side_stream_is_honoured(ea, S, M, sims, L):
    """on a side stream behind a sleep: the copy of B into the inputs, the fill of the buffers, the call, the copy of the tree.  Only
    that stream is synchronised.  A launch on any other stream reads A behind the sleep's back and is overwritten by the fill."""
    p = pool(ea, S)
    bB, dB = rows(ea, S, M, sims)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    EA, EB = ea.puct_search_wide(bA, dA, p["params"], sims, L), ea.puct_search_wide(bB, dB, p["params"], sims, L)
    assert not torch.equal(EA, EB)
    b, d = bA.clone(), dA.clone()
    tree, scratch = buffers(ea, S, M, sims, 0x3C)
    cycles = sleep_cycles()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        b.copy_(bB)
        d.copy_(dB)
        tree.fill_(0xA5)
        scratch.fill_(0xA5)
        raw(ea, S, b, d, p["params"], sims, L, tree, scratch)
        got = tree.clone()
    s.synchronize()
    same(got, EB, "on a side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,M,sims,L", STREAM_SHAPES)
def test_a_captured_graph_replays_like_eager_calls(ea, S, M, sims, L):
    """captured once, replayed three times -- on A, on B, on A again, the buffers refilled between -- against three eager calls"""
    p = pool(ea, S)
    bB, dB = rows(ea, S, M, sims)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    eager = [ea.puct_search_wide(xb, xd, p["params"], sims, L) for xb, xd in ((bA, dA), (bB, dB), (bA, dA))]
    assert torch.equal(eager[0], eager[2]) and not torch.equal(eager[0], eager[1])
    b, d = bA.clone(), dA.clone()
    tree, scratch = buffers(ea, S, M, sims, 0x5A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        raw(ea, S, b, d, p["params"], sims, L, tree, scratch)
    torch.cuda.synchronize()
    assert bool((tree == 0x5A).all()) and bool((scratch == 0x5A).all()), "the captured call ran during the capture"
    for k, (xb, xd) in enumerate(((bA, dA), (bB, dB), (bA, dA))):
        b.copy_(xb)
        d.copy_(xd)
        tree.fill_(0xA5)
        scratch.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        same(tree, eager[k], "replay %d" % (k + 1))


# ---------------------------------------------------------------- 8. the users

@pytest.mark.parametrize("S", [5, 7])
def test_predict_puct_takes_leaves(ea, S):
    p = pool(ea, S)
    b, d = rows(ea, S, 70, 40)
    kw = dict(sims=16, c_puct=1.25, terminal_value=2.0)
    tree = ea.puct_search_wide(b, d, p["params"], 16, 4, c_puct=1.25, terminal_value=2.0)
    want = ea.puct_result(tree, S, 16, return_visits=True, return_q=True, return_value=True)
    for extra in ({}, {"chunk": 32}, {"fused": True}):
        got = ea.predict_puct(b, d, p["params"], leaves=4, return_visits=True, return_q=True, return_value=True, **extra, **kw)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(ea.predict_puct(b, d, p["params"], leaves=4, **kw), want[0])
    one = ea.predict_puct(b, d, p["params"], return_visits=True, **kw)
    assert torch.equal(one[1], ea.predict_puct(b, d, p["params"], leaves=1, return_visits=True, **kw)[1])
    assert not torch.equal(one[1], want[1]) and torch.equal(one[1].sum((1, 2)), want[1].sum((1, 2)))   # other trees, the same budget


@pytest.mark.parametrize("S", [5, 7])
def test_selfplay_puct_takes_leaves(ea, S):
    """per ply the wide search with that ply's selfplay_noise rows, then puct_play"""
    p = pool(ea, S)
    M, sims, T, key, off = 9, 8, 12, 11, 5
    b, d = p["boards"][:M], p["dice"][:M]
    kw = dict(sims=sims, max_plies=T, temp_plies=4, key=key, game_offset=off)
    rec = ea.selfplay_puct(b, d, p["params"], leaves=4, **kw)
    same_records(ea.selfplay_puct(b, d, p["params"], leaves=4, chunk=4, fused=True, **kw), rec)
    cb, cd, game = b.clone(), d.clone(), torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    for t in range(T):
        eta = ea.selfplay_noise(M, 1.0, key, off, t)
        tree = ea.puct_search_wide(cb, cd, p["params"], sims, 4, root_noise=eta, noise_eps=0.25)
        row = ea.puct_play(tree, cb, cd, game, S, sims, temp_plies=4, key=key, game_offset=off)
        for name, x in row.items():
            y = rec[name][t]
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (t, name)
    assert torch.equal(game[:, 2], rec["winner"]) and torch.equal(game[:, 0], rec["plies"]) and int(rec["live"].sum()) > M
    assert not torch.equal(rec["visits"], ea.selfplay_puct(b, d, p["params"], **kw)["visits"])


def test_the_agent_and_the_tournament(ea):
    from classical_policies import PuctAgent
    from envs import EinsteinWuerfeltNichtEnv
    from ewn_gym_amd import tournament
    p = pool(ea, 5)
    agent = PuctAgent(p["model"], board_size=5, sims=8, leaves=4)
    env = EinsteinWuerfeltNichtEnv(board_size=5, seed=3)
    obs, _ = env.reset(seed=3)
    for _ in range(60):
        action, state = agent.predict(obs)
        assert state is None and action.shape == (2,)
        obs, _, terminated, truncated, _ = env.step(action)
        if terminated or truncated:
            break
    assert terminated or truncated                                       # one whole episode
    b, d = p["boards"][:9], p["dice"][:9]
    act, visits = agent.predict_batch(b, d, return_visits=True)
    want = ea.predict_puct(b, d, p["params"], sims=8, leaves=4, return_visits=True)
    assert torch.equal(act, want[0]) and torch.equal(visits, want[1])
    spec = {"kind": "mlp_puct", "model": p["model"], "sims": 8, "leaves": 4}
    r = [tournament.evaluate(spec, {"kind": "random"}, num=64, board_size=5) for _ in range(2)]
    assert r[0]["episodes"] == 64 and 0 <= r[0]["wins"] <= 64
    assert r[0]["wins"] == r[1]["wins"] and torch.equal(r[0]["scores"], r[1]["scores"]) and torch.equal(r[0]["lengths"], r[1]["lengths"])


def test_the_trainers_take_leaves(ea, tmp_path):
    from ewn_gym_amd.distill import SearchDistillTrainer
    from tests.test_gpu_distill_trainer import make_env
    a, again, one = selfplay_trainer(ea, leaves=4), selfplay_trainer(ea, leaves=4), selfplay_trainer(ea)
    assert (a.leaves, one.leaves) == (4, 1)
    for tr in (a, again, one):
        tr.collect_and_update()
    same_records(a.records, again.records)
    assert torch.equal(bits(a.grad), bits(again.grad)) and torch.equal(bits(a.params), bits(again.params))
    assert not torch.equal(a.records["visits"], one.records["visits"]) and not torch.equal(bits(a.grad), bits(one.grad))
    path = str(tmp_path / "selfplay.pt")
    a.save(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["leaves"] == 4
    one.load(path)
    assert one.leaves == 4
    x = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=8, leaves=4)
    y = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=8, leaves=4)
    z = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=8)
    for tr in (x, y, z):
        tr.collect_and_update()
    assert torch.equal(bits(x.grad), bits(y.grad)) and not torch.equal(bits(x.grad), bits(z.grad))
    x.save(path)
    z.load(path)
    assert z.leaves == 4 and (z.search, z.sims) == ("puct", 8)


def test_leaves_with_a_table_or_whole_games_is_refused(ea):
    from tests.test_gpu_distill_trainer import make_env
    from tests.test_gpu_endgame import table
    p = pool(ea, 5)
    t = table(ea, 5, 2, 4)
    b, d = p["boards"][:9], p["dice"][:9]
    with pytest.raises(ValueError, match="predict_puct: leaves=4 does not take endgame_table"):
        ea.predict_puct(b, d, p["params"], sims=4, leaves=4, endgame_table=t)
    with pytest.raises(ValueError, match="selfplay_puct: leaves=4 does not take endgame_table"):
        ea.selfplay_puct(b, d, p["params"], sims=4, leaves=4, endgame_table=t)
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: leaves=4 does not take whole_games=True"):
        selfplay_trainer(ea, leaves=4, whole_games=True)
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: leaves=4 does not take endgame_table"):
        selfplay_trainer(ea, leaves=4, endgame_table=t)
    assert ea.predict_puct(b, d, p["params"], sims=4, leaves=1, endgame_table=t).shape == (9, 2)      # leaves = 1: as before
