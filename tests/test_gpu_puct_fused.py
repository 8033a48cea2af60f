"""The PUCT search in one launch (ewn_puct_search, puct_search, fused=True) against the staged path driven through the
public stage calls: puct_begin, then rounds of predict_policy on the leaf rows and puct_advance (the first with root noise where noise
is given).  The definition, the tree code (csrc/ewn_puct.hpp), the network code and the compiler flags are the same on both paths,
so there is no tolerance anywhere in this file: every comparison is of all bytes of all trees, and any difference is a bug.
How many trees share a block changes no byte either: the small batches here run under the default choice (which gives every tree a
block of its own up to 256 trees) and again with full 32-tree tiles (EWN_PUCT_TILE, read at every call).
1. lock step by rounds.  2. noise.  3. past one grid trip.  4. buffers.  5. a large budget.  6. the users of the search."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, i8  # noqa: E402
from tests.test_gpu_predict_policy import bits, pool  # noqa: E402
from tests.test_gpu_puct import biased_params, check_invariants, host_views  # noqa: E402
from tests.test_gpu_puct_selfplay import noise_rows, same_records  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def planted(S):
    """the rows of test_gpu_puct.py's constructed positions -> (boards [14, S, S], dice [14], which of them are degenerate)"""
    e = S - 1
    b = boards_of(S,
                  {(e, e): 2, (0, 1): -1},                               # 0: already won
                  {(e - 1, e - 1): 1, (0, 0): 3, (1, e): -2},            # 1: dice 2, flag 0 moves cube 1, whose diagonal reaches the corner
                  {(0, 0): -3, (2, 2): 1},                               # 2: already lost
                  {(e - 1, e - 1): 6, (0, 1): 2, (2, 2): -1},            # 3: dice 4, flag 1 moves cube 6 onto the corner
                  {(2, 2): -4},                                          # 4: no agent cube
                  {(e, 1): 5, (0, e): -1, (1, e): -3},                   # 5: the only cube, on the last row: it can only go right
                  {(1, 1): 2},                                           # 6: no opposing cube
                  {(e, 1): 1, (e, 2): 2, (0, e): -6},                    # 7: dice 1, cube 1 on the last row takes its own cube 2
                  {},                                                    # 8: an empty board
                  {(1, 1): 3, (0, 2): 5, (1, 2): -4},                    # 9: dice 4, flag 0 takes the last opposing cube
                  # 10 .. 13: four cubes, both sides one step from their corners: many simulations end on winning edges
                  {(e - 1, e - 1): 1, (e - 2, e - 2): 2, (1, 1): -1, (2, 2): -2},
                  {(e - 1, e): 3, (e - 2, e - 1): 4, (1, 0): -5, (2, 1): -6},
                  {(e, e - 1): 1, (e - 1, e - 2): 6, (0, 1): -1, (1, 2): -6},
                  {(e - 1, e - 1): 2, (e - 2, e - 1): 5, (1, 1): -2, (1, 2): -5})
    d = i8(1, 2, 3, 4, 4, 3, 5, 1, 5, 4, 2, 4, 6, 1)
    dead = [True, False, True, False, True, False, True, False, True, False, False, False, False, False]
    return b, d, dead


_ROWS = {}


def rows(ea, S, M, sims):
    """M observations, computed once and left unchanged: random play; from 31 rows on the planted rows among them, degenerate ones
    between live ones, and dice 0, 7, -128, 127 on four live rows"""
    if (S, M, sims) not in _ROWS:
        p = pool(ea, S)
        off = 100 * sims + 300
        b, d = p["boards"][off:off + M].clone(), p["dice"][off:off + M].clone()
        if M >= 31:
            pb, pd, _ = planted(S)
            b[1:29:2], d[1:29:2] = pb, pd                      # rows 1, 3 .. 27: a plain row between any two of them
            d[[0, 2, 4, 6]] = i8(0, 7, -128, 127)
        _ROWS[(S, M, sims)] = (b.contiguous(), d.contiguous())
    return _ROWS[(S, M, sims)]


def staged(ea, b, d, params, sims, rounds=None, c_puct=1.5, tv=1.0, noise=None, eps=0.25, keep=True):
    """the yardstick: begin, then rounds of predict_policy and advance -> the trees after begin and after every round (clones);
    keep=False: the final trees alone, [tree]"""
    tree, lb, ld = ea.puct_begin(b, d, sims)
    snaps = [tree.clone()] if keep else []
    for rnd in range(sims + 1 if rounds is None else rounds):
        _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        ea.puct_advance(tree, logits, value, lb, ld, sims, c_puct=c_puct, terminal_value=tv,
                        root_noise=noise if rnd == 0 else None, noise_eps=eps)
        if keep:
            snaps.append(tree.clone())
    return snaps if keep else [tree]


def same(got, want, where):
    assert got.dtype == want.dtype == torch.uint8 and got.shape == want.shape, where
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(1)).reshape(-1)
        m = int(bad[0])
        raise AssertionError("%s: %d of %d trees differ, the first is tree %d at bytes %s" % (
            where, int(bad.numel()), got.shape[0], m, torch.nonzero(got[m] != want[m]).reshape(-1)[:8].tolist()))


# ---------------------------------------------------------------- 1. lock step by rounds

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 31, 33, 70])       # either side of a 32-column tile, and tiles of 32, 32 and 6
@pytest.mark.parametrize("sims", [1, 7, 40])
def test_lock_step_by_rounds(ea, monkeypatch, S, M, sims):
    p = pool(ea, S)
    b, d = rows(ea, S, M, sims)
    want = staged(ea, b, d, p["params"], sims)
    assert len(want) == sims + 2
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        for r in range(sims + 2):
            same(ea.puct_search(b, d, p["params"], sims, rounds=r), want[r], "tile %s, %d rounds" % (tile, r))
        same(ea.puct_search(b, d, p["params"], sims), want[-1], "tile %s, all rounds" % tile)
        same(ea.puct_search(b, d, p["params"], sims, rounds=sims + 9), want[-1], "tile %s, more rounds than there are" % tile)
    monkeypatch.setenv("EWN_PUCT_TILE", "5")
    same(ea.puct_search(b, d, p["params"], sims), want[-1], "tile 5")
    v = host_views(ea, want[-1], S, sims)
    check_invariants(v, sims)                                  # the yardstick is a finished search
    assert (v["degenerate"] == 0).any() and (M < 31 or (v["degenerate"] == 1).sum() >= 5)
    if sims == 40 and M == 70:
        assert int(v["count"].max()) > 8                       # trees with depth


@pytest.mark.parametrize("S", [5, 7])
def test_the_planted_rows_alone_and_other_constants(ea, monkeypatch, S):
    pb, pd, dead = planted(S)
    params = biased_params(S, 4)                               # the winning direction gets a prior of about e^-12
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        for sims, c_puct, tv in ((12, 1.5, 1.0), (7, 0.0, 10.0), (3, 2.5, 0.75)):
            want = staged(ea, pb, pd, params, sims, c_puct=c_puct, tv=tv)
            for r in (0, 1, 2, sims, sims + 1):
                same(ea.puct_search(pb, pd, params, sims, c_puct=c_puct, terminal_value=tv, rounds=r), want[r], (tile, sims, r))
    v = host_views(ea, want[-1], S, 3)
    assert v["degenerate"].tolist() == [int(x) for x in dead]


@pytest.mark.parametrize("S", [5, 7])
def test_no_simulations(ea, S):
    p = pool(ea, S)
    b, d = rows(ea, S, 33, 7)
    want = staged(ea, b, d, p["params"], 0)
    assert len(want) == 2
    same(ea.puct_search(b, d, p["params"], 0, rounds=0), want[0], "begin")
    same(ea.puct_search(b, d, p["params"], 0, rounds=1), want[1], "the root's evaluation")
    same(ea.puct_search(b, d, p["params"], 0), want[1], "all rounds")
    act = ea.puct_result(ea.puct_search(b, d, p["params"], 0), S, 0)
    assert torch.equal(act, ea.predict_puct(b, d, p["params"], sims=0))


# ---------------------------------------------------------------- 2. noise

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M,sims", [(1, 1), (33, 7), (70, 40)])
def test_noise(ea, monkeypatch, S, M, sims):
    p = pool(ea, S)
    b, d = rows(ea, S, M, sims)
    eta = torch.as_tensor(noise_rows(b.cpu().numpy(), d.clamp(1, 6).cpu().numpy(), 1000 * S + 10 * M + sims)).cuda()
    assert M == 1 or (bool((eta[1::4] == 0).all()) and bool(torch.isnan(eta).any()) and bool(torch.isinf(eta).any()))   # the awkward rows
    plain = staged(ea, b, d, p["params"], sims, keep=False)[0]
    want = staged(ea, b, d, p["params"], sims, noise=eta, eps=0.25)
    assert M == 1 or not torch.equal(want[-1], plain)
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        same(ea.puct_search(b, d, p["params"], sims, root_noise=eta, noise_eps=0.0), plain, "eps 0 is the plain call")
        same(ea.puct_search(b, d, p["params"], sims, noise_eps=float("nan")), plain, "without noise the weight is not read")
        for r in sorted({0, 1, 2, sims, sims + 1}):
            same(ea.puct_search(b, d, p["params"], sims, root_noise=eta.reshape(M, 2, 3), noise_eps=0.25, rounds=r), want[r],
                 "tile %s, %d rounds" % (tile, r))
    full = staged(ea, b, d, p["params"], sims, noise=eta, eps=1.0, keep=False)[0]
    same(ea.puct_search(b, d, p["params"], sims, root_noise=eta, noise_eps=1.0), full, "eps 1")


# ---------------------------------------------------------------- 3. past one grid trip

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("extra", [1, 6])            # the tile of a block's second trip holds one tree, or six with planted rows
def test_past_one_grid_trip(ea, S, extra):
    from ewn_gym_amd.vec_env import PUCT_FUSED_MAX_BLOCKS, PUCT_FUSED_TILE
    trip = PUCT_FUSED_MAX_BLOCKS * PUCT_FUSED_TILE
    M, sims = trip + extra, 7
    p = pool(ea, S)
    b, d = p["boards"][1000:1000 + M].clone(), p["dice"][1000:1000 + M].clone()
    pb, pd, _ = planted(S)
    # a degenerate row and a one-cube row before and after a plain row, inside one tile: in the first trip and (extra 6) in the second
    for at in (64, trip) if extra == 6 else (64,):
        b[at], d[at] = pb[0], pd[0]
        b[at + 2], d[at + 2] = pb[5], pd[5]
        b[at + 3], d[at + 3] = pb[8], pd[8]
        b[at + 5], d[at + 5] = pb[7], pd[7]
    got = ea.puct_search(b, d, p["params"], sims)
    for i in range(0, M, 1024):
        sl = slice(i, min(M, i + 1024))
        same(got[sl], ea.puct_search(b[sl], d[sl], p["params"], sims), "rows %d .." % i)
    last = slice(trip - 40, M)                                 # the end of the first trip and the second, against the stages
    same(got[last], staged(ea, b[last], d[last], p["params"], sims, keep=False)[0], "the last rows against the stages")
    v = host_views(ea, got[last], S, sims)
    assert (v["done"][v["degenerate"] == 0] == sims).all() and (v["pending"] == -1).all()


# ---------------------------------------------------------------- 4. buffers

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, monkeypatch, S):
    p, M, sims = pool(ea, S), 70, 40
    b, d = rows(ea, S, M, sims)
    nb = ea._lib.load().ewn_puct_tree_bytes(S, 3, sims)
    want = staged(ea, b, d, p["params"], sims, keep=False)[0]
    eta = torch.ones((M, 6), device="cuda")
    alloc = GuardedAllocator()
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        tree = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree, tile %s" % tile)
        assert ea.puct_search(b, d, p["params"], sims, out=tree) is tree
        alloc.check("search")
        same(tree, want, "in a guarded buffer")
        noisy = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree with noise, tile %s" % tile)
        ea.puct_search(b, d, p["params"], sims, root_noise=eta, out=noisy)
        alloc.check("search with noise")


@pytest.mark.parametrize("S", [5, 7])
def test_what_the_buffer_held_does_not_matter(ea, monkeypatch, S):
    p, M, sims = pool(ea, S), 33, 7
    b, d = rows(ea, S, M, sims)
    nb = ea._lib.load().ewn_puct_tree_bytes(S, 3, sims)
    want = staged(ea, b, d, p["params"], sims, keep=False)[0]
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        for fill in (0x00, 0xFF, 0x7F):                        # zeros; a NaN in every float and -1 in every count; huge numbers
            tree = torch.full((M, nb), fill, dtype=torch.uint8, device="cuda")
            same(ea.puct_search(b, d, p["params"], sims, out=tree), want, "fill %#x" % fill)


@pytest.mark.parametrize("S", [5, 7])
def test_a_last_tile_of_one_tree(ea, monkeypatch, S):
    p, sims = pool(ea, S), 7
    b, d = rows(ea, S, 70, 40)
    for M, tile in ((65, "32"), (33, "32"), (65, "8"), (9, "4")):
        monkeypatch.setenv("EWN_PUCT_TILE", tile)
        same(ea.puct_search(b[:M], d[:M], p["params"], sims), staged(ea, b[:M], d[:M], p["params"], sims, keep=False)[0], (M, tile))


# ---------------------------------------------------------------- 5. a large budget

@pytest.mark.parametrize("S", [5, 7])
def test_a_budget_of_512(ea, S):
    p, M, sims = pool(ea, S), 3, 512
    b, d = p["boards"][40:40 + M], p["dice"][40:40 + M]
    want = staged(ea, b, d, p["params"], sims, keep=False)[0]
    same(ea.puct_search(b, d, p["params"], sims), want, "sims 512")
    v = host_views(ea, want, S, sims)
    assert int(v["count"].max()) > 100 and (v["done"] == sims).all()


# ---------------------------------------------------------------- 6. the users

@pytest.mark.parametrize("S", [5, 7])
def test_predict_puct_fused(ea, S):
    p = pool(ea, S)
    b, d = rows(ea, S, 70, 40)
    kw = dict(sims=16, c_puct=1.25, terminal_value=2.0, return_visits=True, return_q=True, return_value=True)
    want = ea.predict_puct(b, d, p["params"], **kw)
    for extra in ({}, {"chunk": 32}):
        got = ea.predict_puct(b, d, p["params"], fused=True, **extra, **kw)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(ea.predict_puct(b, d, p["params"], sims=16, c_puct=1.25, terminal_value=2.0, fused=True), want[0])
    assert int(want[1].sum()) > 0


def test_the_agent_and_the_spec(ea):
    from classical_policies import PuctAgent
    from ewn_gym_amd.tournament import evaluate
    p = pool(ea, 5)
    b, d = rows(ea, 5, 33, 7)
    fused, plain = PuctAgent(p["model"], sims=8, fused=True), PuctAgent(p["model"], sims=8)
    for x, y in zip(fused.predict_batch(b, d, return_visits=True), plain.predict_batch(b, d, return_visits=True)):
        assert torch.equal(x, y)
    r1 = evaluate({"kind": "mlp_puct", "model": p["model"], "sims": 4, "fused": True}, {"kind": "random"}, num=16)
    r0 = evaluate({"kind": "mlp_puct", "model": p["model"], "sims": 4}, {"kind": "random"}, num=16)
    assert (r1["wins"], r1["avg_length"]) == (r0["wins"], r0["avg_length"])


@pytest.mark.parametrize("S", [5, 7])
def test_selfplay_puct_fused(ea, S):
    p = pool(ea, S)
    b, d = p["boards"][:33], p["dice"][:33]
    kw = dict(sims=8, max_plies=12, temp_plies=4, key=11, game_offset=5)
    want = ea.selfplay_puct(b, d, p["params"], **kw)
    same_records(ea.selfplay_puct(b, d, p["params"], fused=True, **kw), want)
    same_records(ea.selfplay_puct(b, d, p["params"], fused=True, chunk=16, **kw), want)
    same_records(ea.selfplay_puct(b, d, p["params"], fused=True, noise_eps=0.0, **kw), ea.selfplay_puct(b, d, p["params"], noise_eps=0.0, **kw))
    assert int(want["live"].sum()) > 33


def test_the_trainers_take_the_fused_search(ea, tmp_path):
    from ewn_gym_amd.distill import SearchDistillTrainer
    from tests.test_gpu_distill_trainer import make_env
    from tests.test_gpu_puct_selfplay import selfplay_trainer
    tr, ref = selfplay_trainer(ea, fused=True), selfplay_trainer(ea)
    assert tr.fused is True and ref.fused is False
    tr.collect_and_update()
    ref.collect_and_update()
    same_records(tr.records, ref.records)
    assert torch.equal(bits(tr.grad), bits(ref.grad)) and torch.equal(bits(tr.params), bits(ref.params))
    path = str(tmp_path / "selfplay.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["fused_search"] is True and sd["fused"] is True and sd["sims"] == 6      # "fused": a fused trainer's checkpoint, as before
    other = selfplay_trainer(ea)
    other.load(path)
    assert other.fused is True
    ref.save(path)
    other.load(path)
    assert other.fused is False
    # the distiller: one update toward the fused search's targets is the update toward the staged search's
    a = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=5, fused=True)
    z = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=5)
    a.collect_and_update()
    z.collect_and_update()
    assert torch.equal(bits(a.grad), bits(z.grad)) and torch.equal(bits(a.params), bits(z.params))
    a.save(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["fused_search"] is True
    z.load(path)
    assert z.fused is True and (z.search, z.sims) == ("puct", 5)
    with pytest.raises(ValueError, match="fused=True"):
        SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, fused=True)               # the lookahead has no fused form
