"""The PUCT search at the budgets it ships with: 512 simulations in lock step with test_gpu_puct's numpy model, the
largest budget of 4 096 through the stages (node indices, per-dice visits and parent triples are int16; here they pass 4 000), a tree
buffer whose last trees start beyond 2^32 bytes, and guard zones around trees of 512 simulations.  No new tolerance: test_gpu_puct's
lock step, its P_TOL bound, its result and invariant checks, called as they are."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, i8  # noqa: E402
from tests.test_gpu_predict_policy import pool  # noqa: E402
from tests.test_gpu_puct import check_invariants, check_result, host_views, lockstep  # noqa: E402

MAX_SIMS = 4096


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def late_position(S):
    """four cubes, both sides a step from their corner; dice 3: flag 0 moves cube 1, whose diagonal wins, flag 1 cube 5.  After any
    other move the reply's cube 2 stands a diagonal step from ITS corner: simulations end on winning edges and add no node"""
    e = S - 1
    return boards_of(S, {(e - 1, e - 1): 1, (e - 2, e - 1): 5, (1, 1): -2, (1, 2): -6}), i8(3)


def live_rows(p, start, n):
    """the first n of the pool's observations from `start` on that are live: both sides hold a cube, neither stands on its corner"""
    b, d = p["boards"][start:start + 8 * n], p["dice"][start:start + 8 * n]
    live = (b > 0).any(2).any(1) & (b < 0).any(2).any(1) & (b[:, 0, 0] >= 0) & (b[:, -1, -1] <= 0)
    idx = torch.nonzero(live).reshape(-1)[:n]
    assert idx.numel() == n
    return b[idx].contiguous(), d[idx].contiguous()


def opening(ea, S, n=1):
    env = ea.VecEWN(n, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=n, philox_key=5)
    b, d = env.reset(seeds=(np.arange(n, dtype=np.uint64) + 21).astype(np.uint32))
    assert int((b[0] != 0).sum()) == 12
    return b.clone(), d.clone()


def staged(ea, b, d, params, sims, rounds=None):
    """begin, then `rounds` (sims + 1: the whole search) rounds of predict_policy and advance, without the model"""
    tree, lb, ld = ea.puct_begin(b, d, sims)
    for _ in range(sims + 1 if rounds is None else rounds):
        _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        ea.puct_advance(tree, logits, value, lb, ld, sims)
    return tree, lb, ld


# ---------------------------------------------------------------- 1. lock step at 512 simulations

@pytest.mark.parametrize("S", [5, 7])
def test_lock_step_at_512_simulations(ea, S):
    sims, p = 512, pool(ea, S)
    pb, pd = live_rows(p, 1000, 2)
    late_b, late_d = late_position(S)
    b, d = torch.cat([pb, late_b]).contiguous(), torch.cat([pd, late_d]).contiguous()
    tree, models, v = lockstep(ea, S, b, d, p["params"], sims)
    assert not any(m.degenerate for m in models)
    count, kind, n, child = v["count"], v["kind"], v["n"], v["child"]
    won = [int(n[m][kind[m] == 1].sum()) for m in range(3)]
    depth = []
    for m in range(3):
        dep = np.zeros(int(count[m]), np.int32)
        for j in range(1, int(count[m])):
            dep[j] = dep[v["parent"][m, j, 0]] + 1
        depth.append(int(dep.max()))
    print("S=%d sims=%d: node counts %s, largest child index %d, largest cn %d, visits that ended on a winning edge %s, depth %s" % (
        S, sims, count.tolist(), int(child.max()), int(v["cn"].max()), won, depth))
    assert int(count.max()) > 256 and int(child.max()) > 255                    # node indices past one byte
    assert any(int(count[m]) < sims + 1 and won[m] > 0 for m in range(3))        # a tree that does not fill
    check_result(ea, tree, models, S, sims)
    check_invariants(v, sims)


# ---------------------------------------------------------------- 2. the largest budget

@pytest.mark.parametrize("S", [5, 7])
def test_the_largest_budget_through_the_stages(ea, S):
    """4 097 rounds of the model beside the kernels do not fit a test's seconds (2.3 s a tree for the model alone, and every round
    copies the trees to the host), so the stages are driven alone and the finished trees checked by what holds of every tree"""
    from ewn_gym_amd.vec_env import _puct_sections
    sims, p, lib = MAX_SIMS, pool(ea, S), ea._lib.load()
    secs, nb = _puct_sections(S, sims)
    assert lib.ewn_puct_tree_bytes(S, 3, sims) == nb and nb > (sims + 1) * (256 if S == 5 else 280)
    ob, od = opening(ea, S)
    pb, pd = live_rows(p, 2000, 1)
    b, d = torch.cat([ob, pb]).contiguous(), torch.cat([od, pd]).contiguous()
    tree, lb, ld = staged(ea, b, d, p["params"], sims)
    assert tree.shape == (2, nb) and not lb.any() and bool((ld == 1).all())      # the search is over: no leaf is pending
    v = host_views(ea, tree, S, sims)
    assert v["board"].shape == (2, sims + 1, S, S) and secs["board"][0] + (sims + 1) * S * S <= nb
    check_invariants(v, sims)
    count, child, parent = v["count"], v["child"], v["parent"]
    print("S=%d sims=%d: node counts %s, largest child index %d, largest cn %d, largest root visit count %d" % (
        S, sims, count.tolist(), int(child.max()), int(v["cn"].max()), int(v["n"][:, 0].max())))
    assert int(count[0]) == sims + 1                                             # from the opening no simulation ends on a win
    where = np.argwhere(child[0] > 4000)
    assert len(where) > 0 and int(child[0].max()) == sims
    for j, a, dd in where:                                                       # ... and the int16 triples of those nodes point back
        ch = int(child[0, j, a, dd])
        assert tuple(int(x) for x in parent[0, ch]) == (j, a, dd + 1, 0) and int(v["dice"][0, ch]) == dd + 1
    assert sorted(int(x) for x in child[0][child[0] >= 0]) == list(range(1, sims + 1))
    want = ea.puct_result(tree, S, sims, return_visits=True, return_q=True, return_value=True)
    got = ea.predict_puct(b, d, p["params"], sims=sims, return_visits=True, return_q=True, return_value=True)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert int(want[1].sum()) == 2 * sims


@pytest.mark.parametrize("S", [5, 7])
def test_a_budget_of_4097_is_refused_before_any_launch(ea, S):
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib = pool(ea, S), ea._lib.load()
    b, d = p["boards"][:2], p["dice"][:2]
    assert lib.ewn_puct_tree_bytes(S, 3, MAX_SIMS + 1) < 0 and lib.ewn_puct_tree_bytes(S, 3, MAX_SIMS) > 0
    with pytest.raises(ValueError, match="sims must be an integer in 0..4096"):
        ea.puct_begin(b, d, MAX_SIMS + 1)
    with pytest.raises(ValueError, match="sims must be an integer in 0..4096"):
        ea.predict_puct(b, d, p["params"], sims=MAX_SIMS + 1)
    nb = lib.ewn_puct_tree_bytes(S, 3, MAX_SIMS)
    tree = torch.full((2, nb), 0x5A, dtype=torch.uint8, device="cuda")
    lb = torch.full((2, S, S), 0x5A, dtype=torch.int8, device="cuda")
    ld = torch.full((2,), 0x5A, dtype=torch.int8, device="cuda")
    lg, val = torch.zeros((2, 5), device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(ValueError, match="sims must be an integer in 0..4096"):
        ea.puct_advance(tree, lg, val, lb, ld, MAX_SIMS + 1)
    assert lib.ewn_puct_begin(S, 3, 2, MAX_SIMS + 1, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) != 0
    assert lib.ewn_puct_advance(S, 3, 2, MAX_SIMS + 1, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(lg), _ptr(val), _ptr(lb), _ptr(ld),
                                _stream()) != 0
    torch.cuda.synchronize()
    assert bool((tree == 0x5A).all()) and bool((lb == 0x5A).all()) and bool((ld == 0x5A).all())   # nothing was launched


# ---------------------------------------------------------------- 3. a tree buffer beyond 4 GiB

def test_trees_that_start_beyond_4_gib(ea):
    """pu_tree forms m * bytes in 64 bits: with 32 the last trees of this buffer would land on the first ones"""
    S, sims = 7, MAX_SIMS
    p, lib = pool(ea, S), ea._lib.load()
    nb = int(lib.ewn_puct_tree_bytes(S, 3, sims))
    M = 2 ** 32 // nb + 5
    assert (M - 4) * nb > 2 ** 32
    pb, pd = live_rows(p, 3000, 5)
    chosen_b, chosen_d, rep_b, rep_d = pb[:4].contiguous(), pd[:4].contiguous(), pb[4:].contiguous(), pd[4:].contiguous()
    assert bool(chosen_b[0].any()) and not torch.equal(chosen_b[0], rep_b[0])
    b = torch.cat([rep_b.expand(M - 4, S, S), chosen_b]).contiguous()
    d = torch.cat([rep_d.expand(M - 4), chosen_d]).contiguous()
    straddle = 2 ** 32 // nb                                                     # the tree that holds byte 2^32: the last repeated one
    assert straddle == M - 5 and straddle * nb < 2 ** 32 < (straddle + 1) * nb
    tree = None
    try:
        try:
            tree, lb, ld = ea.puct_begin(b, d, sims)
        except torch.cuda.OutOfMemoryError:
            pytest.skip("no room for a tree buffer of %d trees x %d bytes = %d bytes: the size is the test" % (M, nb, M * nb))
        assert tree.shape == (M, nb) and tree.numel() > 2 ** 32 + 4 * nb
        small = ea.puct_begin(chosen_b, chosen_d, sims)
        one = ea.puct_begin(rep_b, rep_d, sims)

        def same(where):
            for big, s4, s1, rows in ((tree, small[0], one[0], "trees"), (lb, small[1], one[1], "leaf boards"), (ld, small[2], one[2], "leaf dice")):
                assert torch.equal(big[M - 4:], s4), (where, rows, "the last four")
                for m in (0, 1, straddle - 1, straddle):
                    assert torch.equal(big[m], s1[0]), (where, rows, m)
        same("begin")
        for rnd in range(3):
            for t, x, y in ((tree, lb, ld), small, one):
                _, logits, value = ea.predict_policy(x, y, p["params"], return_logits=True, return_value=True)
                ea.puct_advance(t, logits, value, x, y, sims)
            same("round %d" % rnd)
        v = host_views(ea, tree[M - 4:], S, sims)
        print("M=%d trees x %d bytes = %.2f GiB, the last four start at byte %d and later; node counts %s" % (
            M, nb, M * nb / 2.0 ** 30, (M - 4) * nb, v["count"].tolist()))
        assert (v["count"] > 1).any() and (v["done"] == 3).all()
    finally:
        tree = None                                                              # 4.4 GB
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 4. guard zones at a large budget

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones_at_512_simulations(ea, S):
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib, M, sims, rounds = pool(ea, S), ea._lib.load(), 5, 512, 6
    b, d = p["boards"][4000:4000 + M].contiguous(), p["dice"][4000:4000 + M].contiguous()
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    alloc = GuardedAllocator()
    tree = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree")
    lb = alloc.zeros((M, S, S), dtype=torch.int8, tag="leaf_boards")
    ld = alloc.zeros((M,), dtype=torch.int8, tag="leaf_dice")
    assert lib.ewn_puct_begin(S, 3, M, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) == 0
    torch.cuda.synchronize()
    alloc.check("begin, sims=512")
    for rnd in range(rounds):
        _, logits, val = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
        assert lib.ewn_puct_advance(S, 3, M, sims, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(logits), _ptr(val), _ptr(lb), _ptr(ld),
                                    _stream()) == 0
        torch.cuda.synchronize()
        alloc.check("advance %d, sims=512" % rnd)
    want = staged(ea, b, d, p["params"], sims, rounds=rounds)
    for x, y in zip((tree, lb, ld), want):
        assert torch.equal(x, y)                                                 # all tree bytes
    v = host_views(ea, tree, S, sims)
    print("S=%d M=%d sims=%d, %d rounds inside guard zones: node counts %s" % (S, M, sims, rounds, v["count"].tolist()))
    assert int(v["count"].max()) > 1
