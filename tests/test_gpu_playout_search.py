"""The playout-valued PUCT search in one launch (ewn_playout_search, playout_search, predict_playout_search) against
its definition driven through the public stage calls: puct_begin, then per round playout_wins on the leaf rows (tree m's row at
index obs_id0 + m, key + r * 0x9E3779B97F4A7C15), value = (2 w - n) / n as ONE correctly rounded fp32 division (numpy's, on the
host: torch divides a tensor by a scalar through a reciprocal) and puct_advance with zero logits.  The tree code and the playout
code are the same on both paths and playout x starts from seed(word, x) whichever lane plays it, so there is no tolerance anywhere
in this file: every comparison is of all bytes of all trees, and any difference is a bug.
A tree without a pending leaf gets no playouts and its value is not read; k_playout_wins_lean answers a finished or empty row with
all or nothing, so in the staged call a live position (the first observation) stands in such a tree's row.
1. lock step by rounds.  2. the grid.  3. prior contents.  4. chunks and shards.  5. guard zones.  6. the CPU oracle.
7. the stream contract (this entry is declared outside ewn_hip.h, so tests/test_gpu_stream_contract.py's table cannot name it:
its two cases live here).  8. the agent and the tournament.
Rows: fresh resets, midgames and few-cube endgames of seeded random play, and the two degenerate rows -- a finished position and a
board with one side empty."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_playout_search_cpu import KEY_STEP, MASK64, model_trees  # noqa: E402

SHAPES = [(5, 9, 6, 64), (5, 70, 17, 7), (7, 9, 6, 100), (7, 33, 12, 1)]     # (S, M, sims, playouts)
KEY, OBS0 = 2 ** 64 - 5 * KEY_STEP + 12345, 5                                # the key wraps within the rounds; a first id that is not 0


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_ROWS, _STAGED = {}, {}


def rows(ea, S, M):
    """M observations, computed once and left unchanged -> (boards int8 [M, S, S], dice int8 [M]): row 0 and 2 fresh resets, row 1 a
    finished position, row 3 a board with one side empty, then M // 3 rows with the fewest cubes of 24 steps of 256 random-agent
    games against the random opponent (endgames: many walks end on winning edges), the rest spread over that play"""
    if (S, M) not in _ROWS:
        N, K = 256, 24
        env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=77 + S)
        b0, d0 = env.reset(seeds=(np.arange(N, dtype=np.uint64) * 5 + 3).astype(np.uint32))
        b0, d0 = b0.clone(), d0.clone()
        traj = env.alloc_rollout(K)
        env.rollout(K, agent="random", traj=traj)
        tb, td = traj["board"].reshape(-1, S, S), traj["dice"].reshape(-1)
        order = torch.argsort((tb != 0).flatten(1).sum(1), stable=True)
        n_end = M // 3
        n_mid = M - 4 - n_end
        pick = torch.cat([order[:n_end], order[n_end + 17::max(1, (order.numel() - n_end - 17) // max(1, n_mid))][:n_mid]])
        b, d = torch.cat([b0[:4], tb[pick]]).contiguous(), torch.cat([d0[:4], td[pick]]).contiguous()
        b[1], b[3] = 0, 0
        b[1, S - 1, S - 1], b[1, 0, 1], d[1] = 2, -1, 4        # already won
        b[3, 1, 1], d[3] = 2, 3                                # no opposing cube
        assert b.shape == (M, S, S) and int(d.min()) >= 1 and int(d.max()) <= 6
        _ROWS[(S, M)] = (b, d)
    return _ROWS[(S, M)]


def gpu_wins(ea):
    return lambda batch, n, key: ea.playout_wins(batch, 1, n, key=key).cpu().numpy()


def oracle_wins(batch, n, key):
    from oracle import pyoracle
    return pyoracle.playout_wins(batch.cpu().numpy(), 1, n, key=key)


def staged(ea, b, d, sims, n, key=KEY, obs_id0=OBS0, c_puct=1.5, wins=None):
    """the yardstick: begin, then sims + 1 rounds of playouts on the leaf rows and advance -> the trees after begin and after every
    round (clones).  wins(batch, n, key) -> int32 [rows] on the host: the GPU's playout_wins, or the CPU oracle's"""
    wins = gpu_wins(ea) if wins is None else wins
    M, S = b.shape[0], b.shape[1]
    tree, lb, ld = ea.puct_begin(b, d, sims)
    zeros = torch.zeros((M, 5), dtype=torch.float32, device="cuda")
    spare = b[0]
    snaps = [tree.clone()]
    for r in range(sims + 1):
        pending = ea.puct_tree_views(tree, S, sims)["pending"] >= 0
        batch = torch.cat([spare[None].repeat(obs_id0, 1, 1), torch.where(pending[:, None, None], lb, spare[None])]).contiguous()
        w = wins(batch, n, (key + r * KEY_STEP) & MASK64)[obs_id0:].astype(np.int32)
        value = (2 * w - n).astype(np.float32) / np.float32(n)                 # one correctly rounded division
        ea.puct_advance(tree, zeros, torch.as_tensor(value).cuda(), lb, ld, sims, c_puct=c_puct, terminal_value=1.0)
        snaps.append(tree.clone())
    return snaps


def reference(ea, S, M, sims, n):
    """the staged trees of a shape at KEY and OBS0, computed once, shared and left unchanged"""
    if (S, M, sims, n) not in _STAGED:
        b, d = rows(ea, S, M)
        _STAGED[(S, M, sims, n)] = staged(ea, b, d, sims, n)
    return _STAGED[(S, M, sims, n)]


def same(got, want, where):
    assert got.dtype == want.dtype == torch.uint8 and got.shape == want.shape, where
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(1)).reshape(-1)
        m = int(bad[0])
        raise AssertionError("%s: %d of %d trees differ, the first is tree %d at bytes %s" % (
            where, int(bad.numel()), got.shape[0], m, torch.nonzero(got[m] != want[m]).reshape(-1)[:8].tolist()))


def views(ea, tree, S, sims):
    return {k: v.numpy() for k, v in ea.puct_tree_views(tree.cpu(), S, sims).items()}


# ---------------------------------------------------------------- 1. lock step by rounds

@pytest.mark.parametrize("S,M,sims,n", SHAPES)
def test_lock_step_by_rounds(ea, S, M, sims, n):
    """fails without the feature: the entry does not exist"""
    b, d = rows(ea, S, M)
    want = reference(ea, S, M, sims, n)
    assert len(want) == sims + 2
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0)
    for r in range(sims + 2):
        same(ea.playout_search(b, d, sims, rounds=r, **kw), want[r], "%d rounds" % r)
    same(ea.playout_search(b, d, sims, **kw), want[-1], "all rounds")
    same(ea.playout_search(b, d, sims, rounds=sims + 9, **kw), want[-1], "more rounds than there are")
    if M > 16:                                                 # more trees than one grid trip: 3 blocks of 4 trees
        for r in (0, 1, sims + 1):
            same(ea.playout_search(b, d, sims, rounds=r, blocks=3, **kw), want[r], "3 blocks, %d rounds" % r)
    v = views(ea, want[-1], S, sims)
    assert v["degenerate"].tolist()[:4] == [0, 1, 0, 1]
    live = v["degenerate"] == 0
    assert (v["done"][live] == sims).all() and (v["pending"] == -1).all() and (v["n"][live, 0].sum(1) == sims).all()
    print("S=%d M=%d sims=%d: nodes per live tree %s" % (S, M, sims, v["count"][live].tolist()))
    if M == 70:
        assert (v["count"][live] < sims + 1).any()             # walks that ended on winning edges: no node, no playouts
    other = ea.playout_search(b, d, sims, playouts=n, key=KEY + 1, obs_id0=OBS0)
    assert not torch.equal(other, want[-1])                    # the key reaches the playouts


@pytest.mark.parametrize("S", [5, 7])
def test_other_constants(ea, S):
    b, d = rows(ea, S, 9)
    for sims, n, c_puct, key, obs0 in ((5, 3, 0.0, 0, 0), (4, 65, 2.5, 7, 1000)):
        want = staged(ea, b, d, sims, n, key=key, obs_id0=obs0, c_puct=c_puct)[-1]
        same(ea.playout_search(b, d, sims, playouts=n, c_puct=c_puct, key=key, obs_id0=obs0), want, (sims, n, c_puct))


# ---------------------------------------------------------------- 2. the grid

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[1], SHAPES[3]])
def test_one_block_equals_the_default_grid(ea, S, M, sims, n):
    """70 trees on one block are 18 trips with two idle waves in the last, 33 are 9 trips with three"""
    b, d = rows(ea, S, M)
    want = reference(ea, S, M, sims, n)[-1]
    for blocks in (1, 2, 4096):
        same(ea.playout_search(b, d, sims, playouts=n, key=KEY, obs_id0=OBS0, blocks=blocks), want, "%d blocks" % blocks)


# ---------------------------------------------------------------- 3. prior contents

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[1], SHAPES[2]])
def test_what_the_buffer_held_does_not_matter(ea, S, M, sims, n):
    b, d = rows(ea, S, M)
    want = reference(ea, S, M, sims, n)[-1]
    for fill in (0xFF, 0x7F):                                  # a NaN in every float and -1 in every count; huge numbers
        tree = torch.full(tuple(want.shape), fill, dtype=torch.uint8, device="cuda")
        assert ea.playout_search(b, d, sims, playouts=n, key=KEY, obs_id0=OBS0, out=tree) is tree
        same(tree, want, "fill %#x" % fill)


# ---------------------------------------------------------------- 4. chunks and shards

@pytest.mark.parametrize("S", [5, 7])
def test_chunks_and_shards(ea, S):
    b, d = rows(ea, S, 70)
    kw = dict(sims=9, playouts=20, key=KEY, return_visits=True, return_q=True, return_value=True)
    whole = ea.predict_playout_search(b, d, obs_id0=0, chunk=1024, **kw)
    for x, y in zip(ea.predict_playout_search(b, d, obs_id0=0, chunk=32, **kw), whole):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for x, y in zip(ea.predict_playout_search(b[20:], d[20:], obs_id0=20, **kw), whole):
        assert torch.equal(x.view(torch.uint8), y[20:].contiguous().view(torch.uint8))
    assert torch.equal(ea.predict_playout_search(b, d, sims=9, playouts=20, key=KEY), whole[0])
    tree = ea.playout_search(b, d, 9, playouts=20, key=KEY)
    for x, y in zip(ea.puct_result(tree, S, 9, return_visits=True, return_q=True, return_value=True), whole):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert int(whole[1].sum()) == 9 * int((whole[1].flatten(1).sum(1) > 0).sum()) > 0


# ---------------------------------------------------------------- 5. guard zones

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[1], SHAPES[3]])
def test_guard_zones(ea, S, M, sims, n):
    b, d = rows(ea, S, M)
    want = reference(ea, S, M, sims, n)[-1]
    nb = want.shape[1]
    alloc = GuardedAllocator()
    gb = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards")
    gd = alloc.zeros((M,), dtype=torch.int8, tag="dice")
    gb.copy_(b)
    gd.copy_(d)
    for blocks in (None, 1):
        tree = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree, blocks %s" % blocks, offset=4)   # 4 bytes past a 16-byte boundary
        assert tree.data_ptr() % 16 == 4
        ea.playout_search(gb, gd, sims, playouts=n, key=KEY, obs_id0=OBS0, blocks=blocks, out=tree)
        alloc.check("search, blocks %s" % blocks)
        same(tree, want, "in a guarded buffer")


# ---------------------------------------------------------------- 6. the CPU oracle, independently of the GPU's playout_wins

@pytest.mark.parametrize("S,M,sims,n", [SHAPES[0], SHAPES[3]])
def test_against_the_cpu_oracle(ea, S, M, sims, n):
    """With sims = 0 the one round evaluates the root, and pu_backup has nowhere to put a root's value: key_0's playouts of a root
    leave no trace in a tree, so that search is compared with the stages as a whole, and the playouts are tied to the CPU oracle
    where they first show: with sims = 1 the root edge the one simulation took holds N = 1 and W = -(2 w - n) / n, w =
    pyoracle.playout_wins of node 1's board at key_1 and row index obs_id0 + m.  Then every round: the stages with the oracle's wins
    in place of the GPU's give the kernel's bytes, and so does the numpy tree model on the oracle's wins, field by field."""
    from oracle import pyoracle
    b, d = rows(ea, S, M)
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0)
    same(ea.playout_search(b, d, 0, **kw), staged(ea, b, d, 0, n, wins=oracle_wins)[-1], "sims 0")
    v = views(ea, ea.playout_search(b, d, 1, **kw), S, 1)
    grown = np.nonzero(v["count"] == 2)[0]
    assert grown.size >= 2
    batch = np.stack([b[0].cpu().numpy()] * (OBS0 + M))
    batch[OBS0 + grown] = v["board"][grown, 1]
    w = pyoracle.playout_wins(batch, 1, n, key=(KEY + KEY_STEP) & MASK64)[OBS0:]
    value = (2 * w - n).astype(np.float32) / np.float32(n)
    for m in grown:
        a = int(v["parent"][m, 1, 1])
        assert v["n"][m, 0, a] == 1 and v["n"][m, 0].sum() == 1
        assert v["w"][m, 0, a].view(np.int32) == np.float32(-value[m]).view(np.int32), (m, v["w"][m, 0, a], value[m])
    got = ea.playout_search(b, d, sims, **kw)
    same(got, staged(ea, b, d, sims, n, wins=oracle_wins)[-1], "the stages on the oracle's wins")
    models = model_trees(b.cpu().numpy(), d.cpu().numpy(), sims, n, KEY, OBS0)
    v = views(ea, got, S, sims)
    for name in ("count", "done", "pending", "degenerate"):
        assert np.array_equal(v[name], np.array([int(getattr(mod, name)) for mod in models], np.int32)), name
    for name in ("n", "child", "cn", "parent", "kind", "dice", "board"):
        assert np.array_equal(v[name], np.stack([mod.t[name] for mod in models])), name
    for name in ("w", "p"):
        assert np.array_equal(v[name].view(np.int32), np.stack([mod.t[name] for mod in models]).view(np.int32)), name


# ---------------------------------------------------------------- 7. the stream contract

def sleep_cycles():
    """about 20 ms of torch.cuda._sleep, from one timed sleep"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(1000000)
    e1.record()
    torch.cuda.synchronize()
    return int(20.0 / max(e0.elapsed_time(e1), 1e-3) * 1000000)


@pytest.mark.parametrize("S,M,sims,n", [SHAPES[0], SHAPES[3]])
def test_a_side_stream_is_honoured(ea, S, M, sims, n):
    """on a side stream behind a sleep: the copy of B into the inputs, the fill of the tree, the call, the copy of the tree.  Only
    that stream is synchronised.  A launch on any other stream reads A behind the sleep's back and is overwritten by the fill."""
    bB, dB = rows(ea, S, M)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0)
    EA, EB = ea.playout_search(bA, dA, sims, **kw), reference(ea, S, M, sims, n)[-1]
    assert not torch.equal(EA, EB)
    b, d, tree = bA.clone(), dA.clone(), torch.full_like(EB, 0x3C)
    cycles = sleep_cycles()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        b.copy_(bB)
        d.copy_(dB)
        tree.fill_(0xA5)
        ea.playout_search(b, d, sims, out=tree, **kw)
        got = tree.clone()
    s.synchronize()
    same(got, EB, "on a side stream")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,M,sims,n", [SHAPES[0], SHAPES[3]])
def test_a_captured_graph_replays_like_eager_calls(ea, S, M, sims, n):
    """captured once, replayed three times -- on A, on B, on A again, the tree refilled between -- against three eager calls"""
    bB, dB = rows(ea, S, M)
    bA, dA = bB.flip(0).contiguous(), dB.flip(0).contiguous()
    kw = dict(playouts=n, key=KEY, obs_id0=OBS0)
    EB = reference(ea, S, M, sims, n)[-1]
    eager = [ea.playout_search(bA, dA, sims, **kw), ea.playout_search(bB, dB, sims, **kw), ea.playout_search(bA, dA, sims, **kw)]
    same(eager[1], EB, "the eager call")
    assert torch.equal(eager[0], eager[2]) and not torch.equal(eager[0], eager[1])
    b, d, tree = bA.clone(), dA.clone(), torch.full_like(EB, 0x5A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        ea.playout_search(b, d, sims, out=tree, **kw)
    torch.cuda.synchronize()
    assert bool((tree == 0x5A).all()), "the captured call ran during the capture"
    for k, (xb, xd) in enumerate(((bA, dA), (bB, dB), (bA, dA))):
        b.copy_(xb)
        d.copy_(xd)
        tree.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        same(tree, eager[k], "replay %d" % (k + 1))


# ---------------------------------------------------------------- 8. the agent and the tournament

def test_the_agent_and_the_tournament(ea):
    from classical_policies import PlayoutSearchAgent
    from ewn_gym_amd.tournament import evaluate
    b, d = rows(ea, 5, 33)
    agent = PlayoutSearchAgent(3, 5, sims=8, playouts=16, c_puct=1.25, seed=1)
    want = ea.predict_playout_search(b, d, sims=8, playouts=16, c_puct=1.25, key=99, obs_id0=7, return_visits=True, return_value=True)
    for x, y in zip(agent.predict_batch(b, d, key=99, obs_id0=7, return_visits=True, return_value=True), want):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(agent.predict_batch(b.cpu().numpy(), d.cpu().numpy(), key=99, obs_id0=7), want[0])
    act, _ = agent.predict({"board": b[0].cpu().numpy(), "dice_roll": int(d[0])})
    assert act.shape == (2,) and act.dtype == np.int8
    spec = {"kind": "playout_search", "sims": 8, "playouts": 16}
    r0, r1 = evaluate(spec, {"kind": "random"}, num=16), evaluate(spec, {"kind": "random"}, num=16)
    assert (r0["wins"], r0["avg_length"], r0["engine"]) == (r1["wins"], r1["avg_length"], "ewn_step")
    assert torch.equal(r0["scores"], r1["scores"]) and torch.equal(r0["lengths"], r1["lengths"]) and r0["episodes"] == 16
