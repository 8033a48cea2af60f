"""The PUCT search on the trained actor-critic (ewn_puct_begin / _advance / _result, predict_puct) against a numpy model of
its definition: dict-of-arrays trees, every score and backup in np.float32, operation for operation.  There is no reference oracle (the
reference's MCTS hashes states and has no chance nodes): the definition's model is the yardstick.
1. Lock step: the test drives begin, predict_policy and advance itself and compares every section of every tree with the model after
every call, bit for bit (W by bit pattern).  The model's v is computed from the GPU's value with the definition's three fp32 operations.
The priors are the one tolerance: P of a newly expanded node lies within 32 * 2^-24 absolute of the float64 softmax product of the
same fp32 logits (fewer than 20 fp32 roundings and two expf of at most 2 ulp, each on values of at most 1: derived, not tuned); the
model then adopts the GPU's P bits, so that selection stays bit-comparable.  2. result and driver.  3. invariants of every final tree,
independent of the model.  4. constructed positions.  5. plumbing: guard zones, NULL outputs, the agent, the tournament, the trainer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_predict_lookahead import boards_of, cube_moves, cubes_of, find_cube, i8  # noqa: E402
from tests.test_gpu_predict_policy import bits, make_model, pool  # noqa: E402

F = np.float32
P_TOL = 32 * 2.0 ** -24
FIELDS = ("n", "child", "cn", "parent", "kind", "dice", "board")


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


# ---------------------------------------------------------------- the model of the definition

def flip(b):
    return np.ascontiguousarray(np.rot90(-b, 2))


def degenerate(board):
    return bool(board[0, 0] < 0 or board[-1, -1] > 0 or not (board > 0).any() or not (board < 0).any())


def edges(board, d):
    """(kind int8 [6], b1 per edge or None, both flags name one cube) of the node (board, d): the rules of 4k, from cube_moves"""
    mine = cubes_of(board, 1)
    c = (find_cube(mine, d, False), find_cube(mine, d, True))
    kind, b1 = np.zeros(6, np.int8), [None] * 6
    for f in (0, 1):
        if f == 1 and c[1] == c[0]:
            continue
        for r, nb in cube_moves(board, c[f], 1):
            if nb[-1, -1] > 0 or not (nb < 0).any():
                kind[3 * f + r] = 1
            else:
                kind[3 * f + r], b1[3 * f + r] = 2, nb
    return kind, b1, c[1] == c[0]


def prior64(logits, kind, one):
    l = logits.astype(np.float64)
    pf, pr = np.exp(l[:2] - l[:2].max()), np.exp(l[2:] - l[2:].max())
    pf, pr = pf / pf.sum(), pr / pr.sum()
    raw = np.zeros(6)
    for a in range(6):
        if kind[a]:
            raw[a] = pr[a % 3] if one else pf[a // 3] * pr[a % 3]
    return raw / raw.sum()


class Model:
    def __init__(self, board, dice, sims):
        N, S = sims + 1, board.shape[0]
        self.sims = sims
        self.t = dict(n=np.zeros((N, 6), np.int32), w=np.zeros((N, 6), F), p=np.zeros((N, 6), F), child=np.full((N, 6, 6), -1, np.int16),
                      cn=np.zeros((N, 6, 6), np.int16), parent=np.zeros((N, 4), np.int16), kind=np.zeros((N, 6), np.int8),
                      dice=np.zeros(N, np.int8), board=np.zeros((N, S, S), np.int8))
        self.t["board"][0], self.t["dice"][0], self.t["parent"][0, 0] = board, min(max(int(dice), 1), 6), -1
        self.count, self.done, self.degenerate = 1, 0, degenerate(board)
        self.pending = -1 if self.degenerate else 0

    def leaf(self):
        if self.pending < 0:
            return np.zeros_like(self.t["board"][0]), 1
        return self.t["board"][self.pending], int(self.t["dice"][self.pending])

    def backup(self, j, v):
        t = self.t
        while t["parent"][j, 0] >= 0:
            p, a, d = (int(x) for x in t["parent"][j, :3])
            t["w"][p, a] = F(t["w"][p, a] + F(-v))
            t["n"][p, a] += 1
            t["cn"][p, a, d - 1] += 1
            v, j = F(-v), p

    def advance(self, logits, V, c, inv_tv, gpu_p):
        """one ewn_puct_advance; returns (node, float64 prior) where a node was evaluated.  gpu_p [nodes, 6]: the GPU's priors, adopted"""
        if self.degenerate:
            return None
        t, out = self.t, None
        if self.pending >= 0:
            j = self.pending
            kind, _, one = edges(t["board"][j], int(t["dice"][j]))
            t["kind"][j], t["p"][j] = kind, gpu_p[j]
            out = (j, prior64(logits, kind, one))
            v = F(F(V) * inv_tv)
            v = v if v > F(-1) else F(-1)
            v = v if v < F(1) else F(1)
            self.backup(j, v)
            self.pending = -1
        if self.done < self.sims:
            self.done += 1
            self.simulate(c)
        return out

    def simulate(self, c):
        t, j = self.t, 0
        while True:
            kind, b1, _ = edges(t["board"][j], int(t["dice"][j]))
            n, w, p = t["n"][j], t["w"][j], t["p"][j]
            rs = np.sqrt(F(int(n.sum()) + 1))                  # correctly rounded
            best, sb = -1, F(0)
            for a in range(6):
                if kind[a] == 0:
                    continue
                q = F(w[a] / F(n[a])) if n[a] > 0 else F(0)
                s = F(q + F(F(F(c * p[a]) * rs) / F(1 + int(n[a]))))
                if best < 0 or s > sb:
                    best, sb = a, s
            a = best
            if kind[a] == 1:
                w[a] = F(w[a] + F(1))
                n[a] += 1
                self.backup(j, F(1))
                return
            d = int(np.argmin(t["cn"][j, a])) + 1              # the first minimum
            ch = int(t["child"][j, a, d - 1])
            if ch >= 0:
                j = ch
                continue
            idx = self.count
            self.count += 1
            t["child"][j, a, d - 1], t["board"][idx], t["dice"][idx], t["parent"][idx] = idx, flip(b1[a]), d, (j, a, d, 0)
            self.pending = idx
            return

    def result(self):
        """(action, visits int32 [6], q f32 [6], value f32)"""
        if self.degenerate:
            return (0, 0), np.zeros(6, np.int32), np.full(6, -np.inf, F), F(0)
        kind, n, w = self.t["kind"][0], self.t["n"][0], self.t["w"][0]
        q = np.array([-np.inf if kind[a] == 0 else 1.0 if kind[a] == 1 else (w[a] / F(n[a]) if n[a] > 0 else 0.0) for a in range(6)], F)
        tw = F(F(F(F(F(w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5])
        tn = int(n.sum())
        value = F(tw / F(tn)) if tn > 0 else F(0)
        wins, searched = [a for a in range(6) if kind[a] == 1], [a for a in range(6) if kind[a] == 2]
        best = 0
        if wins:
            best = wins[0]
        elif searched:
            best = searched[0]
            for a in searched[1:]:
                if n[a] > n[best]:
                    best = a
        return (best // 3, best % 3), n.copy(), q, value


def host_views(ea, tree, S, sims):
    return {k: v.numpy() for k, v in ea.puct_tree_views(tree.cpu(), S, sims).items()}


def compare(ea, tree, lb, ld, models, S, sims, where):
    v = host_views(ea, tree, S, sims)
    hlb, hld = lb.cpu().numpy(), ld.cpu().numpy()
    for name in ("count", "done", "pending", "degenerate"):
        want = np.array([int(getattr(m, name)) for m in models], np.int32)
        assert np.array_equal(v[name], want), (where, name, v[name], want)
    for name in FIELDS:
        want = np.stack([m.t[name] for m in models])
        assert np.array_equal(v[name], want), (where, name, np.argwhere(v[name] != want)[:4])
    for name in ("w", "p"):                                    # by bit pattern
        want = np.stack([m.t[name] for m in models])
        assert np.array_equal(v[name].view(np.int32), want.view(np.int32)), (where, name, np.argwhere(v[name] != want)[:4])
    for m, mod in enumerate(models):
        b, d = mod.leaf()
        assert np.array_equal(hlb[m], b) and int(hld[m]) == d, (where, "leaf row", m)
    return v


_RUNS = {}


def lockstep(ea, S, boards, dice, params, sims, c_puct=1.5, tv=1.0, key=None):
    """begin, then sims + 1 rounds of predict_policy and advance, the model beside them and compared after every call ->
    (tree, models, the final host views)"""
    if key is not None and key in _RUNS:
        return _RUNS[key]
    M = boards.shape[0]
    tree, lb, ld = ea.puct_begin(boards, dice, sims)
    assert tree.dtype == torch.uint8 and tree.shape == (M, ea._lib.load().ewn_puct_tree_bytes(S, 3, sims))
    assert lb.shape == (M, S, S) and ld.shape == (M,) and lb.dtype == ld.dtype == torch.int8
    hb, hd = boards.cpu().numpy(), dice.cpu().numpy()
    models = [Model(hb[m], hd[m], sims) for m in range(M)]
    v = compare(ea, tree, lb, ld, models, S, sims, "begin")
    c, inv_tv, pmax = F(c_puct), F(F(1) / F(tv)), 0.0
    for rnd in range(sims + 1):
        _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        out = ea.puct_advance(tree, logits, value, lb, ld, sims, c_puct=c_puct, terminal_value=tv)
        assert out[0] is tree and out[1] is lb and out[2] is ld
        gp = host_views(ea, tree, S, sims)["p"]
        hl, hv = logits.cpu().numpy(), value.cpu().numpy()
        for m, mod in enumerate(models):
            ev = mod.advance(hl[m], hv[m], c, inv_tv, gp[m])
            if ev is not None:
                err = float(np.abs(gp[m, ev[0]].astype(np.float64) - ev[1]).max())
                pmax = max(pmax, err)
                assert err <= P_TOL, (rnd, m, ev[0], gp[m, ev[0]], ev[1])
        v = compare(ea, tree, lb, ld, models, S, sims, "round %d" % rnd)
    print("S=%d M=%d sims=%d: max |P - P_float64| %.3g (bound %.3g)" % (S, M, sims, pmax, P_TOL))
    for mod in models:
        assert mod.pending == -1 and (mod.degenerate or mod.done == sims)
    if key is not None:
        _RUNS[key] = (tree, models, v)
    return tree, models, v


def pool_run(ea, S, M, sims):
    p = pool(ea, S)
    off = 100 * sims                                           # other observations per budget
    return lockstep(ea, S, p["boards"][off:off + M], p["dice"][off:off + M], p["params"], sims, key=(S, M, sims))


# ---------------------------------------------------------------- 1. lock step

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 33, 70])       # a lone wave, one wave past eight full blocks, several blocks
@pytest.mark.parametrize("sims", [1, 7, 40])
def test_lock_step(ea, S, M, sims):
    tree, models, v = pool_run(ea, S, M, sims)
    assert any(not m.degenerate for m in models)
    if sims == 40 and M == 70:
        assert int(v["count"].max()) > 8 and bool((v["parent"][:, 1:, 0] > 0).any())           # trees with depth


# ---------------------------------------------------------------- 2. result and driver

@pytest.mark.parametrize("S,M,sims", [(5, 70, 40), (7, 70, 40), (5, 33, 7), (7, 1, 1)])
def test_result_against_the_model(ea, S, M, sims):
    tree, models, _ = pool_run(ea, S, M, sims)
    check_result(ea, tree, models, S, sims)


def check_result(ea, tree, models, S, sims):
    """puct_result of lockstep's trees against the results of its models"""
    M = len(models)
    act, visits, q, value = ea.puct_result(tree, S, sims, return_visits=True, return_q=True, return_value=True)
    assert act.shape == (M, 2) and act.dtype == torch.int8 and visits.shape == (M, 2, 3) and visits.dtype == torch.int32
    assert q.shape == (M, 2, 3) and q.dtype == torch.float32 and value.shape == (M,) and value.dtype == torch.float32
    want = [m.result() for m in models]
    assert np.array_equal(act.cpu().numpy(), np.array([w[0] for w in want], np.int8))
    assert np.array_equal(visits.cpu().numpy().reshape(M, 6), np.stack([w[1] for w in want]))
    assert np.array_equal(q.cpu().numpy().reshape(M, 6).view(np.int32), np.stack([w[2] for w in want]).view(np.int32))
    assert np.array_equal(value.cpu().numpy().view(np.int32), np.array([w[3] for w in want], F).view(np.int32))
    assert float(q[torch.isfinite(q)].abs().max()) <= 1.0 and float(value.abs().max()) <= 1.0
    # NULL optional outputs: the same actions, alone and in every combination
    assert torch.equal(ea.puct_result(tree, S, sims), act)
    a2, q2 = ea.puct_result(tree, S, sims, return_q=True)
    assert torch.equal(a2, act) and torch.equal(bits(q2), bits(q))
    a3, v3, val3 = ea.puct_result(tree, S, sims, return_visits=True, return_value=True)
    assert torch.equal(a3, act) and torch.equal(v3, visits) and torch.equal(bits(val3), bits(value))


@pytest.mark.parametrize("S,M,sims", [(5, 70, 40), (7, 33, 7)])
def test_the_driver_is_the_stages(ea, S, M, sims):
    p = pool(ea, S)
    tree, _, _ = pool_run(ea, S, M, sims)
    off = 100 * sims
    b, d = p["boards"][off:off + M], p["dice"][off:off + M]
    kw = dict(sims=sims, return_visits=True, return_q=True, return_value=True)
    want = ea.puct_result(tree, S, sims, return_visits=True, return_q=True, return_value=True)
    got = ea.predict_puct(b, d, p["params"], **kw)
    again = ea.predict_puct(b, d, p["params"], **kw)
    chunked = ea.predict_puct(b, d, p["params"], chunk=32, **kw)
    for x, y, z, w in zip(got, again, chunked, want):
        assert x.dtype == w.dtype and x.shape == w.shape
        for other in (y, z, w):
            assert torch.equal(x.view(torch.uint8), other.view(torch.uint8))
    assert torch.equal(ea.predict_puct(b, d, p["params"], sims=sims), want[0])


@pytest.mark.parametrize("S", [5, 7])
def test_what_the_buffer_held_does_not_matter(ea, S):
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib, M, sims = pool(ea, S), ea._lib.load(), 33, 7
    b, d = p["boards"][:M], p["dice"][:M]
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    trees = []
    for fill in (0x00, 0xFF, 0x7F):                            # zeros; 0xFFFFFFFF, a NaN in every float and -1 in every count; 0x7F7F7F7F, huge
        tree = torch.full((M, nb), fill, dtype=torch.uint8, device="cuda")
        lb = torch.full((M, S, S), fill & 0x7F, dtype=torch.int8, device="cuda")
        ld = torch.full((M,), fill & 0x7F, dtype=torch.int8, device="cuda")
        assert lib.ewn_puct_begin(S, 3, M, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) == 0
        for _ in range(sims + 1):
            _, logits, value = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
            ea.puct_advance(tree, logits, value, lb, ld, sims)
        trees.append((tree, lb, ld))
    for t in trees[1:]:
        for x, y in zip(t, trees[0]):
            assert torch.equal(x, y)                           # all tree bytes
    assert int(ea.puct_tree_views(trees[0][0], S, sims)["count"].max()) > 1


# ---------------------------------------------------------------- 3. invariants

@pytest.mark.parametrize("S,M,sims", [(5, 70, 40), (7, 70, 40), (5, 33, 7), (7, 33, 7), (5, 1, 1), (7, 70, 1)])
def test_invariants(ea, S, M, sims):
    _, _, v = pool_run(ea, S, M, sims)
    check_invariants(v, sims)


def check_invariants(v, sims):
    """what holds of every finished tree, whatever the model says: v the host views (host_views) of trees after sims + 1 rounds"""
    M = v["count"].shape[0]
    live = v["degenerate"] == 0
    n, w, p, kind, cn, child, parent = (v[k] for k in ("n", "w", "p", "kind", "cn", "child", "parent"))
    assert np.array_equal(n[:, 0].sum(1)[live], np.full(int(live.sum()), sims))
    assert (v["count"] <= sims + 1).all() and (v["count"] >= 1).all() and (v["pending"] == -1).all()
    assert np.array_equal(v["done"][live], np.full(int(live.sum()), sims))
    k2 = kind == 2
    assert np.array_equal(n[k2], cn.sum(3, dtype=np.int32)[k2])
    assert (cn.max(3) - cn.min(3) <= 1).all()
    assert (np.abs(w) <= n).all()
    k0 = kind == 0
    assert not n[k0].any() and not w[k0].any() and not p[k0].any()
    assert np.array_equal(w[kind == 1], n[kind == 1].astype(F))                # a winning edge backs up +1 every time
    for m in range(M):
        cnt = int(v["count"][m])
        assert (child[m, cnt:] == -1).all() and not n[m, cnt:].any() and not kind[m, cnt:].any()
        seen = np.zeros(cnt, bool)
        for j in range(cnt):
            for a in range(6):
                for dd in range(6):
                    ch = int(child[m, j, a, dd])
                    if ch >= 0:
                        assert j < ch < cnt and not seen[ch] and kind[m, j, a] == 2
                        assert tuple(parent[m, ch]) == (j, a, dd + 1, 0)      # every child's parent triple points back at it
                        assert int(v["dice"][m, ch]) == dd + 1
                        seen[ch] = True
                    else:
                        assert ch == -1 and cn[m, j, a, dd] == 0
        assert tuple(parent[m, 0]) == (-1, 0, 0, 0) and seen[1:].all() and not seen[0]   # a true tree: one parent each
        if live[m]:
            expanded = kind[m, :cnt].any(1)
            assert expanded.all()                                                        # nothing is left pending
            s = p[m, :cnt].astype(np.float64).sum(1)
            assert (np.abs(s - 1.0) <= 8 * 2.0 ** -24).all(), s


# ---------------------------------------------------------------- 4. constructed positions

def biased_params(S, index, bias=-12.0):
    m = make_model(S, 5)
    with torch.no_grad():
        m.action_net.bias[index] = bias
    return m.flat_parameters()


@pytest.mark.parametrize("S", [5, 7])
def test_a_win_on_the_board_is_played_whatever_the_priors(ea, S):
    e = S - 1
    b = boards_of(S,
                  {(e - 1, e - 1): 1, (0, 0): 3, (1, e): -2},            # dice 2: flag 0 moves cube 1, whose diagonal reaches the corner
                  {(1, 1): 3, (0, 2): 5, (1, 2): -4},                    # dice 4: flag 0 moves cube 3, to the right it takes the last opposing cube
                  {(e - 1, e - 1): 6, (0, 1): 2, (2, 2): -1})            # dice 4: flag 1 moves cube 6 onto the corner
    d = i8(2, 4, 4)
    for index, rows in ((4, (0, 2)), (2, (1,))):                         # the direction the winning move takes gets a prior of about e^-12
        params = biased_params(S, index)
        _, logits = ea.predict_policy(b, d, params, return_logits=True)
        pr = torch.softmax(logits[:, 2:], 1)
        for sims in (0, 1, 7):
            act, visits, q, value = ea.predict_puct(b, d, params, sims=sims, return_visits=True, return_q=True, return_value=True)
            for row in rows:
                assert float(pr[row, index - 2]) < 1e-3
                f, r = ((0, 2), (0, 0), (1, 2))[row]
                assert act[row].tolist() == [f, r] and float(q[row, f, r]) == 1.0
                assert int(visits[row].sum()) == sims
    # ... and the search is the model's on these rows too
    lockstep(ea, S, b, d, biased_params(S, 4), 7)


@pytest.mark.parametrize("S", [5, 7])
def test_one_cube_one_direction(ea, S):
    e = S - 1
    p = pool(ea, S)
    b = boards_of(S, {(e, 1): 5, (0, e): -1, (1, e): -3},                # the only cube, on the last row: it can only go right
                  {(e, 1): 1, (e, 2): 2, (0, e): -6})                    # dice 1: cube 1 on the last row takes its own cube 2
    d = i8(3, 1)
    sims = 12
    tree, models, v = lockstep(ea, S, b, d, p["params"], sims)
    act, visits = ea.puct_result(tree, S, sims, return_visits=True)
    assert act.tolist() == [[0, 0], [0, 0]]
    assert visits.reshape(2, 6).tolist() == [[sims, 0, 0, 0, 0, 0]] * 2                  # all visits there
    assert v["kind"][:, 0].tolist() == [[2, 0, 0, 0, 0, 0]] * 2                          # one cube: edges 3..5 are no actions
    for m in range(2):                                                                   # both flags name one cube wherever one is left
        for j in range(int(v["count"][m])):
            if len(cubes_of(v["board"][m, j], 1)) == 1:
                assert not v["kind"][m, j, 3:].any() and (v["child"][m, j, 3:] == -1).all()
    # the mover took its own cube: no node under the root holds it any more (the opponent's side after the flip)
    assert int(v["count"][1]) > 1
    for j in range(1, int(v["count"][1])):
        held = {abs(int(x)) for x in v["board"][1, j].flat if x != 0}
        assert 2 not in held and 1 in held


@pytest.mark.parametrize("S", [5, 7])
def test_degenerate_rows_among_live_ones(ea, S):
    p = pool(ea, S)
    e = S - 1
    live = p["boards"][:4]
    dead = boards_of(S, {(e, e): 2, (0, 1): -1},          # already won
                     {(0, 0): -3, (2, 2): 1},             # already lost
                     {(2, 2): -4},                        # no agent cube
                     {(1, 1): 2},                         # no opposing cube
                     {})                                  # an empty board
    order = [0, 4, 1, 5, 6, 2, 7, 8, 3]
    b = torch.cat([live, dead])[order].contiguous()
    d = torch.cat([p["dice"][:4], i8(1, 2, 3, 4, 5)])[order].contiguous()
    is_dead = torch.tensor([i >= 4 for i in order], device="cuda")
    sims = 7
    tree, models, v = lockstep(ea, S, b, d, p["params"], sims)                           # zero-board leaf rows: compared in every round
    assert [m.degenerate for m in models] == is_dead.tolist() and v["degenerate"].tolist() == [int(x) for x in is_dead.tolist()]
    act, visits, q, value = ea.predict_puct(b, d, p["params"], sims=sims, return_visits=True, return_q=True, return_value=True)
    assert not act[is_dead].any() and not visits[is_dead].any() and not value[is_dead].any()
    assert bool((q[is_dead] == float("-inf")).all())
    alone = ea.predict_puct(live, p["dice"][:4], p["params"], sims=sims, return_visits=True, return_q=True, return_value=True)
    for x, y in zip((act, visits, q, value), alone):                                     # ... without disturbing their neighbours
        assert torch.equal(x[~is_dead].view(torch.uint8), y.view(torch.uint8))
    tree0, lb, ld = ea.puct_begin(b, d, sims)
    assert not lb[is_dead].any() and bool((ld[is_dead] == 1).all()) and bool(lb[~is_dead].any(1).any(1).all())


@pytest.mark.parametrize("S", [5, 7])
def test_dice_outside_the_range_clamp(ea, S):
    p = pool(ea, S)
    b = p["boards"][:20]
    kw = dict(sims=7, return_visits=True, return_q=True, return_value=True)
    for bad, good in ((0, 1), (7, 6), (-128, 1), (127, 6)):
        x = ea.predict_puct(b, torch.full((20,), bad, dtype=torch.int8, device="cuda"), p["params"], **kw)
        y = ea.predict_puct(b, torch.full((20,), good, dtype=torch.int8, device="cuda"), p["params"], **kw)
        for s, t in zip(x, y):
            assert torch.equal(s.view(torch.uint8), t.view(torch.uint8))
    tree, lb, ld = ea.puct_begin(b, i8(*([0, 7] * 10)), 7)
    assert ea.puct_tree_views(tree, S, 7)["dice"][:, 0].tolist() == [1, 6] * 10 and ld.tolist() == [1, 6] * 10
    lockstep(ea, S, b[:3], i8(0, 7, 9), p["params"], 3)


# ---------------------------------------------------------------- 5. plumbing

@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    from ewn_gym_amd.vec_env import _ptr, _stream
    p, lib, M, sims = pool(ea, S), ea._lib.load(), 33, 7
    b, d = p["boards"][200:200 + M].contiguous(), p["dice"][200:200 + M].contiguous()
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    alloc = GuardedAllocator()
    tree = alloc.zeros((M, nb), dtype=torch.uint8, tag="tree")
    lb = alloc.zeros((M, S, S), dtype=torch.int8, tag="leaf_boards")
    ld = alloc.zeros((M,), dtype=torch.int8, tag="leaf_dice")
    act = alloc.zeros((M, 2), dtype=torch.int8, tag="actions")
    visits = alloc.zeros((M, 2, 3), dtype=torch.int32, tag="visits")
    q = alloc.zeros((M, 2, 3), dtype=torch.float32, tag="q")
    value = alloc.zeros((M,), dtype=torch.float32, tag="value")
    act2 = alloc.zeros((M, 2), dtype=torch.int8, tag="actions alone")
    assert lib.ewn_puct_begin(S, 3, M, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()) == 0
    alloc.check("begin")
    for rnd in range(sims + 1):
        _, logits, val = ea.predict_policy(lb, ld, p["params"], return_logits=True, return_value=True)
        assert lib.ewn_puct_advance(S, 3, M, sims, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(logits), _ptr(val), _ptr(lb), _ptr(ld),
                                    _stream()) == 0
    alloc.check("advance")
    assert lib.ewn_puct_result(S, 3, M, _ptr(tree), _ptr(act), _ptr(visits), _ptr(q), _ptr(value), _stream()) == 0
    assert lib.ewn_puct_result(S, 3, M, _ptr(tree), _ptr(act2), None, None, None, _stream()) == 0      # NULL optional outputs
    alloc.check("result")
    want = ea.predict_puct(b, d, p["params"], sims=sims, return_visits=True, return_q=True, return_value=True)
    for x, y in zip((act, visits, q, value), want):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.equal(act2, act) and int(visits.sum()) == sims * M


def test_the_agent_over_one_episode(ea):
    from classical_policies import PuctAgent
    from envs import EinsteinWuerfeltNichtEnv
    p = pool(ea, 5)
    agent = PuctAgent(p["model"], board_size=5, sims=8)
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
    want = ea.predict_puct(b, d, p["params"], sims=8, return_visits=True)
    assert torch.equal(act, want[0]) and torch.equal(visits, want[1])
    assert torch.equal(agent.policy_fn()(b, d, 0), act)


def test_the_tournament_plays_it_and_repeats_itself(ea):
    from ewn_gym_amd import tournament
    p = pool(ea, 5)
    spec = {"kind": "mlp_puct", "model": p["model"], "sims": 4, "c_puct": 1.25, "terminal_value": 1.0}
    r = [tournament.evaluate(spec, {"kind": "random"}, num=16, board_size=5) for _ in range(2)]
    assert r[0]["episodes"] == 16 and 0 <= r[0]["wins"] <= 16
    assert r[0]["wins"] == r[1]["wins"] and torch.equal(r[0]["scores"], r[1]["scores"]) and torch.equal(r[0]["lengths"], r[1]["lengths"])


def test_one_puct_update_is_the_public_calls_composed(ea):
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.distill import SearchDistillTrainer, puct_targets
    from ewn_gym_amd.vec_env import _ptr, _stream
    from tests.test_gpu_distill_trainer import make_env
    N, K = 64, 3
    tr = SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=5, search="puct", sims=8)
    assert (tr.search, tr.sims, tr.c_puct) == ("puct", 8, 1.5)
    params = tr.params.clone()
    sq = torch.zeros_like(params)
    tr.collect_and_update()
    env = make_env(ea, N)                                                # by hand, on a second, identically seeded env
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, params, traj=traj, noise_key=tr.noise_key)
    assert torch.equal(traj["record"], tr.traj["record"])
    b = traj["obs_board"][:K].reshape(K * N, 5, 5).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    _, visits, q, value = ea.predict_puct(b, d, params, sims=8, c_puct=1.5, terminal_value=1.0, return_visits=True, return_q=True,
                                          return_value=True)
    # the target arithmetic, written out
    vis = visits.reshape(-1, 2, 3).float()
    tot = vis.sum((1, 2))
    w = (tot > 0).float()
    den = torch.where(tot > 0, tot, torch.ones_like(tot))[:, None]
    flag, direction = vis.sum(2) / den, vis.sum(1) / den
    one = (tot > 0) & (q[:, 1] == float("-inf")).all(1)
    flag = torch.where(one[:, None], torch.full_like(flag, 0.5), flag)
    tp = (torch.cat([flag, direction], 1) * w[:, None]).contiguous()
    tv = torch.where(tot > 0, 1.0 * value, torch.zeros_like(value))
    got = puct_targets(visits, q, value, 1.0)
    assert torch.equal(got[0], tp) and torch.equal(got[1], tv) and torch.equal(got[2], w)
    assert float(w.sum()) > 0 and bool(one.any()) and bool(((tp[:, :2].sum(1) - 1).abs() < 1e-6)[w > 0].all())
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    norm = torch.zeros(1, device="cuda")
    check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    assert torch.equal(bits(params), bits(tr.params)) and torch.equal(bits(sq), bits(tr.sq_avg))
    # the default is the lookahead trainer, untouched
    assert SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=5).search == "lookahead"


@pytest.mark.parametrize("S", [5, 7])
def test_a_puct_update_with_an_endgame_table(ea, S):
    """covered rows get the exact q's targets, as the lookahead trainer's rows get them; the others the search's.  On 7x7, with the
    (7, 2, 3) table, every second lane is put on a covered position: a rollout does not reach one within the test"""
    from ewn_gym_amd.distill import SearchDistillTrainer, puct_targets
    from tests.test_gpu_distill_trainer import make_env
    from tests.test_gpu_endgame import few_cube_lanes, table
    N, K = 256, 5
    t = table(ea, 5, 2, 4) if S == 5 else table(ea, 7, 2, 3)
    tr = SearchDistillTrainer(make_env(ea, N, S), n_steps=K, seed=5, search="puct", sims=6, c_puct=1.0, endgame_table=t, terminal_value=0.75)
    params = tr.params.clone()
    tr.env.rollout_policy(14, params, noise_key=1)     # past the openings: a rollout from the reset holds no position with few cubes
    if S == 7:
        few_cube_lanes(tr.env, 2, 3, 7)
    tr.collect_and_update()
    b, d = tr._boards, tr._dice
    _, visits, q, value = ea.predict_puct(b, d, params, sims=6, c_puct=1.0, terminal_value=0.75, return_visits=True, return_q=True,
                                          return_value=True)
    tp, tv, w = puct_targets(visits, q, value, 0.75)
    _, cov, qe = t.lookup(b, d, return_q=True)
    print("puct update %dx%d: %d of %d rows covered" % (S, S, int(cov.sum()), K * N))
    assert 0 < int(cov.sum()) < K * N
    if S == 7:
        assert int(cov[:N].sum()) >= N // 2                                # the lanes that were put on covered positions
    ep, ev, ew = ea.lookahead_targets(0.75 * qe, 0.0)
    tp, tv, w = torch.where(cov[:, None], ep, tp), torch.where(cov, ev, tv), torch.where(cov, ew, w)
    assert bool((w[cov] == 1).all()) and float(tv[cov].abs().max()) <= 0.75
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))


def test_the_checkpoint_records_the_search(ea, tmp_path):
    from ewn_gym_amd.distill import SearchDistillTrainer
    from tests.test_gpu_distill_trainer import make_env
    tr = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=4, search="puct", sims=5, c_puct=2.0)
    tr.collect_and_update()
    path = str(tmp_path / "puct.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["search"], sd["sims"], sd["c_puct"], sd["plies"]) == ("SEARCH", "puct", 5, 2.0, 1)
    other = SearchDistillTrainer(make_env(ea, 64), n_steps=3, seed=9)
    assert (other.search, other.sims, other.c_puct) == ("lookahead", 64, 1.5)
    other.load(path)
    assert (other.search, other.sims, other.c_puct) == ("puct", 5, 2.0) and torch.equal(bits(other.params), bits(tr.params))
    other.collect_and_update()                                           # ... and goes on with the loaded search
    assert bool(torch.isfinite(other.grad).all()) and other.stats_dict()["grad_norm"] > 0


def test_train_a2c_search_puct_end_to_end(ea, tmp_path):
    """one epoch of SEARCH --search puct with tiny numbers, in a fresh child process: the command line is what this test is about"""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SEARCH", "--search", "puct", "--sims", "4", "--c_puct", "1.25",
                        "--num_envs", "64", "--n_steps", "3", "--epoch_num", "1", "--timesteps_per_epoch", "384", "--eval_episode_num", "16",
                        "--eval_opponent", "random", "--save_dir", str(tmp_path)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 1 and ep[0]["timesteps"] == 384 and math.isfinite(ep[0]["policy_loss"])
    sd = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu", weights_only=True)
    assert (sd["algorithm"], sd["search"], sd["sims"], sd["c_puct"]) == ("SEARCH", "puct", 4, 1.25)
