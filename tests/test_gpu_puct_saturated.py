"""PUCT priors and leaf values on saturated network outputs, on the device (pu_evaluate, csrc/ewn_puct.hpp).  The
positions, logit vectors and values are tests/test_puct_saturated_cpu.py's, which shows on the host that they have teeth; here they
go through every kernel that evaluates a node.
1. Staged, in lock step with tests/test_gpu_puct.py's Model: the logits and the value of a tree are constants handed to
puct_advance directly, no network is called; one batch per magnitude g (its 27 vectors of groups A, B and C on the 13 positions,
351 trees, a value of the list each) and one for groups D and E, so that a case stays at a few hundred trees.  Every evaluated
node's P is finite, exactly 0 on the edges that are no actions and within P_TOL of prior64 on the same logits (the root's mixed P under root noise: within NOISE_TOL of the mix); the Model adopts the
bits and every section of every tree is compared after every round, W and P by bit pattern.  2. An offset of 8192 on all five
logits changes no byte.  3. The value clamp binds on both sides.  4. Networks with constant outputs (zero head weights, the vector
and the value as biases) carry the vectors on which the former arithmetic fails, and the controls, into the kernels that hold the
network: puct_search, predict_puct, puct_search_wide, selfplay_puct, each against the staged trees of the same vector, byte for
byte, or against WideModel.  5. lookahead_targets, whose maximum is taken over the set it normalises over, at small temperatures."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_predict_lookahead import boards_of, i8  # noqa: E402
from tests.test_gpu_predict_policy import pool  # noqa: E402
from tests.test_gpu_puct import F, P_TOL, Model, compare, degenerate, edges, host_views  # noqa: E402
from tests.test_gpu_puct_fused import planted, same  # noqa: E402
from tests.test_gpu_puct_selfplay import NOISE_TOL, NoiseModel, by_hand, noise_rows, same_records  # noqa: E402
from tests.test_gpu_puct_wide import against_the_model  # noqa: E402
from tests.test_gpu_sup_grad import targets_model  # noqa: E402
from tests.test_puct_saturated_cpu import GS, SIMS, TERMINAL_VALUES, VALUES, VECTORS, failing_pairs, position_specs, positions  # noqa: E402

NET_VALUES = (0.25, -0.5, 1.5, -64.0)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_POS = {}


def all_positions(ea, S):
    """(boards [13, S, S], dice [13]) on the device: the five constructed positions, then eight rows of ordinary play"""
    if S not in _POS:
        sp = position_specs(S)
        b = boards_of(S, *[cells for _, cells, _, _ in sp])
        d = i8(*[dice for _, _, dice, _ in sp])
        hb, hd = positions(S)
        assert np.array_equal(b.cpu().numpy(), hb) and np.array_equal(d.cpu().numpy(), hd)
        pb, pd, _ = planted(S)
        assert torch.equal(b[0], pb[5]) and int(d[0]) == int(pd[5])                        # the only cube on the last row
        p = pool(ea, S)
        qb, qd = p["boards"][:64].cpu().numpy(), p["dice"][:64].cpu().numpy()
        play = [m for m in range(64) if not degenerate(qb[m]) and edges(qb[m], int(qd[m]))[0].any()][:8]
        assert len(play) == 8
        idx = torch.as_tensor(play).cuda()
        _POS[S] = (torch.cat([b, p["boards"][idx]]).contiguous(), torch.cat([d, p["dice"][idx]]).contiguous())
    return _POS[S]


def batch(b, d, ks, shift=0):
    """every position under every vector of ks, a value of the list per tree -> (boards, dice, logits [M, 5], value [M], the
    vector of every tree)"""
    P = b.shape[0]
    which = [k for k in ks for _ in range(P)]
    lg = torch.as_tensor(np.stack([VECTORS[k][2] for k in which])).cuda()
    val = torch.as_tensor(np.array([VALUES[(t + shift) % len(VALUES)] for t in range(len(which))], F)).cuda()
    return b.repeat(len(ks), 1, 1).contiguous(), d.repeat(len(ks)).contiguous(), lg, val, which


def advance_all(ea, b, d, lg, val, sims=SIMS, c_puct=1.5, tv=1.0, noise=None, eps=0.25):
    """begin, then sims + 1 rounds of puct_advance on constant outputs -> the trees"""
    tree, lb, ld = ea.puct_begin(b, d, sims)
    for rnd in range(sims + 1):
        ea.puct_advance(tree, lg, val, lb, ld, sims, c_puct=c_puct, terminal_value=tv, root_noise=noise if rnd == 0 else None, noise_eps=eps)
    return tree


class ClampModel(Model):
    """Model that keeps (V * inv_tv before the clamp, the v it backed up) of every evaluation"""

    def __init__(self, board, dice, sims):
        super().__init__(board, dice, sims)
        self.evaluated, self.x = [], None

    def advance(self, logits, V, c, inv_tv, gpu_p):
        self.x = F(F(V) * inv_tv) if self.pending >= 0 and not self.degenerate else None
        return super().advance(logits, V, c, inv_tv, gpu_p)

    def backup(self, j, v):
        if self.x is not None:                                 # advance backs the evaluation up before it simulates
            self.evaluated.append((self.x, v))
            self.x = None
        super().backup(j, v)


def lockstep_constants(ea, S, b, d, lg, val, which, sims=SIMS, c_puct=1.5, tv=1.0, eta=None, eps=0.25, model=Model, where=""):
    """tests/test_gpu_puct.py's lock step on injected outputs.  Every node evaluated in a round is checked and every tree compared
    after every round; the figures are printed before anything about P is asserted -> (tree, models)"""
    M = b.shape[0]
    hb, hd, hl, hv = b.cpu().numpy(), d.cpu().numpy(), lg.cpu().numpy(), val.cpu().numpy()
    noise = None if eta is None else torch.as_tensor(eta).cuda()
    models = [model(hb[m], hd[m], sims) if eta is None else NoiseModel(hb[m], hd[m], sims, eta[m], eps) for m in range(M)]
    tree, lb, ld = ea.puct_begin(b, d, sims)
    compare(ea, tree, lb, ld, models, S, sims, "begin")
    c, inv_tv = F(c_puct), F(F(1) / F(tv))
    worst, nans, nodes, bad = {}, {}, 0, []
    for rnd in range(sims + 1):
        ea.puct_advance(tree, lg, val, lb, ld, sims, c_puct=c_puct, terminal_value=tv, root_noise=noise if rnd == 0 else None, noise_eps=eps)
        gp = host_views(ea, tree, S, sims)["p"]
        for m, mod in enumerate(models):
            with np.errstate(all="ignore"):
                ev = mod.advance(hl[m], hv[m], c, inv_tv, gp[m])
            if ev is None:
                continue
            j, p64 = ev
            got, kind, grp = gp[m, j], mod.t["kind"][j], VECTORS[which[m]][0]
            nodes += 1
            tol = NOISE_TOL if eta is not None and j == 0 else P_TOL
            if not np.isfinite(got).all():
                nans[grp] = nans.get(grp, 0) + 1
                bad.append((rnd, m, j, grp, got.tolist()))
                continue
            err = float(np.abs(got.astype(np.float64) - p64).max())
            worst[grp] = max(worst.get(grp, 0.0), err)
            if err > tol or (got[kind == 0] != 0).any():
                bad.append((rnd, m, j, grp, got.tolist(), p64.tolist()))
        compare(ea, tree, lb, ld, models, S, sims, "%s round %d" % (where, rnd))
    for grp in sorted(set(worst) | set(nans)):
        print("%s S=%d group %s: max |P - P_float64| %.3g over the finite ones (bound %.3g), %d nodes with a P that is not finite" % (
            where, S, grp, worst.get(grp, 0.0), P_TOL, nans.get(grp, 0)))
    assert nodes >= M and not bad, (where, len(bad), bad[:3])
    for mod in models:
        assert mod.pending == -1 and mod.done == sims and not mod.degenerate
    return tree, models


# ---------------------------------------------------------------- 1. staged, one batch per magnitude

CASES = list(GS) + ["DE"]


def case_vectors(case):
    if case == "DE":
        return [k for k, v in enumerate(VECTORS) if v[0] in "DE"]
    return [k for k, v in enumerate(VECTORS) if v[0] in "ABC" and v[1] == case]


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("noise", [False, True])
def test_staged_lock_step_on_injected_outputs(ea, S, case, noise):
    b, d = all_positions(ea, S)
    ks = case_vectors(case)
    assert len(ks) == (14 if case == "DE" else 27)
    bb, dd, lg, val, which = batch(b, d, ks, shift=CASES.index(case))
    eta = noise_rows(bb.cpu().numpy(), dd.cpu().numpy(), 100 * S + CASES.index(case)) if noise else None
    tree, models = lockstep_constants(ea, S, bb, dd, lg, val, which, eta=eta, where="g %s%s" % (case, ", root noise" if noise else ""))
    v = host_views(ea, tree, S, SIMS)
    assert np.array_equal(v["n"][:, 0].sum(1), np.full(len(models), SIMS)) and np.isfinite(v["w"]).all() and np.isfinite(v["p"]).all()
    assert int(v["count"].max()) > 6                                                     # trees with nodes below the root's children


# ---------------------------------------------------------------- 2. shift invariance

@pytest.mark.parametrize("S", [5, 7])
def test_a_common_offset_changes_no_byte(ea, S):
    b, d = all_positions(ea, S)
    shifted = [k for k, v in enumerate(VECTORS) if v[0] == "D"]
    plain = []
    for k in shifted:                                                                    # the same vector without the offset
        (twin,) = [j for j, v in enumerate(VECTORS) if v[0] == "B" and np.array_equal(v[2], VECTORS[k][2] - VECTORS[k][2].max())]
        plain.append(twin)
    assert len(shifted) == 12 and sorted({VECTORS[k][1] for k in plain}) == [24, 104]
    eta = torch.as_tensor(noise_rows(b.repeat(12, 1, 1).cpu().numpy(), d.repeat(12).cpu().numpy(), 7 * S)).cuda()
    for noise in (None, eta):
        bb, dd, lg, val, _ = batch(b, d, plain)
        want = advance_all(ea, bb, dd, lg, val, noise=noise)
        bb, dd, lg, val, _ = batch(b, d, shifted)
        assert float(lg.max()) == 8192 and float(lg.min()) == 8192 - 104
        same(advance_all(ea, bb, dd, lg, val, noise=noise), want, "logits + 8192%s" % ("" if noise is None else ", root noise"))
    assert int(host_views(ea, want, S, SIMS)["count"].max()) > 6


# ---------------------------------------------------------------- 3. the value clamp

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("tv", TERMINAL_VALUES)
def test_the_value_clamp_binds_on_both_sides(ea, S, tv):
    b, d = all_positions(ea, S)
    (k,) = [k for k, v in enumerate(VECTORS) if v[0] == "E"][:1]
    P, nv = b.shape[0], len(VALUES)
    bb, dd = b.repeat_interleave(nv, 0).contiguous(), d.repeat_interleave(nv).contiguous()       # every value on every position
    val = torch.as_tensor(np.array(VALUES * P, F)).cuda()
    lg = torch.as_tensor(np.tile(VECTORS[k][2], (P * nv, 1))).cuda()
    tree, models = lockstep_constants(ea, S, bb, dd, lg, val, [k] * (P * nv), tv=tv, model=ClampModel, where="tv %g" % tv)
    seen = np.array([xv for mod in models for xv in mod.evaluated], F)              # (V / tv before the clamp, what was backed up)
    x, v = seen[:, 0], seen[:, 1]
    above, below, inside = x > 1, x < -1, np.abs(x) <= 1
    print("tv %g: %d evaluations, %d clamped to 1, %d clamped to -1, %d inside" % (tv, len(x), above.sum(), below.sum(), inside.sum()))
    assert len(x) >= 13 * len(models) // 2 and not np.isnan(x).any()
    assert above.sum() > len(models) and (v[above] == 1).all() and below.sum() > len(models) and (v[below] == -1).all()
    assert inside.sum() > len(models) and np.array_equal(v[inside].view(np.int32), x[inside].view(np.int32))
    assert np.isinf(x).any() and (np.abs(x) > 1e36).any() and ((x != 0) & (np.abs(x) < 1e-37)).any()        # 3e38 / 0.75 is inf as well
    w = host_views(ea, tree, S, SIMS)["w"]
    assert np.isfinite(w).all() and float(np.abs(w).max()) <= SIMS


# ---------------------------------------------------------------- 4. networks with constant outputs

_NET, _CASES = {}, {}


def constant_params(S, logits, value):
    """the flat parameters of an ActorCritic whose heads have zero weights: its logits and value are the biases on every row"""
    from ewn_gym_amd.a2c import ActorCritic
    if S not in _NET:
        torch.manual_seed(3)
        m = ActorCritic(S, 6).cuda()
        with torch.no_grad():
            m.action_net.weight.zero_()
            m.value_net.weight.zero_()
        _NET[S] = m
    m = _NET[S]
    with torch.no_grad():
        m.action_net.bias.copy_(torch.as_tensor(logits))
        m.value_net.bias.fill_(float(value))
    return m.flat_parameters()


def network_cases(ea, S):
    """[(vector, boards, dice, params, logits [M, 5], value [M])]: per vector the constructed positions on which the former
    arithmetic fails (tests/test_puct_saturated_cpu.py::failing_pairs), all of them under the controls"""
    if S in _CASES:
        return _CASES[S]
    b, d = all_positions(ea, S)
    rows = {}
    for i, k in failing_pairs(S):
        rows.setdefault(k, []).append(i)
    for k, idx in rows.items():
        if len(idx) == 1:                                      # two rows at the least: a healthy position beside the failing one
            idx.append((idx[0] + 1) % 5)
    for k, v in enumerate(VECTORS):
        if v[0] == "E":
            rows[k] = list(range(5))
    out = []
    for n, (k, idx) in enumerate(sorted(rows.items())):
        value = NET_VALUES[n % len(NET_VALUES)]
        ix = torch.as_tensor(idx).cuda()
        bb, dd = b[ix].contiguous(), d[ix].contiguous()
        params = constant_params(S, VECTORS[k][2], value)
        lg = torch.as_tensor(np.tile(VECTORS[k][2], (len(idx), 1))).cuda()
        val = torch.full((len(idx),), value, dtype=torch.float32, device="cuda")
        _, gl, gv = ea.predict_policy(bb, dd, params, return_logits=True, return_value=True)
        assert torch.equal(gl, lg) and torch.equal(gv, val), (k, gl, gv)                  # exactly those numbers, on every row
        out.append((k, bb, dd, params, lg, val))
    assert len(out) > 40 and {VECTORS[c[0]][0] for c in out} == set("ABCE")
    _CASES[S] = out
    return out


@pytest.mark.parametrize("S", [5, 7])
def test_the_fused_search_on_constant_networks(ea, monkeypatch, S):
    cases = network_cases(ea, S)
    for tile in (None, "32"):
        if tile is not None:
            monkeypatch.setenv("EWN_PUCT_TILE", tile)
        for k, b, d, params, lg, val in cases:
            eta = torch.as_tensor(noise_rows(b.cpu().numpy(), d.cpu().numpy(), k)).cuda()
            eta[0] = 1.0                                                                 # a root that the noise moves
            want = advance_all(ea, b, d, lg, val)
            same(ea.puct_search(b, d, params, SIMS), want, "vector %d, tile %s" % (k, tile))
            noisy = advance_all(ea, b, d, lg, val, noise=eta)
            same(ea.puct_search(b, d, params, SIMS, root_noise=eta, noise_eps=0.25), noisy, "vector %d, tile %s, root noise" % (k, tile))
            if tile is None:
                v = host_views(ea, want, S, SIMS)
                assert np.isfinite(v["p"]).all() and np.isfinite(host_views(ea, noisy, S, SIMS)["p"]).all(), k
                assert np.array_equal(v["n"][:, 0].sum(1), np.full(b.shape[0], SIMS)), k


@pytest.mark.parametrize("S", [5, 7])
def test_predict_puct_and_one_wide_leaf_on_constant_networks(ea, S):
    for k, b, d, params, lg, val in network_cases(ea, S):
        tree = advance_all(ea, b, d, lg, val)
        want = ea.puct_result(tree, S, SIMS, return_visits=True, return_q=True, return_value=True)
        for fused in (True, False):
            got = ea.predict_puct(b, d, params, sims=SIMS, fused=fused, return_visits=True, return_q=True, return_value=True)
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (k, fused)
        assert bool(torch.isfinite(want[3]).all()) and bool((want[1].sum((1, 2)) == SIMS).all()), k
        same(ea.puct_search_wide(b, d, params, SIMS, 1), ea.puct_search(b, d, params, SIMS), "vector %d, one leaf" % k)


@pytest.mark.parametrize("S", [5, 7])
def test_four_wide_leaves_on_constant_networks_against_the_model(ea, S):
    for k, b, d, params, lg, val in network_cases(ea, S):
        got = ea.puct_search_wide(b, d, params, SIMS, 4)
        models = against_the_model(ea, S, b, d, params, SIMS, 4, got, where="vector %d" % k)        # the same P rule: P_TOL, then the bits
        assert all(mod.done == SIMS for mod in models) and np.isfinite(host_views(ea, got, S, SIMS)["p"]).all(), k


@pytest.mark.parametrize("S", [5, 7])
def test_selfplay_on_constant_networks(ea, S):
    T, key, off = 6, 11, 5
    live_rows = 0
    for k, b, d, params, lg, val in network_cases(ea, S):
        kw = dict(sims=SIMS, max_plies=T, key=key, game_offset=off)
        rec = ea.selfplay_puct(b, d, params, **kw)
        same_records(rec, by_hand(ea, S, b, d, params, SIMS, T, key, off))                        # per ply the staged search, then puct_play
        same_records(ea.selfplay_puct(b, d, params, fused=True, chunk=2, **kw), rec)
        live = rec["live"]
        assert bool(live[0].all()) and bool((rec["visits"].sum((2, 3))[live] == SIMS).all()), k
        assert not bool(torch.isnan(rec["value"]).any()) and float(rec["value"].abs().max()) <= 1.0, k
        live_rows += int(live.sum())
    assert live_rows > 3 * len(network_cases(ea, S))


# ---------------------------------------------------------------- 5. lookahead_targets

@pytest.mark.parametrize("tv", [1.0, 10.0])
def test_lookahead_targets_at_small_temperatures(ea, tv):
    rs = np.random.RandomState(int(tv))
    q = (rs.uniform(-tv, tv, size=(96, 6))).astype(F)
    q[rs.uniform(size=q.shape) < 0.35] = -np.inf
    q[0], q[1] = -np.inf, tv                                   # nothing finite; all at the bound
    q[2] = [-tv, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf]  # a lone entry at the lower bound
    q[3] = [tv, -tv, -np.inf, tv, -tv, -np.inf]                # ties at both bounds
    q[4] = [-tv, -tv, -tv, -tv, -tv, F(-tv * (1 - 2.0 ** -23))]  # the maximum one ulp above the rest
    dev = torch.as_tensor(q).cuda()
    for T in (1.0, 1e-3, 1e-6):
        pi, val, w = (t.cpu().numpy() for t in ea.lookahead_targets(dev, T))
        mpi, mval, mw = targets_model(q, T)
        assert np.array_equal(val.view(np.int32), mval.view(np.int32)) and np.array_equal(w, mw)
        qmax = np.where(np.isfinite(q), np.abs(q), 0.0).max(1)
        bound = 8 * 2.0 ** -24 * np.maximum(1.0, qmax / T)     # tests/test_gpu_sup_grad.py's bound at a temperature
        print("tv %g T %g: max |pi - pi_float64| %.3g, the smallest bound %.3g" % (tv, T, np.abs(pi - mpi).max(), bound.min()))
        assert np.isfinite(pi).all() and (pi >= 0).all()
        assert (np.abs(pi - mpi).max(1) <= bound).all(), float((np.abs(pi - mpi).max(1) / bound).max())
        live = w > 0
        assert live.sum() > 80 and not pi[~live].any()
        assert (np.abs(pi[live, :2].sum(1, dtype=np.float64) - 1.0) <= bound[live]).all()
        assert (np.abs(pi[live, 2:].sum(1, dtype=np.float64) - 1.0) <= bound[live]).all()
