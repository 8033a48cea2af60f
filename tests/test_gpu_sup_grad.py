"""ewn_sup_grad (the supervised gradient of the actor-critic on given observations and targets) against torch autograd of the same
loss, and ewn_lookahead_targets against a numpy model of its definition (include/ewn_hip.h).  Observations come from real play (a
RandomAgent rollout with auto-reset), targets from the lookahead search and from random soft distributions with zero weights and
masked heads."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_POOL = {}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def pool(ea, S):
    """34 816 observations of real play on an SxS board (2 048 lanes x 17 steps of RandomAgent against RandomAgent, auto-reset: every
    recorded observation is a live one), every 97th replaced by a finished position (the agent on the far corner: the search returns
    six -inf there), a model and the lookahead's q on all of them: computed once per board size, never modified"""
    if S not in _POOL:
        from tests.test_gpu_policy import make_model
        N, K = 2048, 17
        env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=31 + S)
        env.reset(seeds=(np.arange(N, dtype=np.uint64) + 7).astype(np.uint32))
        traj = env.alloc_rollout(K)
        env.rollout(K, agent="random", traj=traj)
        boards = traj["board"].reshape(K * N, S, S).contiguous()
        dice = traj["dice"].reshape(K * N).contiguous()
        won = torch.zeros((S, S), dtype=torch.int8, device="cuda")
        won[S - 1, S - 1], won[1, 1], won[S - 2, 2] = 2, 5, -3
        boards[::97] = won
        model = make_model(S, 11 + S, head_gain=1.0)
        params = model.flat_parameters()
        _, q = ea.predict_lookahead(boards, dice, params, return_q=True)
        _POOL[S] = {"env": env, "boards": boards, "dice": dice, "model": model, "params": params, "q": q}
    return _POOL[S]


def soft_targets(M, seed, device="cuda"):
    """random soft targets: each head a random distribution, head 0 masked on ~15 % of the rows and head 1 on another ~15 %, random
    weights k / 64 in [0.5, 1.5] with ~10 % zeros (multiples of 1/64: every partial sum of up to 2^17 of them is exact in fp32, in
    any order, so the weight sum [P + 3] can be held to equality)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tp = torch.cat([torch.softmax(2.0 * torch.randn(M, 2, generator=g), 1), torch.softmax(2.0 * torch.randn(M, 3, generator=g), 1)], 1)
    u = torch.rand(M, generator=g)
    tp[u < 0.15, :2] = 0.0
    tp[(u >= 0.15) & (u < 0.30), 2:] = 0.0
    tv = 2.0 * torch.rand(M, generator=g) - 1.0
    w = torch.randint(32, 97, (M,), generator=g).float() / 64.0
    w[torch.rand(M, generator=g) < 0.10] = 0.0
    return tp.to(device), tv.to(device), w.to(device)


def pick_flag(z):
    return (z[:, 1] > z[:, 0]).long()


def pick_dir(z):
    two = torch.full_like(z[:, 0], 2, dtype=torch.long)
    return torch.where(z[:, 1] > z[:, 0], torch.where(z[:, 2] > z[:, 1], two, two - 1), torch.where(z[:, 2] > z[:, 0], two, two - 2))


def torch_loss(model, b, d, tp, tv, w, pi_coef, vf_coef):
    """the loss of include/ewn_hip.h in plain torch (the model's dtype); zero-weight rows' targets are replaced by zeros.  Returns
    (loss, the five sums [P + 0 .. P + 4])"""
    dt = model.value_net.weight.dtype
    M = b.shape[0]
    w = torch.ones(M, device=b.device) if w is None else w
    live = w > 0
    zero = torch.zeros((), device=b.device, dtype=dt)
    tp0, tv0, w0 = torch.where(live[:, None], tp.to(dt), zero), torch.where(live, tv.to(dt), zero), torch.where(live, w.to(dt), zero)
    l0, l1, V = model(b, d)
    lp0, lp1 = torch.log_softmax(l0, 1), torch.log_softmax(l1, 1)
    ce = -(tp0[:, :2] * lp0).sum(1) - (tp0[:, 2:] * lp1).sum(1)
    loss = (w0 * (pi_coef * ce + vf_coef * (V - tv0) ** 2)).sum() / M
    with torch.no_grad():
        ent = -(lp0.exp() * lp0).sum(1) - (lp1.exp() * lp1).sum(1)
        ok0 = (tp0[:, :2].sum(1) == 0) | (pick_flag(l0) == pick_flag(tp0[:, :2]))
        ok1 = (tp0[:, 2:].sum(1) == 0) | (pick_dir(l1) == pick_dir(tp0[:, 2:]))
        sums = [float((w0 * ce).sum()), float((w0 * ent).sum()), int((ok0 & ok1 & live).sum()), float(w0.sum()), float((w0 * (V - tv0) ** 2).sum())]
    return loss, sums


def torch_grad(model, *args):
    m = copy.deepcopy(model)
    m.zero_grad()
    loss, sums = torch_loss(m, *args)
    loss.backward()
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]), sums


def check_against_torch(model, got, b, d, tp, tv, w, pi_coef, vf_coef, ctx):
    """tests/test_gpu_a2c_fused.py's bounds on this body: relative L2 < 2e-4, allclose(rtol 5e-3, atol 2e-5 max|ref|), every named
    block < 2e-3; the sums within 1e-4 of the sum, the agreement count and the weight sum [P + 3] exactly (the weights of every case
    here are multiples of 1/64: their sums are exact in fp32 in any order)"""
    ref, sums = torch_grad(model, b, d, tp, tv, w, pi_coef, vf_coef)
    g, st = got[:-8], got[-8:].tolist()
    if float(ref.norm()) > 0:
        rel = float((g - ref).norm() / ref.norm())
        assert rel < 2e-4, (ctx, rel, float(ref.norm()))
    assert torch.allclose(g, ref, rtol=5e-3, atol=2e-5 * float(ref.abs().max())), (ctx, float((g - ref).abs().max()))
    off = 0
    for name, p in model.named_parameters():
        x, y = g[off:off + p.numel()], ref[off:off + p.numel()]
        off += p.numel()
        if float(y.norm()) > 0:
            assert float((x - y).norm() / y.norm()) < 2e-3, (ctx, name)
        else:
            assert float(x.abs().max()) == 0.0, (ctx, name)
    assert off == g.numel()
    print("sums", ctx, st, sums)
    for i in (0, 1, 4):
        assert abs(st[i] - sums[i]) <= 1e-4 * max(abs(sums[i]), 1e-30), (ctx, i, st[i], sums[i])
    assert st[2] == float(sums[2]), (ctx, st[2], sums[2])
    wsum = float(torch.where(w > 0, w, torch.zeros_like(w)).double().sum()) if w is not None else float(b.shape[0])
    assert st[3] == wsum and sums[3] == wsum, (ctx, st[3], sums[3], wsum)
    assert st[5:] == [0.0, 0.0, 0.0], (ctx, st)
    return ref


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 31, 33, 129, 32801])
def test_gradient_matches_torch_autograd(ea, S, M):
    """a lone lane; a partial tile and a tile plus one; a second block (four tiles fill one); past the 256-block cap of 32 768 samples
    (the grid-stride path).  Targets from the search (weights 0 / 1: [P + 3] is then a count and must match exactly) and random soft
    ones."""
    p = pool(ea, S)
    off = 1000 if M < 1000 else 0
    b, d, q = p["boards"][off:off + M], p["dice"][off:off + M], p["q"][off:off + M]
    tp, tv, w = ea.lookahead_targets(q)
    got = ea.sup_grad(b, d, tp, tv, p["params"], weight=w, pi_coef=1.0, vf_coef=0.5)
    check_against_torch(p["model"], got, b, d, tp, tv, w, 1.0, 0.5, ("search", S, M))
    assert float(got[-5]) == float((w > 0).sum())
    tp, tv, w = soft_targets(M, 100 + M)
    got = ea.sup_grad(b, d, tp, tv, p["params"], weight=w, pi_coef=0.7, vf_coef=0.3)
    check_against_torch(p["model"], got, b, d, tp, tv, w, 0.7, 0.3, ("soft", S, M))


def test_finished_rows_carry_weight_zero(ea):
    """the pool's finished observations: the search returns six -inf there, and the targets give exactly them weight 0"""
    for S in (5, 7):
        p = pool(ea, S)
        dead = torch.isneginf(p["q"]).all(2).all(1)
        _, _, w = ea.lookahead_targets(p["q"])
        assert torch.equal(w == 0, dead) and bool(dead[::97].all()) and int(dead.sum()) < dead.numel() // 50


@pytest.mark.parametrize("S,M", [(5, 6000), (7, 2000)])
def test_gradient_is_fp32_accurate_against_float64(ea, S, M):
    """Against the same model and loss in FLOAT64 the engine's gradient must be within twice plain fp32 torch's relative error on the
    same inputs (test_bf16x3_7x7_gradient_is_fp32_accurate's construction).  Measured on the MI355X on these inputs: 5x5, M = 6 000:
    the engine 1.35e-7, plain fp32 torch 7.91e-8; 7x7, M = 2 000: the engine 7.28e-8, fp32 torch 4.14e-7 (both
    figures are printed by this test)."""
    p = pool(ea, S)
    b, d = p["boards"][:M], p["dice"][:M]
    tp, tv, w = soft_targets(M, 7)
    got = ea.sup_grad(b, d, tp, tv, p["params"], weight=w, pi_coef=1.0, vf_coef=0.5)[:-8].double()
    g64, _ = torch_grad(copy.deepcopy(p["model"]).double(), b, d, tp, tv, w, 1.0, 0.5)
    g32, _ = torch_grad(p["model"], b, d, tp, tv, w, 1.0, 0.5)
    e_engine = float((got - g64).norm() / g64.norm())
    e_torch = float((g32.double() - g64).norm() / g64.norm())
    print("float64 accuracy S=%d M=%d: engine %.3e, fp32 torch %.3e" % (S, M, e_engine, e_torch))
    assert e_engine < 2.0 * e_torch, (e_engine, e_torch)


def _blocks(model):
    out, off = {}, 0
    for name, p in model.named_parameters():
        out[name] = (off, off + p.numel())
        off += p.numel()
    return out


@pytest.mark.parametrize("S", [5, 7])
def test_exactness(ea, S):
    p = pool(ea, S)
    M = 1000
    b, d, params, model = p["boards"][:M], p["dice"][:M], p["params"], p["model"]
    tp, tv, w = soft_targets(M, 3)
    bits = lambda x: x.view(torch.int32)          # noqa: E731
    g = ea.sup_grad(b, d, tp, tv, params, weight=w)
    assert torch.equal(bits(g), bits(ea.sup_grad(b, d, tp, tv, params, weight=w)))            # call to call
    blk = _blocks(model)
    pol = torch.zeros(g.numel() - 8, dtype=torch.bool, device="cuda")
    for name, (lo, hi) in blk.items():
        if name.startswith("pi.") or name.startswith("action_net."):
            pol[lo:hi] = True
    # vf_coef 0: value body and head exactly zero, the policy part bit-equal; pi_coef 0: the mirror image
    g0 = ea.sup_grad(b, d, tp, tv, params, weight=w, vf_coef=0.0)
    assert float(g0[:-8][~pol].abs().max()) == 0.0 and torch.equal(bits(g0[:-8][pol]), bits(g[:-8][pol]))
    assert torch.equal(bits(g0[-8:-4]), bits(g[-8:-4]))
    g1 = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=0.0)
    assert float(g1[:-8][pol].abs().max()) == 0.0 and torch.equal(bits(g1[:-8][~pol]), bits(g[:-8][~pol]))
    assert torch.equal(bits(g1[-4:]), bits(g[-4:]))
    # weight None == explicit ones
    assert torch.equal(bits(ea.sup_grad(b, d, tp, tv, params)), bits(ea.sup_grad(b, d, tp, tv, params, weight=torch.ones(M, device="cuda"))))
    # zero-weight rows: other boards, NaN / -inf targets -> finite and bit-identical to zeros there
    dead = w == 0
    assert int(dead.sum()) > 10
    tpz, tvz = tp.clone(), tv.clone()
    tpz[dead], tvz[dead] = 0.0, 0.0
    gz = ea.sup_grad(b, d, tpz, tvz, params, weight=w)
    b2, d2, tpn, tvn = b.clone(), d.clone(), tp.clone(), tv.clone()
    b2[dead], d2[dead] = p["boards"][5000:5000 + M][dead], p["dice"][5000:5000 + M][dead]
    idx = torch.nonzero(dead).reshape(-1)
    tpn[idx[0::2]], tvn[idx[0::2]] = float("nan"), float("-inf")
    tpn[idx[1::2]], tvn[idx[1::2]] = float("-inf"), float("nan")
    gn = ea.sup_grad(b2, d2, tpn, tvn, params, weight=w)
    assert bool(torch.isfinite(gn).all()) and torch.equal(bits(gn), bits(gz)) and torch.equal(bits(gz), bits(g))
    # a masked head: its action-head rows get exactly nothing, the other head's rows are what torch computes for that head alone
    (alo, _), (blo, _) = blk["action_net.weight"], blk["action_net.bias"]
    for rows, sl in (((0, 1), slice(0, 2)), ((2, 3, 4), slice(2, 5))):
        tm = tp.clone()
        tm[:, sl] = 0.0
        gm = ea.sup_grad(b, d, tm, tv, params, weight=w)
        ref = check_against_torch(model, gm, b, d, tm, tv, w, 1.0, 0.5, ("masked", S, rows))
        for r in range(5):
            row = torch.cat([gm[alo + 64 * r:alo + 64 * (r + 1)], gm[blo + r:blo + r + 1]])
            rrow = torch.cat([ref[alo + 64 * r:alo + 64 * (r + 1)], ref[blo + r:blo + r + 1]])
            if r in rows:
                assert float(row.abs().max()) == 0.0 and float(rrow.abs().max()) == 0.0, (S, r)
            else:
                assert float((row - rrow).norm() / rrow.norm()) < 2e-3, (S, r)


def targets_model(q, T):
    """ewn_lookahead_targets as include/ewn_hip.h defines it, row by row in numpy (float64 for temperature > 0)"""
    M = q.shape[0]
    pi, val, w = np.zeros((M, 5), np.float64), np.zeros(M, np.float32), np.zeros(M, np.float32)
    for m in range(M):
        x = q[m]
        fin = [i for i in range(6) if x[i] > -np.inf]
        if not fin:
            continue
        best = fin[0]
        for i in fin:
            if x[i] > x[best]:
                best = i
        w[m], val[m] = 1.0, x[best]
        if T == 0:
            f, r = divmod(best, 3)
            pi[m, 2 + r] = 1.0
            if x[r:r + 1].view(np.int32)[0] == x[3 + r:4 + r].view(np.int32)[0]:
                pi[m, 0] = pi[m, 1] = 0.5
            else:
                pi[m, f] = 1.0
        else:
            e = np.zeros(6)
            for i in fin:
                e[i] = math.exp((float(x[i]) - float(x[best])) / T)
            e /= e.sum()
            pi[m] = [e[0] + e[1] + e[2], e[3] + e[4] + e[5], e[0] + e[3], e[1] + e[4], e[2] + e[5]]
    return pi, val, w


def constructed_q(ea):
    """q rows that exercise every rule: the search on a one-cube position (both flags name the cube: equal bits), on a finished board
    (six -inf) and on play positions; equal finite entries (the first maximum), -inf patterns, a lone finite entry, large values"""
    S, E = 5, 4
    p = pool(ea, S)
    b = torch.zeros((2, S, S), dtype=torch.int8)
    b[0, 1, 1], b[0, 3, 3] = 3, -2                       # one cube a side, dice 4: both flags move cube 3
    b[1, E, E], b[1, 1, 1], b[1, E - 1, 2] = 2, 5, -3    # already won: six -inf
    _, qc = ea.predict_lookahead(b.cuda(), torch.tensor([4, 2], dtype=torch.int8).cuda(), p["params"], return_q=True)
    ninf = -np.inf
    hand = np.array([[0.25, 0.25, 0.1, 0.25, 0.3, 0.3],          # the maximum 0.3 twice: (1, 1) is the first
                     [0.5, 0.5, 0.5, 0.5, 0.5, 0.5],             # all equal: (0, 0), and the flag entries tie
                     [ninf, 0.2, ninf, 0.2, ninf, 0.7],
                     [ninf, ninf, ninf, ninf, -0.9, ninf],       # a lone finite entry
                     [ninf] * 6,
                     [-0.0, 0.0, -1.0, 0.0, -0.0, -1.0],         # equal values, different bits: no flag tie where the bits differ
                     [30.0, -30.0, 1.0, 29.5, 0.0, ninf],
                     [1.0, -1.0, ninf, 1.0, -1.0, ninf]], dtype=np.float32)
    return torch.cat([qc.reshape(-1, 6), torch.from_numpy(hand).cuda(), p["q"][:500].reshape(-1, 6)])


def test_lookahead_targets_against_the_numpy_model(ea):
    q = constructed_q(ea)
    qn = q.cpu().numpy()
    assert qn[0, 0:3].view(np.int32).tolist() == qn[0, 3:6].view(np.int32).tolist() and np.isfinite(qn[0]).any()   # the one-cube tie
    assert np.isneginf(qn[1]).all() and np.isneginf(qn[10:]).all(1).any()
    pi, val, w = (t.cpu().numpy() for t in ea.lookahead_targets(q.reshape(-1, 2, 3), 0.0))
    mpi, mval, mw = targets_model(qn, 0.0)
    assert np.array_equal(pi, mpi.astype(np.float32)) and np.array_equal(val.view(np.int32), mval.view(np.int32)) and np.array_equal(w, mw)
    assert pi[0, :2].tolist() == [0.5, 0.5] and w[1] == 0 and not pi[1].any()
    assert pi[2].tolist() == [0, 1, 0, 1, 0] and pi[3].tolist() == [0.5, 0.5, 1, 0, 0]
    for T in (0.5, 2.0):
        pi, val, w = (t.cpu().numpy() for t in ea.lookahead_targets(q, T))
        mpi, mval, mw = targets_model(qn, T)
        assert np.array_equal(val.view(np.int32), mval.view(np.int32)) and np.array_equal(w, mw)
        qmax = np.where(np.isfinite(qn), np.abs(qn), 0.0).max(1)
        bound = 8 * 2.0 ** -24 * np.maximum(1.0, qmax / T)
        assert (np.abs(pi - mpi).max(1) <= bound).all(), float((np.abs(pi - mpi).max(1) / bound).max())
        live = w > 0
        assert (np.abs(pi[live, :2].sum(1, dtype=np.float64) - 1.0) <= bound[live]).all()
        assert (np.abs(pi[live, 2:].sum(1, dtype=np.float64) - 1.0) <= bound[live]).all()
        assert not pi[~live].any()


@pytest.mark.parametrize("S", [5, 7])
def test_guard_zones(ea, S):
    """4 KB guard zones directly around every buffer of ewn_sup_grad at M = 33 (a tile plus one), with the scratch 16-byte aligned and
    4 bytes past (the row area is then rounded up inside it, and the other reduce kernel runs), and around ewn_lookahead_targets'
    three outputs"""
    from tests.guarded_alloc import GuardedAllocator
    from ewn_gym_amd import _lib
    p = pool(ea, S)
    M = 33
    alloc = GuardedAllocator()
    P = p["params"].numel()
    nscr = int(_lib.load().ewn_sup_scratch_bytes(S, 3, M))
    tp0, tv0, w0 = soft_targets(M, 5)
    buf = {}
    for name, src in (("boards", p["boards"][40:40 + M]), ("dice", p["dice"][40:40 + M]), ("target_pi", tp0), ("target_value", tv0),
                      ("weight", w0), ("params", p["params"])):
        buf[name] = alloc.zeros(src.shape, dtype=src.dtype, tag=name)
        buf[name].copy_(src)
    ref = None
    for offset in (0, 4):
        grad = alloc.zeros(P + 8, dtype=torch.float32, tag="grad")
        scratch = alloc.zeros(nscr, dtype=torch.uint8, tag="scratch+%d" % offset, offset=offset)
        assert scratch.data_ptr() % 16 == offset
        out = ea.sup_grad(buf["boards"], buf["dice"], buf["target_pi"], buf["target_value"], buf["params"], weight=buf["weight"], out=grad,
                          scratch=scratch)
        torch.cuda.synchronize()
        assert out.data_ptr() == grad.data_ptr()
        alloc.check("ewn_sup_grad S=%d scratch offset %d" % (S, offset))
        if ref is None:
            ref = grad.clone()
            check_against_torch(p["model"], grad, buf["boards"], buf["dice"], tp0, tv0, w0, 1.0, 0.5, ("guard", S))
        else:
            assert float((grad[:-8] - ref[:-8]).abs().max()) <= 1e-6 * float(ref[:-8].abs().max())
    with alloc.patch("lookahead_targets"):
        outs = ea.lookahead_targets(p["q"][:M], 0.5)
    torch.cuda.synchronize()
    assert all(alloc.owns(t) for t in outs)
    alloc.check("ewn_lookahead_targets")


@pytest.mark.parametrize("S", [5, 7])
def test_fixed_batch_descent(ea, S):
    """one fixed batch of 257 play positions with random one-hot targets and random values, 30 x (ewn_sup_grad, ewn_a2c_apply with
    lr 7e-4 and clip 0.5): the mean cross-entropy and the mean squared error end strictly below where they started.  (The same loop
    in fp32 torch on the CPU, on random boards: CE 1.62 -> 0.61 and MSE 0.69 -> 0.004 on 5x5, 1.64 -> 0.41 and 0.75 -> 0.002 on 7x7.)"""
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    p = pool(ea, S)
    M = 257
    b, d = p["boards"][2000:2000 + M], p["dice"][2000:2000 + M]
    g = torch.Generator().manual_seed(S)
    tp = torch.zeros(M, 5)
    tp[torch.arange(M), torch.randint(0, 2, (M,), generator=g)] = 1.0
    tp[torch.arange(M), 2 + torch.randint(0, 3, (M,), generator=g)] = 1.0
    tv = 2.0 * torch.rand(M, generator=g) - 1.0
    tp, tv = tp.cuda(), tv.cuda()
    params = p["params"].clone()
    sq = torch.zeros_like(params)
    grad = torch.zeros(params.numel() + 8, device="cuda")
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    env = p["env"]
    hist = []
    for _ in range(30):
        ea.sup_grad(b, d, tp, tv, params, out=grad)
        hist.append(grad[-8:].clone())
        check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), None, _stream()), "ewn_a2c_apply")
    first, last = hist[0].tolist(), hist[-1].tolist()
    assert first[3] == M and last[3] == M
    print("descent S=%d: CE %.4f -> %.4f, MSE %.4f -> %.4f" % (S, first[0] / M, last[0] / M, first[4] / M, last[4] / M))
    assert last[0] / last[3] < first[0] / first[3]
    assert last[4] / last[3] < first[4] / first[3]
