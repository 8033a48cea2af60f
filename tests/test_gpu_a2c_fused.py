"""The fused A2C update (ewn_a2c_grad / ewn_a2c_apply) against torch autograd of the same loss on the same trajectory, and the
fused trainer end to end.  SB3 itself is absent (parity unpinned): the reference here is a plain fp32 torch implementation of
SB3's documented A2C loss (ewn_gym_amd.a2c: n-step returns with gae_lambda 1, policy gradient + vf_coef * MSE + ent_coef * -entropy,
clip_grad_norm_, RMSprop)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def _torch_loss(model, traj, K, gamma, vf_coef, ent_coef):
    from ewn_gym_amd.a2c import n_step_returns
    obs_b, obs_d = traj["obs_board"], traj["obs_dice"]
    N = obs_b.shape[1]
    S = obs_b.shape[2]
    with torch.no_grad():
        vals = torch.stack([model(obs_b[t], obs_d[t])[2] for t in range(K)])
        last = model(obs_b[K], obs_d[K])[2]
        adv, ret = n_step_returns(traj["reward"].float(), vals, traj["terminated"].float(), last, gamma, 1.0)
    logp, ent, value = model.evaluate_actions(obs_b[:K].reshape(K * N, S, S), obs_d[:K].reshape(K * N), traj["action"].reshape(K * N, 2))
    pl = -(adv.reshape(-1) * logp).mean()
    vl = torch.nn.functional.mse_loss(ret.reshape(-1), value)
    en = ent.mean()
    return pl + vf_coef * vl - ent_coef * en, pl, vl, en


@pytest.mark.parametrize("N,S,K,ent_coef,opp", [(3000, 5, 5, 0.0, "minimax"), (1000, 5, 3, 0.01, "random"), (40000, 5, 5, 0.0, "minimax"),
                                                (700, 7, 4, 0.02, "minimax"),
                                                # edges: one lane; K = 1 in a single partial 32-lane tile; a 7x7 tile and a bit; an odd
                                                # K * N (partial only 4-byte aligned: the fallback k_a2c_reduce); 7x7 past the 256-block cap
                                                (1, 5, 5, 0.01, "minimax"), (31, 5, 1, 0.0, "random"), (33, 7, 3, 0.01, "minimax"),
                                                (1001, 5, 3, 0.0, "minimax"), (40000, 7, 5, 0.0, "minimax")])
def test_fused_gradient_matches_torch_autograd(ea, N, S, K, ent_coef, opp):
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    from tests.test_gpu_policy import make_model
    env = ea.VecEWN(N, board_size=S, opponent_policy=opp, max_depth=2, rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=5,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=21)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 3).astype(np.uint32))
    model = make_model(S, 11, head_gain=1.0)
    params = model.flat_parameters()
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    for _ in range(3):            # a few launches so that the trajectories hold terminal steps, resets and tolerance penalties
        env.rollout_policy(K, params, traj=traj, noise_key=5)
    gamma, vf_coef = 0.97, 0.5
    hp = EwnA2cHyper(gamma, vf_coef, ent_coef, 0.5, 7e-4, 0.99, 1e-5, 1)
    nscr = check(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), K))
    scratch = torch.zeros(int(nscr), dtype=torch.uint8, device="cuda")
    grad = torch.zeros(params.numel() + 8, dtype=torch.float32, device="cuda")
    check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad),
                               _ptr(scratch), _stream()), "ewn_a2c_grad")
    loss, pl, vl, en = _torch_loss(model, traj, K, gamma, vf_coef, ent_coef)
    model.zero_grad()
    loss.backward()
    ref = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    pl, vl, en = pl.detach(), vl.detach(), en.detach()
    got = grad[:-8]
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 2e-4, (rel, float(ref.norm()))
    assert torch.allclose(got, ref, rtol=5e-3, atol=2e-5 * float(ref.abs().max())), float((got - ref).abs().max())
    # every parameter block on its own (a mis-indexed block would hide in the global norm)
    off = 0
    for name, p in model.named_parameters():
        a, b = got[off:off + p.numel()], ref[off:off + p.numel()]
        off += p.numel()
        if float(b.norm()) > 0:
            assert float((a - b).norm() / b.norm()) < 2e-3, name
    st = grad[-8:].tolist()
    n = K * N
    assert abs(st[0] / n - float(pl)) < 1e-4 * max(1.0, abs(float(pl))) and abs(st[5] / n - float(vl)) < 1e-4 * max(1.0, float(vl))
    assert abs(st[2] / n - float(en)) < 1e-4
    # the other five of the eight loss sums (include/ewn_hip.h, ewn_a2c_grad): the policy pass counts no value loss, the value pass no
    # policy loss or entropy, and slots 3 / 7 are always zero -- exactly
    assert [st[1], st[3], st[4], st[6], st[7]] == [0.0] * 5, st
    # bit-reproducible: the same call again gives the same bits
    grad2 = torch.zeros_like(grad)
    check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad2),
                               _ptr(scratch), _stream()), "ewn_a2c_grad")
    assert torch.equal(grad, grad2)
    # the other reduce kernel on the same inputs: the scratch 4 bytes further on flips the 8-byte alignment of `partial`
    # (= scratch + 4 K N bytes), so of k_a2c_reduce2 / k_a2c_reduce the call takes the one the first did not
    scratch4 = torch.zeros(int(nscr) + 4, dtype=torch.uint8, device="cuda")
    grad3 = torch.zeros_like(grad)
    check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad3),
                               C.c_void_p(scratch4.data_ptr() + 4), _stream()), "ewn_a2c_grad")
    assert (scratch.data_ptr() + 4 * K * N) % 8 != (scratch4.data_ptr() + 4 + 4 * K * N) % 8
    assert float((grad3[:-8] - grad[:-8]).abs().max()) <= 1e-6 * float(grad[:-8].abs().max())
    for i in range(8):
        assert abs(float(grad3[-8 + i]) - st[i]) <= 1e-6 * abs(st[i]), (i, float(grad3[-8 + i]), st[i])


def _apply_f64(params, sq, grad, P, world, max_norm, lr=7e-4, alpha=0.99, eps=1e-5):
    """clip_grad_norm_ + RMSprop in float64 on (params, sq) in place; returns the norm before clipping"""
    g = grad[:P].double() / world
    norm = float(g.norm())
    if max_norm > 0:
        g = g * min(1.0, max_norm / (norm + 1e-6))
    sq.mul_(alpha).add_((1 - alpha) * g * g)
    params.sub_(lr * g / (sq.sqrt() + eps))
    return norm


def test_fused_apply_is_clip_plus_rmsprop(ea):
    """5x5 and 7x7, each on aligned buffers (k_a2c_apply<true>) and on views one float past a 16-byte boundary (the scalar k_a2c_apply<false>);
    max_grad_norm 0 takes no clipping (the norm is still reported).  Against torch fp32 and float64."""
    for S in (5, 7):
        for offset in (0, 1):
            _apply_case(ea, S, offset)


def _apply_case(ea, S, offset):
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    env = ea.VecEWN(64, board_size=S, opponent_policy="random", rng="philox")
    P = env.policy_param_count()
    g = torch.Generator(device="cuda").manual_seed(0)
    for scale, world, mgn in ((3.0, 1, 0.5), (1e-3, 1, 0.5), (2.0, 4, 0.5), (3.0, 1, 0.0), (2.0, 4, 0.0)):
        params = torch.zeros(P + offset, device="cuda")[offset:]
        params.copy_(torch.randn(P, device="cuda", generator=g))
        grad = torch.zeros(P + 8 + offset, device="cuda")[offset:]
        grad.copy_(torch.randn(P + 8, device="cuda", generator=g) * scale)
        assert (params.data_ptr() % 16 == 0) == (offset == 0)
        ref_p = torch.nn.Parameter(params.clone())
        opt = torch.optim.RMSprop([ref_p], lr=7e-4, alpha=0.99, eps=1e-5)
        p64, sq64 = params.double(), torch.zeros(P, dtype=torch.float64, device="cuda")
        sq = torch.zeros(P + offset, device="cuda")[offset:]
        norm = torch.zeros(1, device="cuda")
        hp = EwnA2cHyper(0.99, 0.5, 0.0, mgn, 7e-4, 0.99, 1e-5, world)
        for it in range(3):
            ref_p.grad = grad[:P].clone() / world
            if mgn > 0:
                tn = torch.nn.utils.clip_grad_norm_([ref_p], mgn)
            else:
                tn = ref_p.grad.norm()
            opt.step()
            n64 = _apply_f64(p64, sq64, grad, P, world, mgn)
            check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()))
            ctx = (S, offset, scale, world, mgn, it)
            assert abs(float(norm) - float(tn)) < 1e-4 * float(tn), ctx
            assert abs(float(norm) - n64) < 1e-4 * n64, ctx
            assert torch.allclose(params, ref_p.data, rtol=1e-5, atol=1e-6), ctx
            assert torch.allclose(params.double(), p64, rtol=1e-5, atol=1e-6), ctx
            assert torch.allclose(sq.double(), sq64, rtol=1e-4, atol=1e-12), ctx


def test_fused_trainer_learns_and_matches_the_torch_trainer_step(ea):
    """One update of FusedA2CTrainer == the same update done by torch (autograd + clip + RMSprop) on the trajectory it collected;
    a short run beats the illegal-move habit of a fresh policy (mean reward rises)."""
    from ewn_gym_amd.a2c import ActorCritic, FusedA2CTrainer
    N = 8192
    env = ea.VecEWN(N, opponent_policy="minimax", max_depth=3, rng="philox", shaped=True, reward=10.0, illegal_move_reward=-1.0,
                    illegal_move_tolerance=10, shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=9487)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 9487).astype(np.uint32))
    tr = FusedA2CTrainer(env, n_steps=5, learning_rate=7e-4, seed=1, use_graph=True)
    before = tr.params.clone()
    tr.collect_and_update()        # eager
    torch.cuda.synchronize()
    ref = ActorCritic(5, 6).cuda()
    ref.load_flat_parameters(before)
    loss, _, _, _ = _torch_loss(ref, tr.traj, 5, 0.99, 0.5, 0.0)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
    opt = torch.optim.RMSprop(ref.parameters(), lr=7e-4, alpha=0.99, eps=1e-5)
    opt.step()
    assert torch.allclose(tr.params, ref.flat_parameters(), rtol=1e-4, atol=2e-6), float((tr.params - ref.flat_parameters()).abs().max())
    # the module views the flat vector: the torch-side policy sees the update
    assert torch.equal(tr.model.flat_parameters(), tr.params)
    first = None
    for it in range(150):          # graph replays from the second update on
        tr.collect_and_update()
        if it == 1:
            first = tr.stats_dict()
    last = tr.stats_dict()
    assert np.isfinite(last["loss"]) and last["grad_norm"] > 0
    assert last["mean_reward"] > first["mean_reward"] + 0.05, (first, last)


def test_bf16x3_forward_and_gradient_are_fp32_accurate(ea):
    """The network runs on the bf16 matrix pipe with every operand split into three bf16 parts (csrc/ewn_mlp3.hpp).  The claim is fp32
    accuracy: against the same model evaluated in FLOAT64 the engine's logits and gradient must be as close as plain fp32 torch is
    (measured, tools/a2c_accuracy.py: logits 6.9e-7 vs 1.0e-6, gradient 5.6e-8 vs 6.3e-8 relative)."""
    import copy
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.a2c import n_step_returns
    from ewn_gym_amd.vec_env import _ptr, _stream
    from tests.test_gpu_policy import make_model
    N, S, K = 6000, 5, 5
    env = ea.VecEWN(N, board_size=S, opponent_policy="minimax", max_depth=2, rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=5,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=23)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 5).astype(np.uint32))
    model = make_model(S, 13, head_gain=1.0)
    params = model.flat_parameters()
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    logits = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    for _ in range(3):
        env.rollout_policy(K, params, traj=traj, noise_key=5, logits=logits)
    gamma, vf_coef, ent_coef = 0.97, 0.5, 0.01
    hp = EwnA2cHyper(gamma, vf_coef, ent_coef, 0.5, 7e-4, 0.99, 1e-5, 1)
    scratch = torch.zeros(int(check(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), K))), dtype=torch.uint8, device="cuda")
    grad = torch.zeros(params.numel() + 8, dtype=torch.float32, device="cuda")
    check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad),
                               _ptr(scratch), _stream()), "ewn_a2c_grad")
    m64 = copy.deepcopy(model).double()
    obs_b, obs_d = traj["obs_board"], traj["obs_dice"]
    with torch.no_grad():
        l64 = torch.stack([torch.cat(m64(obs_b[t], obs_d[t])[:2], 1) for t in range(K)])
        vals = torch.stack([m64(obs_b[t], obs_d[t])[2] for t in range(K)])
        adv, ret = n_step_returns(traj["reward"].double(), vals, traj["terminated"].double(), m64(obs_b[K], obs_d[K])[2], gamma, 1.0)
    logp, ent, value = m64.evaluate_actions(obs_b[:K].reshape(K * N, S, S), obs_d[:K].reshape(K * N), traj["action"].reshape(K * N, 2))
    loss = -(adv.reshape(-1) * logp).mean() + vf_coef * torch.nn.functional.mse_loss(ret.reshape(-1), value) - ent_coef * ent.mean()
    loss.backward()
    g64 = torch.cat([p.grad.reshape(-1) for p in m64.parameters()])
    assert float((logits.double() - l64).abs().max()) < 3e-6
    assert float((grad[:-8].double() - g64).norm() / g64.norm()) < 5e-7


def _errors_vs_float64(ea, N, S, K, philox_key, seed):
    """(engine logits, engine gradient, fp32 torch logits, fp32 torch gradient): max abs logit error and relative gradient error of the
    engine and of plain fp32 torch against the same model evaluated in float64, on one trajectory"""
    import copy
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.a2c import n_step_returns
    from ewn_gym_amd.vec_env import _ptr, _stream
    from tests.test_gpu_policy import make_model
    env = ea.VecEWN(N, board_size=S, opponent_policy="minimax", max_depth=2, rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=5,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=philox_key)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 5).astype(np.uint32))
    model = make_model(S, seed, head_gain=1.0)
    params = model.flat_parameters()
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    logits = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    for _ in range(3):
        env.rollout_policy(K, params, traj=traj, noise_key=5, logits=logits)
    gamma, vf_coef, ent_coef = 0.97, 0.5, 0.01
    hp = EwnA2cHyper(gamma, vf_coef, ent_coef, 0.5, 7e-4, 0.99, 1e-5, 1)
    scratch = torch.zeros(int(check(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), K))), dtype=torch.uint8, device="cuda")
    grad = torch.zeros(params.numel() + 8, dtype=torch.float32, device="cuda")
    check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad),
                               _ptr(scratch), _stream()), "ewn_a2c_grad")
    obs_b, obs_d = traj["obs_board"], traj["obs_dice"]

    def torch_run(m, dt):
        with torch.no_grad():
            lg = torch.stack([torch.cat(m(obs_b[t], obs_d[t])[:2], 1) for t in range(K)])
            vals = torch.stack([m(obs_b[t], obs_d[t])[2] for t in range(K)])
            adv, ret = n_step_returns(traj["reward"].to(dt), vals, traj["terminated"].to(dt), m(obs_b[K], obs_d[K])[2], gamma, 1.0)
        logp, ent, value = m.evaluate_actions(obs_b[:K].reshape(K * N, S, S), obs_d[:K].reshape(K * N), traj["action"].reshape(K * N, 2))
        loss = -(adv.reshape(-1) * logp).mean() + vf_coef * torch.nn.functional.mse_loss(ret.reshape(-1), value) - ent_coef * ent.mean()
        loss.backward()
        return lg.double(), torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double()

    l64, g64 = torch_run(copy.deepcopy(model).double(), torch.float64)
    l32, g32 = torch_run(copy.deepcopy(model), torch.float32)

    def rel(g):
        return float((g - g64).norm() / g64.norm())
    return (float((logits.double() - l64).abs().max()), rel(grad[:-8].double()), float((l32 - l64).abs().max()), rel(g32))


def test_bf16x3_7x7_gradient_is_fp32_accurate(ea):
    """test_bf16x3_forward_and_gradient_are_fp32_accurate's construction on 7x7 (F = 56 features, P = 16 006), 2 000 lanes x 5 steps.
    Measured against float64 on these inputs (MI355X): plain fp32 torch 4.6e-7 max abs on the logits and 8.7e-8 relative on the
    gradient; the engine 6.0e-7 and 7.6e-8.  The bounds are about twice fp32 torch's error: 1e-6 and 2e-7."""
    el, eg, tl, tg = _errors_vs_float64(ea, 2000, 7, 5, 29, 19)
    assert el < 1e-6, (el, tl)
    assert eg < 2e-7, (eg, tg)
