"""The data-parallel update of the fused trainers: two ranks on half the lanes each, whose flat gradients are summed between `grad` and
`apply`, take the step one trainer on all the lanes takes.  Rehearsed on one GPU in one process, without a collective, a second rank or
a thread (tests/data_parallel.py: the sum is built by replay): a whole trainer on 514 lanes, and two shard trainers on 257 lanes each
with lane_offset 0 / 257, seed_stride 514, the same seed, world = hyper.world_size = 2.

Per case: (1) the first update's data of the shards are the whole's slices bit for bit; (2) counts and exactly representable sums in
the gradient's tail add up exactly; (3) every statistic computed from the tail agrees within the suite's bound for those sums,
1e-4 * max(1, |x|), while mean_reward and episodes, per rank by design, combine to the whole's as a mean and a sum; (4) the gradient
of the whole and the summed shard gradients divided by 2 are each within twice plain fp32 torch's error of the float64 gradient of the
same loss on the same data (the margin tests/test_gpu_a2c_fused.py allows the 7x7 gradient: summation order, not precision);
(5) after the last step the two shards are bit-identical, and within one step's bound of the whole: rtol 1e-4, atol 2e-6 for RMSprop
(test_fused_trainer_learns_and_matches_the_torch_trainer_step), 1 % of lr per Adam step for PPO
(test_trainer_update_is_the_torch_maths_on_its_records); the parameters moved by more than lr / 2.  Updates after the first start from
parameters that differ in the last bits, so nothing exact is asked of their data."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.data_parallel import record_gradients, rehearse  # noqa: E402

N = 514
SHAPED = dict(shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10, shaped_refresh_on_reset=True)
TAIL_STATS = ("loss", "policy_loss", "value_loss", "entropy", "grad_norm", "agreement", "live_fraction", "clip_fraction", "approx_kl",
              "mean_game_length", "finished_fraction", "first_mover_win_fraction")


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def bits(t):
    return t.contiguous().view(torch.uint8)


def rank_env(ea, S, n, lane_offset, warm=0, **kw):
    """lanes [lane_offset, lane_offset + n) of the N-lane run: global lane ids, the whole's seeds.  warm: launches of five steps under a
    fixed policy before the trainer gets the env -- no 7x7 game ends within the five steps of a first update, so without them the
    update's records would hold no terminal step and no reset (tests/test_gpu_shards.py holds this call to shard invariance)"""
    env = ea.VecEWN(n, board_size=S, rng="philox", autoreset=True, seed_stride=N, lane_offset=lane_offset, philox_key=9487, **kw)
    env.reset(seeds=(np.arange(lane_offset, lane_offset + n, dtype=np.uint64) + 9487).astype(np.uint32))
    if warm:
        from tests.test_gpu_policy import make_model
        params, traj = make_model(S, 5).flat_parameters(), env.alloc_rollout(5)
        for _ in range(warm):
            env.rollout_policy(5, params, traj=traj, noise_key=3)
    return env


def as_rank_of_two(tr):
    tr.world = 2
    tr.hyper.world_size = 2
    return tr


def rehearsal(ea, S, env_kw, make, updates, steps, first_data, reference, after_update=None):
    """make(env, whole) -> a trainer; first_data(tr) -> {name: (clone of a tensor of the first update's data, the lane's dimension)};
    reference(whole, params0) -> (g64, g32), the float64 and the plain fp32 torch gradient of the loss on the whole's first-update
    data, called before the second update overwrites them.  after_update(rank, tr): the case's hook after every update of a shard."""
    whole = make(rank_env(ea, S, N, 0, **env_kw), True)
    params0 = whole.params.clone()
    whole_grads = record_gradients(whole)
    whole.collect_and_update()
    torch.cuda.synchronize()
    out = SimpleNamespace(whole=whole, params0=params0, whole_grads=whole_grads, whole_data=first_data(whole), whole_stats=whole.stats_dict())
    out.g64, out.g32 = reference(whole, params0)
    for _ in range(updates - 1):
        whole.collect_and_update()

    def build():
        ranks = [as_rank_of_two(make(rank_env(ea, S, N // 2, lo, **env_kw), False)) for lo in (0, N // 2)]
        assert all(torch.equal(tr.params, params0) for tr in ranks)                     # the same seed: the same initial parameters
        return ranks

    def run(ranks):
        data, stats = [], []
        for r, tr in enumerate(ranks):
            for u in range(updates):
                tr.collect_and_update()
                if after_update is not None:
                    after_update(r, tr)
                if u == 0:
                    torch.cuda.synchronize()
                    data.append(first_data(tr))
                    stats.append(tr.stats_dict())
        return data, stats
    out.ranks, out.sums, (out.data, out.stats) = rehearse(build, run, steps)
    torch.cuda.synchronize()
    assert len(whole_grads) == steps == len(out.sums)
    return out


def check_first_data(out):
    for r, lo in enumerate((0, N // 2)):
        assert sorted(out.data[r]) == sorted(out.whole_data)
        for name, (t, dim) in out.data[r].items():
            want = out.whole_data[name][0].narrow(dim, lo, N // 2)
            assert t.shape == want.shape and torch.equal(bits(t), bits(want)), ("rank %d's first update" % r, name)


def check_stats(out, timesteps_slack=0):
    ws = out.whole_stats
    for r in range(2):
        st = out.stats[r]
        assert sorted(st) == sorted(ws)
        for k in st:
            if k in TAIL_STATS:
                assert abs(st[k] - ws[k]) <= 1e-4 * max(1.0, abs(ws[k])), (r, k, st[k], ws[k])
            else:
                assert k in ("mean_reward", "episodes"), k
    if "mean_reward" in ws:                                                           # per rank by design: they combine to the whole's
        assert abs((out.stats[0]["mean_reward"] + out.stats[1]["mean_reward"]) / 2 - ws["mean_reward"]) <= 1e-12 * max(1.0, abs(ws["mean_reward"]))
        assert out.stats[0]["episodes"] + out.stats[1]["episodes"] == ws["episodes"] > 0
    assert ws["grad_norm"] > 0
    for tr in out.ranks:
        assert abs(2 * tr.num_timesteps - out.whole.num_timesteps) <= timesteps_slack, (tr.num_timesteps, out.whole.num_timesteps)


def check_gradient(out, ctx):
    """-> the three relative L2 errors against float64: the whole's gradient, the summed shard gradients / 2, plain fp32 torch"""
    P = out.params0.numel()

    def rel(g):
        return float((g.double() - out.g64).norm() / out.g64.norm())
    e_whole, e_shards, e_torch = rel(out.whole_grads[0][:P]), rel(out.sums[0][:P].double() / 2), rel(out.g32)
    print("data parallel %s: relative L2 error of the gradient against float64: whole %.3g, summed shards / 2 %.3g, fp32 torch %.3g"
          % (ctx, e_whole, e_shards, e_torch))
    assert float(out.g64.norm()) > 0 and e_torch > 0
    assert e_whole <= 2 * e_torch, (ctx, e_whole, e_torch)
    assert e_shards <= 2 * e_torch, (ctx, e_shards, e_torch)
    return e_whole, e_shards, e_torch


def check_parameters(out, state, lr, close):
    a, b = out.ranks
    for name in ("params",) + state:
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name       # the same summed gradient, the same optimiser state
    close(a.params, out.whole.params)
    assert float((a.params - out.params0).abs().max()) > lr / 2 and float((out.whole.params - out.params0).abs().max()) > lr / 2


def rms_close(got, want):
    assert torch.allclose(got, want, rtol=1e-4, atol=2e-6), float((got - want).abs().max())


def rollout_data(tr):
    return {"record": (tr.traj["record"].clone(), 1), "reward": (tr.traj["reward"].clone(), 1)}


def torch_models(S, params0):
    from ewn_gym_amd.a2c import ActorCritic
    m32 = ActorCritic(S, 6).cuda()
    m32.load_flat_parameters(params0)
    return copy.deepcopy(m32).double(), m32


def flat_grad(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double()


# ---------------------------------------------------------------- A2C

def a2c_reference(S, K, gamma=0.99, vf_coef=0.5, ent_coef=0.0):
    """tests/test_gpu_a2c_fused.py::_errors_vs_float64's construction on the trainer's own records and hyper-parameters"""
    from ewn_gym_amd.a2c import n_step_returns

    def reference(whole, params0):
        traj = whole.traj
        obs_b, obs_d, n = traj["obs_board"], traj["obs_dice"], whole.env.N

        def torch_run(m, dt):
            with torch.no_grad():
                vals = torch.stack([m(obs_b[t], obs_d[t])[2] for t in range(K)])
                adv, ret = n_step_returns(traj["reward"].to(dt), vals, traj["terminated"].to(dt), m(obs_b[K], obs_d[K])[2], gamma, 1.0)
            logp, ent, value = m.evaluate_actions(obs_b[:K].reshape(K * n, S, S), obs_d[:K].reshape(K * n), traj["action"].reshape(K * n, 2))
            loss = -(adv.reshape(-1) * logp).mean() + vf_coef * torch.nn.functional.mse_loss(ret.reshape(-1), value) - ent_coef * ent.mean()
            loss.backward()
            return flat_grad(m)
        m64, m32 = torch_models(S, params0)
        return torch_run(m64, torch.float64), torch_run(m32, torch.float32)
    return reference


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("opponent", [None, "self"], ids=["minimax3", "self"])
def test_fused_a2c_two_ranks_take_the_whole_trainers_steps(ea, S, opponent):
    """FusedA2CTrainer, n_steps 5, two updates: against the shaped env's own depth-3 minimax opponent, and with opponent="self" (the
    rollout is ewn_step_k_selfplay with a sampling opponent: its noise word is keyed by the global lane too).  The local 1 / (K N)
    of ewn_a2c_grad and apply's division by world_size give the global mean.
    Measured relative L2 errors of the first gradient against float64 (MI355X; whole, summed shards / 2, plain fp32 torch):
      5x5 minimax3  2.12e-7, 2.09e-7, 4.92e-7      5x5 self  9.05e-8, 9.03e-8, 7.34e-7
      7x7 minimax3  1.03e-7, 1.00e-7, 4.50e-7      7x7 self  1.64e-7, 1.55e-7, 5.15e-7"""
    from ewn_gym_amd.a2c import FusedA2CTrainer
    K, lr = 5, 7e-4
    env_kw = dict(opponent_policy="minimax" if opponent is None else "random", max_depth=3, warm=4 if S == 7 else 0, **SHAPED)

    def make(env, whole):
        return FusedA2CTrainer(env, n_steps=K, learning_rate=lr, seed=1, use_graph=False, opponent=opponent, opponent_update_every=100)
    out = rehearsal(ea, S, env_kw, make, updates=2, steps=2, first_data=rollout_data, reference=a2c_reference(S, K))
    check_first_data(out)
    assert int(out.whole_data["record"][0][1:, :, S * S + 3].sum()) > 0                 # the first update's records hold terminations
    check_stats(out)
    check_gradient(out, "A2C %dx%d %s" % (S, S, opponent or "minimax3"))
    check_parameters(out, ("sq_avg",), lr, rms_close)
    if opponent == "self":
        assert all(torch.equal(tr.opp_params, out.params0) for tr in out.ranks + [out.whole])


# ---------------------------------------------------------------- PPO

def ppo_reference(S, K, clip, gamma=0.99, lam=0.95, vf_coef=0.5):
    from ewn_gym_amd.a2c import n_step_returns
    from ewn_gym_amd.ppo import PPOTrainer

    def reference(whole, params0):
        traj = whole.traj
        ob, od, n = traj["obs_board"], traj["obs_dice"], whole.env.N
        boards, dices, acts = ob[:K].reshape(K * n, S, S), od[:K].reshape(K * n), traj["action"].reshape(K * n, 2)

        def torch_run(m, dt):
            with torch.no_grad():                    # tests/test_gpu_ppo_fused.py::_torch_prepare in the model's dtype
                vals = torch.stack([m(ob[t], od[t])[2] for t in range(K)])
                adv, ret = n_step_returns(traj["reward"].to(dt), vals, traj["terminated"].to(dt), m(ob[K], od[K])[2], gamma, lam)
                logp = m.evaluate_actions(boards, dices, acts)[0]
            ns = SimpleNamespace(model=m, normalize_advantage=False, clip_range=clip, ent_coef=0.0, vf_coef=vf_coef)
            PPOTrainer.ppo_loss(ns, boards, dices, acts, logp, adv.reshape(-1), ret.reshape(-1))[0].backward()
            return flat_grad(m)
        m64, m32 = torch_models(S, params0)
        return torch_run(m64, torch.float64), torch_run(m32, torch.float32)
    return reference


def test_fused_ppo_two_ranks_take_the_whole_trainers_steps(ea):
    """FusedPPOTrainer, n_steps 4, normalize_advantage=False, n_epochs=2 and batch_size the whole batch (4 N for the whole, 4 N / 2 for a
    shard): one minibatch per epoch, hence two optimiser steps in the one update.  No other setting has a whole-run equivalent: the
    advantage normalisation is per rank by design (each rank takes the mean and deviation of its own minibatch), and with more than
    one minibatch every rank shuffles its own samples, so the union of the ranks' minibatches is no minibatch of the whole run.  The
    shuffle still orders the one minibatch differently on the whole and on a shard: only the summation order changes.
    clip_range is 0.005, not the default 0.2, so that the second step (the first has ratio 1 everywhere) clips some samples and the
    clipped count [P + 2], compared exactly, is not 0 == 0: one Adam step of 3e-4 moves the ratios by a fraction of a percent.
    Measured relative L2 errors of the first gradient against float64 (MI355X; whole, summed shards / 2, plain fp32 torch):
      5x5  1.29e-7, 1.28e-7, 5.94e-7; the second step clips 1 060 of the 2 056 samples, on the whole and on the shards together"""
    from ewn_gym_amd.ppo import FusedPPOTrainer
    S, K, lr, clip = 5, 4, 3e-4, 0.005
    env_kw = dict(opponent_policy="minimax", max_depth=3, **SHAPED)

    def make(env, whole):
        tr = FusedPPOTrainer(env, n_steps=K, batch_size=K * env.N, n_epochs=2, learning_rate=lr, clip_range=clip, normalize_advantage=False,
                             seed=3, use_graph=False)
        assert tr.n_minibatches == 1
        return tr
    out = rehearsal(ea, S, env_kw, make, updates=1, steps=2, first_data=rollout_data, reference=ppo_reference(S, K, clip))
    check_first_data(out)
    assert int(out.whole_data["record"][0][1:, :, S * S + 3].sum()) > 0
    P = out.params0.numel()
    clipped = [(float(s[P + 2]), float(g[P + 2])) for s, g in zip(out.sums, out.whole_grads)]
    print("data parallel PPO: clipped samples per step (summed shards, whole): %s of %d" % (clipped, K * N))
    assert clipped[0] == (0.0, 0.0) and clipped[1][0] == clipped[1][1] > 0, clipped
    check_stats(out)
    check_gradient(out, "PPO 5x5")
    assert all(int(tr.step) == 2 for tr in out.ranks + [out.whole])

    def close(got, want):
        assert float((got - want).abs().max()) <= 2 * 0.01 * lr, (float((got - want).abs().max()), lr)
    check_parameters(out, ("exp_avg", "exp_avg_sq", "step"), lr, close)


# ---------------------------------------------------------------- the supervised trainers

def sup_gradients(S, params0, b, d, tp, tv, w, pi_coef=1.0, vf_coef=0.5):
    from tests.test_gpu_sup_grad import torch_loss
    grads = []
    for m in torch_models(S, params0):
        torch_loss(m, b, d, tp, tv, w, pi_coef, vf_coef)[0].backward()
        grads.append(flat_grad(m))
    return grads


def check_exact_sums(out):
    """ewn_sup_grad's agreement count [P + 2] and weight sum [P + 3]: integers below 2^24, exact in fp32 in any order"""
    P = out.params0.numel()
    for i in (2, 3):
        got, want = float(out.sums[0][P + i]), float(out.whole_grads[0][P + i])
        assert got == want and want > 0 and want == int(want), (i, got, want)


def test_search_distill_two_ranks_take_the_whole_trainers_step(ea):
    """SearchDistillTrainer, search="lookahead", n_steps 3, one update.  ewn_sup_grad normalises by its own row count, 1 / M; with
    apply's division by world_size that is the mean over all ranks' rows.
    Measured relative L2 errors of the gradient against float64 (MI355X; whole, summed shards / 2, plain fp32 torch):
      5x5  1.53e-7, 1.47e-7, 5.28e-7"""
    from ewn_gym_amd.distill import SearchDistillTrainer
    S, K, lr = 5, 3, 7e-4
    env_kw = dict(opponent_policy="random", **SHAPED)

    def make(env, whole):
        return SearchDistillTrainer(env, n_steps=K, learning_rate=lr, search="lookahead", seed=5)

    def reference(whole, params0):
        _, q = ea.predict_lookahead(whole._boards, whole._dice, params0, terminal_value=1.0, return_q=True)
        tp, tv, w = ea.lookahead_targets(q, 0.0)
        return sup_gradients(S, params0, whole._boards, whole._dice, tp, tv, w)
    out = rehearsal(ea, S, env_kw, make, updates=1, steps=1, first_data=rollout_data, reference=reference)
    check_first_data(out)
    check_exact_sums(out)
    check_stats(out)
    check_gradient(out, "SearchDistill 5x5")
    check_parameters(out, ("sq_avg",), lr, rms_close)


@pytest.mark.parametrize("S", [5, 7])
def test_puct_selfplay_two_ranks_take_the_whole_trainers_step(ea, S, monkeypatch):
    """PuctSelfPlayTrainer as tests/test_gpu_puct_selfplay.py::selfplay_trainer builds it (sims 6, temp_plies 4, max_plies 16; 40 on 7x7), one
    update; distill.all_reduce_counters adds the other shard's counts, as that file patches it.  same_records on the games pins
    fresh_positions' seeds (counter x N x world + lane_offset), the global game number of the move's draw, and the root noise, which
    must belong to the global game as well (selfplay_noise).
    Measured relative L2 errors of the gradient against float64 (MI355X; whole, summed shards / 2, plain fp32 torch):
      5x5  1.09e-7, 1.07e-7, 8.08e-8      7x7  1.12e-7, 1.13e-7, 9.15e-8"""
    from ewn_gym_amd import distill
    from ewn_gym_amd.distill import PuctSelfPlayTrainer, both_flags_one_cube, puct_targets
    from tests.test_gpu_puct_selfplay import same_records
    T, lr = (16 if S == 5 else 40), 7e-4                                # no 7x7 game ends within 16 plies: its rows would all weigh nothing
    env_kw = dict(opponent_policy="random", **SHAPED)
    other = [torch.zeros(4, dtype=torch.int64, device="cuda")]          # what the counters' `all-reduce` adds: nothing for the whole
    monkeypatch.setattr(distill, "all_reduce_counters", lambda c: c + other[0])

    def make(env, whole):
        return PuctSelfPlayTrainer(env, sims=6, seed=5, temp_plies=4, max_plies=T, learning_rate=lr)

    def after_update(r, tr):
        """this rank's counts are what the rank that runs next adds: rank 1 now, rank 0 in the next pass (a rank's games are the same
        in every pass; only the first pass's rank 0 adds nothing, and that pass is thrown away)"""
        rec = tr.records
        other[0] = torch.stack([rec["live"].sum(), rec["plies"].sum(), (rec["winner"] != 0).sum(), (rec["winner"] == 1).sum()]).to(torch.int64)

    def reference(whole, params0):
        rec, R = whole.records, T * N
        b, d = rec["board"].reshape(R, S, S), rec["dice"].reshape(R).clamp(min=1)
        tp, _, _ = puct_targets(rec["visits"].reshape(R, 2, 3), None, rec["value"].reshape(R), 1.0, one_cube=both_flags_one_cube(b, d))
        return sup_gradients(S, params0, b, d, tp, rec["z"].reshape(R).contiguous(), rec["weight"].reshape(R).contiguous())

    def games(tr):
        return {k: (v.clone(), 0 if v.dim() == 1 else 1) for k, v in tr.records.items()}
    out = rehearsal(ea, S, env_kw, make, updates=1, steps=1, first_data=games, reference=reference, after_update=after_update)
    whole_rec = {k: t for k, (t, _) in out.whole_data.items()}
    same_records({k: torch.cat([out.data[0][k][0], out.data[1][k][0]], out.whole_data[k][1]) for k in whole_rec}, whole_rec)
    assert 0 < float(whole_rec["weight"].sum()) <= float(whole_rec["live"].sum()) < T * N   # some games ended: their rows weigh
    assert S == 7 or float(whole_rec["weight"].sum()) < float(whole_rec["live"].sum())      # 16 plies leave 5x5 games unfinished too
    check_exact_sums(out)
    check_stats(out, timesteps_slack=1)
    assert all(tr.seed_counter == 1 for tr in out.ranks + [out.whole])
    check_gradient(out, "PuctSelfPlay %dx%d" % (S, S))
    check_parameters(out, ("sq_avg",), lr, rms_close)
