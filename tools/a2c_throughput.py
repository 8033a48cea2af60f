"""Throughput of the on-device A2C loop (BASELINE config 4 on one GPU): shaped env, depth-3 minimax opponent, n_steps 5.
   python tools/a2c_throughput.py [--algorithm A2C|PPO] [--trainer fused|torch|both] [--lanes 65536] [--updates 200]
fused: ewn_step_k_policy + ewn_a2c_grad + ewn_a2c_apply (five kernel launches per update, one hipGraph replay);
torch: the round-2 loop (torch policy forward per step + ewn_step, torch autograd update).
--algorithm PPO: FusedPPOTrainer against PPOTrainer at their defaults (10 epochs x 4 minibatches) with the same n_steps.
--opponent random | minimax | self: the env's opponent; self = the fused trainers' opponent="self" (ewn_step_k_selfplay; fused only).
--rollout-only: no update, only the trainer's rollout call (records + reward column, sampled actions, K = n-steps per launch) against
RandomAgent, minimax(3) and a second parameter vector, in one process: time per env step of the three k_rollout_mlp instances."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import A2CTrainer, FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.ppo import FusedPPOTrainer, PPOTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--algorithm", default="A2C", choices=["A2C", "PPO"])
ap.add_argument("--trainer", default="both", choices=["fused", "torch", "both"])
ap.add_argument("--lanes", type=int, nargs="*", default=[4096, 65536])
ap.add_argument("--updates", type=int, default=200)
ap.add_argument("--n-steps", type=int, default=5)
ap.add_argument("--opponent", default="minimax", choices=["random", "minimax", "self"])
ap.add_argument("--rollout-only", action="store_true")
ap.add_argument("--board_size", type=int, default=5)
a = ap.parse_args()
S = a.board_size


def make_env(N, opp):
    env = ea.VecEWN(N, board_size=S, opponent_policy="random" if opp == "self" else opp, max_depth=3, rng="philox", shaped=True, reward=10.0,
                    illegal_move_reward=-1.0, illegal_move_tolerance=10, autoreset=True, shaped_refresh_on_reset=True, philox_key=1)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    return env


if a.rollout_only:
    from ewn_gym_amd.a2c import ActorCritic
    K = a.n_steps
    for N in a.lanes:
        torch.manual_seed(0)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        other = ActorCritic(S, 6).cuda().flat_parameters()
        for opp in ("random", "minimax", "self"):
            env = make_env(N, opp)
            traj = env.alloc_rollout(K, layout="record", initial_obs=True)
            kw = dict(opponent_params=other, opponent_noise_key=5) if opp == "self" else {}
            for _ in range(10):
                env.rollout_policy(K, params, traj=traj, noise_key=3, **kw)
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(a.updates):
                    env.rollout_policy(K, params, traj=traj, noise_key=3, **kw)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / (a.updates * K))
            ts.sort()
            print("rollout %dx%d N=%d opponent %s: %.2f us per env step (median of 5; min %.2f, max %.2f), %.3e env steps/s" %
                  (S, S, N, {"random": "RandomAgent", "minimax": "minimax(3)", "self": "policy"}[opp], ts[2] * 1e6, ts[0] * 1e6, ts[-1] * 1e6,
                   N / ts[2]), flush=True)
    sys.exit(0)
for kind in (("fused", "torch") if a.trainer == "both" else (a.trainer,)):
    for N in a.lanes:
        if a.opponent == "self" and kind != "fused":
            continue            # the torch trainers step the env with ewn_step: no policy opponent
        env = make_env(N, a.opponent)
        if a.algorithm == "PPO":
            cls = FusedPPOTrainer if kind == "fused" else PPOTrainer
        else:
            cls = FusedA2CTrainer if kind == "fused" else A2CTrainer
        okw = dict(opponent="self") if a.opponent == "self" else {}
        tr = cls(env, n_steps=a.n_steps, learning_rate=3e-4, seed=0, **okw)
        n_upd = a.updates if kind == "fused" else max(10, a.updates // 5)
        if a.algorithm == "PPO":   # forty optimiser steps per update
            n_upd = max(5, n_upd // 10)
        for _ in range(5):
            tr.collect_and_update()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n0 = tr.num_timesteps
        for _ in range(n_upd):
            st = tr.collect_and_update()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        sd = tr.stats_dict() if kind == "fused" else tr.stats_dict(st)
        print("%s %s opponent %s N=%d: %.3e env steps/s (%.3f ms per %d-step update), mean reward %.3f" %
              (a.algorithm, kind, a.opponent, N, (tr.num_timesteps - n0) / dt, dt / n_upd * 1e3, a.n_steps, sd["mean_reward"]), flush=True)
