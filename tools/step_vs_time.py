"""Timing of the model-opponent step calls.

  python tools/step_vs_time.py [--reps 5]

Per board (5x5, 7x7) and lane count (1 024, 65 536), device-event time per env step of
  step() against a model (ewn_step_vs),  the K-step call at K = 16 per step (ewn_step_k_vs, sample agent, no trajectory),
  and ewn_step with the minimax(3) opponent, alternated in the same process;
then tournament.evaluate_vs_model over 1 024 episodes for the random and minimax(5) agents, K steps per launch against ply by ply.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd import tournament  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402


def model(S, seed):
    torch.manual_seed(seed)
    m = ActorCritic(S, 6).cuda()
    with torch.no_grad():
        m.action_net.weight.mul_(300.0)
    return m


def timed(fn, launches, steps_per_launch, reps):
    """median, min, max of `reps` windows of `launches` calls: microseconds of device time per env step"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / (launches * steps_per_launch))
    return [round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for S in (5, 7):
        po = model(S, 9).flat_parameters()
        for N in (1024, 65536):
            seeds = (np.arange(N, dtype=np.uint64) + 9487).astype(np.uint32)
            kw = dict(board_size=S, rng="philox", autoreset=True, seed_stride=N, philox_key=7)
            vs = ea.VecEWN(N, opponent_policy="random", **kw)
            mm = ea.VecEWN(N, opponent_policy="minimax", max_depth=3, **kw)
            for e in (vs, mm):
                e.reset(seeds=seeds)
            vs.set_opponent_model(po)
            act = torch.zeros((N, 2), dtype=torch.int8, device="cuda")   # [0, 0]: mostly legal, auto-reset keeps every lane playing
            launches = 200 if N <= 8192 else 100
            for fn in (lambda: vs.step(act), lambda: mm.step(act), lambda: vs.rollout(16, agent="sample")):   # warm-up
                for _ in range(10):
                    fn()
            rows = {}
            for _ in range(2):                                            # alternate the three, keep the later pass
                rows["ewn_step_vs"] = timed(lambda: vs.step(act), launches, 1, a.reps)
                rows["ewn_step minimax(3)"] = timed(lambda: mm.step(act), launches, 1, a.reps)
                rows["ewn_step_k_vs K=16 sample"] = timed(lambda: vs.rollout(16, agent="sample"), launches // 4, 16, a.reps)
            print(json.dumps({"board": S, "lanes": N, "us_per_env_step_median_min_max": rows}), flush=True)
    opp = {"kind": "mlp", "model": model(5, 9)}
    for agent in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
        for use_rollout in (True, False):
            tournament.evaluate_vs_model(agent, opp, num=1024, use_rollout=use_rollout)      # warm-up
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = tournament.evaluate_vs_model(agent, opp, num=1024, use_rollout=use_rollout)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1000.0)
            print(json.dumps({"evaluate_vs_model": agent, "engine": r["engine"], "episodes": 1024, "win_rate": r["win_rate"],
                              "avg_length": r["avg_length"],
                              "wall_ms_median_min_max": [round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)]}), flush=True)


if __name__ == "__main__":
    main()
