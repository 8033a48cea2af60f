"""Wall time of the trainer's per-epoch evaluation (train.py:66-117): a trained policy's argmax vs minimax(5), MT19937-compat dice,
seeds 0..n-1, on both paths -- in the engine (ewn_policy_eval, K steps per launch) and per step (model.act + ewn_step per ply).

    python tools/eval_policy_time.py [--board_size 5] [--nums 256 1024] [--reps 5]

The policy is a FusedA2CTrainer trained briefly against RandomAgent (an untrained one forfeits at its first move).  EWN_EVAL_NT=64 / 256
in the environment forces the evaluation kernel's block size.  One JSON line per (path, episodes): median of --reps calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board_size", type=int, default=5)
    ap.add_argument("--nums", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--max_depth", type=int, default=5)
    a = ap.parse_args()
    S, N = a.board_size, 4096
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=10,
                    autoreset=True, shaped_refresh_on_reset=True, philox_key=1)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    tr = FusedA2CTrainer(env, n_steps=5, learning_rate=1e-3, seed=0)
    for _ in range(a.updates):
        tr.collect_and_update()
    torch.cuda.synchronize()
    opp = {"kind": "minimax", "max_depth": a.max_depth}
    paths = (("ewn_policy_eval", {"kind": "mlp", "model": tr.model}), ("ewn_step", tr.policy_fn(True)))
    for num in a.nums:
        for name, agent in paths:
            evaluate(agent, opp, num=num, board_size=S)                 # warm-up: tables, kernels, allocator
            ts, r = [], None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = evaluate(agent, opp, num=num, board_size=S)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert r["engine"] == name, (r["engine"], name)
            ts.sort()
            print(json.dumps({"path": name, "episodes": num, "board_size": S, "opponent_depth": a.max_depth,
                              "eval_nt": os.environ.get("EWN_EVAL_NT", "auto"), "median_s": ts[len(ts) // 2], "min_s": ts[0],
                              "win_rate": r["win_rate"], "avg_length": r["avg_length"]}), flush=True)


if __name__ == "__main__":
    main()
