"""Wall time of the four tournament cells with an MCTS agent, or a minimax agent against MCTS (eval_pairs.py:10-35's matrix), on both
paths -- in the engine (ewn_step_k_agent, `chunk` steps per launch) and per step (predict_mcts / predict_minimax + ewn_step per ply).

    python tools/tournament_time.py [--board_size 5] [--nums 1024] [--reps 5] [--big 65536]

Default shape: 5x5, minimax max_depth 5 ('hybrid'), MCTS(10 x 5), MT19937-compat dice, seeds 0..n-1.  --big N adds MCTS vs MCTS at N
episodes (0: skip).  One JSON line per (cell, path, episodes): median of --reps calls, after one warm-up call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ewn_gym_amd.tournament import evaluate  # noqa: E402


def timed(agent, opp, num, S, use_rollout, reps):
    evaluate(agent, opp, num=num, board_size=S, use_rollout=use_rollout)      # warm-up: kernels, allocator
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = evaluate(agent, opp, num=num, board_size=S, use_rollout=use_rollout)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board_size", type=int, default=5)
    ap.add_argument("--nums", type=int, nargs="+", default=[1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max_depth", type=int, default=5)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--big_reps", type=int, default=3)
    a = ap.parse_args()
    S = a.board_size
    spec = {"random": {"kind": "random"}, "minimax": {"kind": "minimax", "max_depth": a.max_depth, "heuristic": "hybrid"},
            "mcts": {"kind": "mcts", "num_simulations": 10, "num_env_copies": 5}}
    cells = [("mcts", "random"), ("mcts", "minimax"), ("mcts", "mcts"), ("minimax", "mcts")]
    runs = [(c, n, a.reps) for n in a.nums for c in cells]
    if a.big:
        runs.append((("mcts", "mcts"), a.big, a.big_reps))
    for (ag, op), num, reps in runs:
        row = {}
        for use_rollout in (True, False):
            ts, r = timed(spec[ag], spec[op], num, S, use_rollout, reps)
            row[r["engine"]] = r
            print(json.dumps({"cell": "%s vs %s" % (ag, op), "path": r["engine"], "episodes": num, "board_size": S,
                              "median_s": ts[len(ts) // 2], "min_s": ts[0], "win_rate": r["win_rate"],
                              "avg_length": r["avg_length"]}), flush=True)
        e, p = row["ewn_step_k_agent"], row["ewn_step"]
        assert torch.equal(e["scores"].view(torch.int64), p["scores"].view(torch.int64)) and torch.equal(e["lengths"], p["lengths"])


if __name__ == "__main__":
    main()
