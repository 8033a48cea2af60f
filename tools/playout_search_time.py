"""The playout-valued PUCT search in one launch beside its staged composition, and how it plays.

  python tools/playout_search_time.py [--runs 5] [--sims 64] [--playouts 64] [--batches 1 1024 16384] [--num 1024] [--model best.pt]
                                      [--skip_timing] [--skip_play]

Part 1, per board (5x5, 7x7) and batch: playout_search (one launch) and the staged composition through the public calls --
puct_begin, then per round playout_wins on the leaf rows, the value in torch on the device and puct_advance with zero logits -- on
the same observations, alternated in one process.  Each figure is the median (min, max) of `--runs` timed windows after warm-up,
a window being `launches` back-to-back calls between two device events with a synchronisation before and after; microseconds per
call, and the staged median over the one-launch one.  "same_trees" says whether the two left the same bytes in the warm-up call.

Part 2, 5x5: wins of `--num` episodes of {"kind": "playout_search"} against random, mcts(10 x 5) and minimax(5); with --model (a
checkpoint of any of the trainers) predict_puct of the same budget on that network beside them.
Prints one JSON line per row.  No pass bar."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.tournament import evaluate, load_policy  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402

KEY_STEP = 0x9E3779B97F4A7C15


def staged(b, d, sims, n, key=0):
    """the composition of the definition; a tree without a pending leaf shows a zero board, whose wins are not read"""
    M = b.shape[0]
    tree, lb, ld = ea.puct_begin(b, d, sims)
    zeros, nf = torch.zeros((M, 5), dtype=torch.float32, device="cuda"), torch.full((M,), float(n), dtype=torch.float32, device="cuda")
    for r in range(sims + 1):
        w = ea.playout_wins(lb, 1, n, key=(key + r * KEY_STEP) & 0xFFFFFFFFFFFFFFFF)
        ea.puct_advance(tree, zeros, (2 * w - n).to(torch.float32) / nf, lb, ld, sims, terminal_value=1.0)
    return tree


def part1(runs, sims, n, batches):
    for S in (5, 7):
        for M in batches:
            b, d = observations(S, M)
            fns = {"staged": lambda: staged(b, d, sims, n), "one_launch": lambda: ea.playout_search(b, d, sims, playouts=n)}
            same = torch.equal(fns["staged"](), fns["one_launch"]())              # the warm-up of both; tests/test_gpu_playout_search.py asserts it
            launches = max(2, min(50, 2048 // M))
            rows = {}
            for _ in range(2):                                                 # alternate them, keep the later pass
                for name, fn in fns.items():
                    rows[name] = timed(fn, launches, runs)
            print(json.dumps({"board": S, "M": M, "sims": sims, "playouts": n, "launches": launches, "same_trees": same, "us_per_call_median_min_max": rows,
                              "staged_over_one_launch": round(rows["staged"][0] / rows["one_launch"][0], 2)}), flush=True)


def part2(num, sims, n, model):
    agents = [("playout_search(%d x %d)" % (sims, n), {"kind": "playout_search", "sims": sims, "playouts": n})]
    if model is not None:
        agents.append(("puct(%d)" % sims, {"kind": "mlp_puct", "model": load_policy(model, 5, 3), "sims": sims, "fused": True}))
    else:
        print(json.dumps({"note": "no --model given: the rows of predict_puct on a trained network are left out"}), flush=True)
    for name, opp in (("random", {"kind": "random"}), ("mcts(10 x 5)", {"kind": "mcts", "num_simulations": 10, "num_env_copies": 5}),
                      ("minimax(5)", {"kind": "minimax", "max_depth": 5})):
        for label, spec in agents:
            r = evaluate(spec, opp, num=num)
            print(json.dumps({"agent": label, "opponent": name, "wins": r["wins"], "episodes": r["episodes"], "ci95": [round(x, 3) for x in r["ci95"]],
                              "avg_length": round(r["avg_length"], 2), "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024, 16384])
    ap.add_argument("--num", type=int, default=1024)
    ap.add_argument("--model", default=None)
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_play", action="store_true")
    a = ap.parse_args()
    if not a.skip_timing:
        part1(a.runs, a.sims, a.playouts, a.batches)
    if not a.skip_play:
        part2(a.num, a.sims, a.playouts, a.model)


if __name__ == "__main__":
    main()
