"""The playout tree search with and without an endgame table at the leaves: time, leaf counts, and how it plays.

  python tools/playout_exact_time.py [--runs 5] [--launches 20] [--sims 64] [--playouts 64] [--batches 1 1024 16384] [--num 1024]
                                     [--skip_timing] [--skip_play]

Part 1, per board (5x5 with the (5, 2, 4) table, 7x7 with the (7, 2, 3) table), batch and kind of observation: playout_search and
playout_search_exact on the same observations, alternated in one process.  "random play": observations of a random-agent rollout,
where next to no leaf is covered, so the difference is what the coverage test costs.  "few cubes": sampled positions with two or three
cubes a side, half of them covered at the root and half just outside.  Each figure is the median (min, max) of `--runs` timed
windows after warm-up, a window being `--launches` back-to-back calls between two device events with a synchronisation before and
after; microseconds per call.  Beside them the leaves the table valued, the leaves playouts valued, and the table's share.

Part 2, 5x5: wins of `--num` episodes of {"kind": "playout_search"} with and without the (5, 2, 4) table against random,
mcts(10 x 5) and minimax(5), on the same episodes.
Prints one JSON line per row.  No pass bar."""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402

TABLES = {5: (2, 4), 7: (2, 3)}
FEW = {5: [(2, 2), (1, 2), (3, 2), (2, 3)], 7: [(1, 2), (2, 1), (2, 2), (2, 2)]}   # (own, opposing) cubes: half covered, half just outside


def few_cubes(S, M, seed=1):
    """M live positions with FEW[S]'s cube counts in turn, distinct random numbers and cells, and random dice; up to 4 096 distinct ones"""
    rng = random.Random(seed)
    N, C = min(M, 4096), S * S
    b = np.zeros((N, C), np.int8)
    for i in range(N):
        ka, ko = FEW[S][i % 4]
        while True:
            cells = rng.sample(range(C), ka + ko)
            if C - 1 not in cells[:ka] and 0 not in cells[ka:]:
                break
        b[i, cells[:ka]] = rng.sample(range(1, 7), ka)
        b[i, cells[ka:]] = [-k for k in rng.sample(range(1, 7), ko)]
    d = np.array([rng.randint(1, 6) for _ in range(N)], np.int8)
    idx = torch.arange(M, device="cuda") % N
    return torch.as_tensor(b.reshape(N, S, S)).cuda()[idx].contiguous(), torch.as_tensor(d).cuda()[idx].contiguous()


def part1(runs, launches, sims, n, batches):
    for S in (5, 7):
        table = ea.EndgameTable.build(S, *TABLES[S])
        for M in batches:
            for kind, (b, d) in (("random play", observations(S, M)), ("few cubes", few_cubes(S, M))):
                fns = {"playout_search": lambda: ea.playout_search(b, d, sims, playouts=n),
                       "playout_search_exact": lambda: ea.playout_search_exact(b, d, sims, table, playouts=n)}
                plain = fns["playout_search"]()
                exact, counts = ea.playout_search_exact(b, d, sims, table, playouts=n, return_leaf_counts=True)   # the warm-up of both
                by_table, by_playouts = (int(x) for x in counts.sum(0))
                rows = {}
                for _ in range(2):                                             # alternate them, keep the later pass
                    for name, fn in fns.items():
                        rows[name] = timed(fn, launches, runs)
                print(json.dumps({"board": S, "table": [S, *TABLES[S]], "M": M, "observations": kind, "sims": sims, "playouts": n,
                                  "launches": launches, "leaves_by_table": by_table, "leaves_by_playouts": by_playouts,
                                  "table_share": round(by_table / max(1, by_table + by_playouts), 4),
                                  "same_trees_as_without": torch.equal(plain, exact), "us_per_call_median_min_max": rows,
                                  "exact_over_plain": round(rows["playout_search_exact"][0] / rows["playout_search"][0], 3)}), flush=True)


def part2(num, sims, n):
    table = ea.EndgameTable.build(5, *TABLES[5])
    agents = [("playout_search(%d x %d)" % (sims, n), {"kind": "playout_search", "sims": sims, "playouts": n}),
              ("playout_search(%d x %d) + table(5, 2, 4)" % (sims, n), {"kind": "playout_search", "sims": sims, "playouts": n, "endgame_table": table})]
    for name, opp in (("random", {"kind": "random"}), ("mcts(10 x 5)", {"kind": "mcts", "num_simulations": 10, "num_env_copies": 5}),
                      ("minimax(5)", {"kind": "minimax", "max_depth": 5})):
        for label, spec in agents:
            r = evaluate(spec, opp, num=num)
            print(json.dumps({"agent": label, "opponent": name, "wins": r["wins"], "episodes": r["episodes"], "ci95": [round(x, 3) for x in r["ci95"]],
                              "avg_length": round(r["avg_length"], 2), "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024, 16384])
    ap.add_argument("--num", type=int, default=1024)
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_play", action="store_true")
    a = ap.parse_args()
    if not a.skip_timing:
        part1(a.runs, a.launches, a.sims, a.playouts, a.batches)
    if not a.skip_play:
        part2(a.num, a.sims, a.playouts)


if __name__ == "__main__":
    main()
