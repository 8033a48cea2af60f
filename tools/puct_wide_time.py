"""The PUCT search in one launch with several leaves per tree and round beside puct_search, and what the leaves cost in playing
strength.

  python tools/puct_wide_time.py [--runs 5] [--sims 64 256] [--batches 1 1024 4096 16384] [--leaves 1 2 4 8 16 32] [--num 1024]
                                 [--model best.pt] [--skip_timing] [--skip_play] [--out profiles/puct_wide/puct_wide_time.txt]

Part 1, per board (5x5, 7x7), batch and budget: puct_search (ewn_puct_search, the yardstick: one leaf per tree and round) and
puct_search_wide at every L of --leaves into preallocated trees on the same observations, alternated in one process.  Each figure
is the median (min, max) of `--runs` timed windows after a warm-up, a window being `launches` back-to-back calls between two device
events with a synchronisation before and after; microseconds per call, and puct_search's median over each L's.  "one_leaf_same"
says whether L = 1 left puct_search's trees in the warm-up call (tests/test_gpu_puct_wide.py asserts it); "below" lists the L whose
whole min - max range lies below puct_search's.

Part 2, 5x5: wins of `--num` episodes of {"kind": "mlp_puct", "leaves": L} against minimax(5) with Wilson 95 % intervals, for L in
{1, 4, 8, 32} at each budget of --sims, on the same episodes (the tournament's seeds).  --model: a checkpoint of any of the trainers;
without it the network is a freshly initialised one (seed 9) and the rows say so.
Prints one JSON line per row and writes the same lines to --out.  No pass bar."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402
from ewn_gym_amd.tournament import evaluate, load_policy  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402


def launches_for(M, sims):
    """about a tenth of a second of puct_search per window at the least, two calls at the most expensive shapes"""
    return max(2, min(200, 12000 // ((sims + 1) * max(1, M // 1024))))


def part1(runs, budgets, batches, leaves, emit):
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in batches:
            b, d = observations(S, M)
            for sims in budgets:
                tree, wide = ea.puct_search(b, d, params, sims), ea.puct_search(b, d, params, sims)
                fns = {"puct_search": lambda: ea.puct_search(b, d, params, sims, out=tree)}
                for L in leaves:
                    fns["L=%d" % L] = lambda L=L: ea.puct_search_wide(b, d, params, sims, L, out=wide)
                same = None
                if 1 in leaves:
                    same = torch.equal(fns["L=1"](), fns["puct_search"]())
                n = launches_for(M, sims)
                for fn in fns.values():                                    # warm-up
                    for _ in range(2):
                        fn()
                rows = {}
                for _ in range(2):                                         # alternate them, keep the later pass
                    for name, fn in fns.items():
                        rows[name] = timed(fn, n, runs)
                base = rows["puct_search"]
                emit({"board": S, "M": M, "sims": sims, "launches": n, "one_leaf_same": same, "us_per_call_median_min_max": rows,
                      "puct_search_over": {k: round(base[0] / v[0], 2) for k, v in rows.items() if k != "puct_search"},
                      "below": [k for k, v in rows.items() if k != "puct_search" and v[2] < base[1]]})


def part2(num, budgets, model, emit):
    if model is not None:
        net, which = load_policy(model, 5, 3), os.path.basename(model)
    else:
        torch.manual_seed(9)
        net, which = ActorCritic(5, 6).cuda(), "a freshly initialised network (seed 9): no checkpoint given"
    for sims in budgets:
        for L in (1, 4, 8, 32):
            r = evaluate({"kind": "mlp_puct", "model": net, "sims": sims, "fused": True, "leaves": L}, {"kind": "minimax", "max_depth": 5}, num=num)
            emit({"agent": "puct(%d), leaves %d" % (sims, L), "network": which, "opponent": "minimax(5)", "wins": r["wins"],
                  "episodes": r["episodes"], "ci95": [round(x, 3) for x in r["ci95"]], "avg_length": round(r["avg_length"], 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024, 4096, 16384])
    ap.add_argument("--leaves", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--num", type=int, default=1024)
    ap.add_argument("--model", default=None)
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_play", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "puct_wide",
                                                  "puct_wide_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/puct_wide_time.py measures on the GPU and found none")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if not a.skip_timing:
            part1(a.runs, a.sims, a.batches, a.leaves, emit)
        if not a.skip_play:
            part2(a.num, a.sims, a.model, emit)


if __name__ == "__main__":
    main()
