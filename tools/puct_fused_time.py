"""The PUCT search in one launch beside the staged search.

  python tools/puct_fused_time.py [--runs 5] [--sims 16 64 256] [--batches 1 32 1024 4096 16384] [--tiles 1 4 8 16 32] [--skip_selfplay]

Part 1, per board (5x5, 7x7), batch and budget: predict_puct (actions only, one chunk of M observations) staged and with fused=True
on the same observations, alternated in one process.  Each figure is the median (min, max) of `--runs` timed windows after warm-up,
a window being `launches` back-to-back calls between two device events with a synchronisation before and after; microseconds per
call, and the staged median over the fused one.  The staged figures at M = 1 and 1 024, 64 simulations, 5x5 are 4o's: the cross-check
that a run is sound.

Part 2, 5x5 and 7x7, 64 simulations: the fused search alone under each forced tile size (EWN_PUCT_TILE) at every batch the tile
choice matters for, beside the default choice.

Part 3: recorded positions per second of selfplay_puct, staged and fused, at M = 1 024 and 4 096 openings with 64 simulations
(tools/selfplay_time.py's windows).
Prints one JSON line per row.  No pass bar."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402
from tools.selfplay_time import openings, window  # noqa: E402


def launches_for(M, sims):
    """about a quarter of a second of staged work per window at the least, two calls at the most expensive shapes"""
    return max(2, min(200, 12000 // ((sims + 1) * max(1, M // 1024))))


def part1(runs, budgets, batches):
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in batches:
            b, d = observations(S, M)
            for sims in budgets:
                fns = {"staged": lambda: ea.predict_puct(b, d, params, sims=sims, chunk=M),
                       "fused": lambda: ea.predict_puct(b, d, params, sims=sims, chunk=M, fused=True)}
                assert torch.equal(fns["staged"](), fns["fused"]())
                n = launches_for(M, sims)
                for fn in fns.values():                                    # warm-up
                    for _ in range(2):
                        fn()
                rows = {}
                for _ in range(2):                                         # alternate them, keep the later pass
                    for name, fn in fns.items():
                        rows[name] = timed(fn, n, runs)
                print(json.dumps({"board": S, "M": M, "sims": sims, "launches": n, "us_per_call_median_min_max": rows,
                                  "staged_over_fused": round(rows["staged"][0] / rows["fused"][0], 2)}), flush=True)


def part2(runs, batches, tiles, sims=64):
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in batches:
            b, d = observations(S, M)
            fn = lambda: ea.predict_puct(b, d, params, sims=sims, chunk=M, fused=True)   # noqa: E731
            n = launches_for(M, sims)
            rows = {}
            for tile in [None] + [t for t in tiles if (t * 256 >= M or t == 32) and (t <= M or t == 1)]:   # a smaller tile only adds trips
                if tile is None:
                    os.environ.pop("EWN_PUCT_TILE", None)
                else:
                    os.environ["EWN_PUCT_TILE"] = str(tile)
                fn()
                rows["default" if tile is None else "tile %d" % tile] = timed(fn, n, runs)
            os.environ.pop("EWN_PUCT_TILE", None)
            print(json.dumps({"board": S, "M": M, "sims": sims, "fused_us_per_call_median_min_max": rows}), flush=True)


def part3(runs, sims=64):
    cases = {}
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in (1024, 4096):
            b, d = openings(S, M)
            for fused in (False, True):
                cases[(S, M, fused)] = lambda b=b, d=d, params=params, fused=fused: ea.selfplay_puct(b, d, params, sims=sims, key=3, fused=fused)
    rates = {k: [] for k in cases}
    for k, fn in cases.items():                                            # warm-up
        window(fn)
    for _ in range(runs):                                                  # alternated
        for k, fn in cases.items():
            s, n = window(fn)
            rates[k].append((n / s, n, s))
    for (S, M, fused), r in rates.items():
        pps = [x[0] for x in r]
        print(json.dumps({"board": S, "M": M, "sims": sims, "fused": fused,
                          "positions_per_s_median_min_max": [round(statistics.median(pps)), round(min(pps)), round(max(pps))],
                          "positions_per_call": r[0][1], "seconds_per_call_median": round(statistics.median(x[2] for x in r), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sims", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 1024, 4096, 16384])
    ap.add_argument("--tiles", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_tiles", action="store_true")
    ap.add_argument("--skip_selfplay", action="store_true")
    a = ap.parse_args()
    if not a.skip_timing:
        part1(a.runs, a.sims, a.batches)
    if not a.skip_tiles:
        part2(a.runs, a.batches, a.tiles)
    if not a.skip_selfplay:
        part3(a.runs)


if __name__ == "__main__":
    main()
