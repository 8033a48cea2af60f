"""The one-launch PUCT search with and without an endgame table at the leaves, and the staged search it replaces: time and leaf
counts.

  python tools/puct_exact_time.py [--runs 5] [--launches 20] [--sims 64] [--batches 1 1024 16384] [--skip_random] [--skip_few]
                                  [--plain LABEL]

Per board (5x5 with the (5, 2, 4) table, 7x7 with the (7, 2, 3) table) and batch, on a freshly initialised actor-critic (seed 9):
"random play": observations of a random-agent rollout, where next to no leaf is covered: puct_search and puct_search_exact on the
same observations, alternated in one process, so the difference is what the coverage test costs.
"few cubes": tools/playout_exact_time.py's sampled positions, half covered at the root and half just outside:
predict_puct(leaf_table=), the one launch per chunk, against predict_puct(endgame_table=), the staged path it replaces, alternated.
--plain LABEL: puct_search alone on the random-play observations, rows tagged LABEL: run once per library (EWN_HIP_LIB) to compare
two builds, a process each.
Each figure is the median (min, max) of `--runs` timed windows after warm-up, a window being back-to-back calls between two device
events with a synchronisation before and after (`--launches` of them up to 8 192 observations, in proportion fewer above, never under 2);
microseconds per call.  Prints one JSON line per row.  No pass bar."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402
from tools.playout_exact_time import TABLES, few_cubes  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402


def params_of(S):
    torch.manual_seed(9)
    return ActorCritic(S, 6).cuda().flat_parameters()


def launches_for(M, launches):
    return max(2, launches * 8192 // max(M, 8192))


def alternated(fns, launches, runs):
    rows = {}
    for _ in range(2):                                         # alternate them, keep the later pass
        for name, fn in fns.items():
            rows[name] = timed(fn, launches, runs)
    return rows


def random_play(runs, launches, sims, batches):
    for S in (5, 7):
        table, params = ea.EndgameTable.build(S, *TABLES[S]), params_of(S)
        for M in batches:
            b, d = observations(S, M)
            n = launches_for(M, launches)
            fns = {"puct_search": lambda: ea.puct_search(b, d, params, sims),
                   "puct_search_exact": lambda: ea.puct_search_exact(b, d, params, sims, table)}
            plain = fns["puct_search"]()
            exact, counts = ea.puct_search_exact(b, d, params, sims, table, return_leaf_counts=True)   # the warm-up of both
            by_table, by_value = (int(x) for x in counts.sum(0))
            rows = alternated(fns, n, runs)
            print(json.dumps({"board": S, "table": [S, *TABLES[S]], "M": M, "observations": "random play", "sims": sims, "launches": n,
                              "leaves_by_table": by_table, "leaves_by_value_head": by_value,
                              "table_share": round(by_table / max(1, by_table + by_value), 4), "same_trees_as_without": torch.equal(plain, exact),
                              "us_per_call_median_min_max": rows,
                              "exact_over_plain": round(rows["puct_search_exact"][0] / rows["puct_search"][0], 3)}), flush=True)


def few(runs, launches, sims, batches):
    for S in (5, 7):
        table, params = ea.EndgameTable.build(S, *TABLES[S]), params_of(S)
        for M in batches:
            b, d = few_cubes(S, M)
            n = launches_for(M, launches)
            kw = dict(sims=sims, return_visits=True, return_value=True)
            fns = {"predict_puct(leaf_table=)": lambda: ea.predict_puct(b, d, params, leaf_table=table, **kw),
                   "predict_puct(endgame_table=)": lambda: ea.predict_puct(b, d, params, endgame_table=table, **kw)}
            one, staged = fns["predict_puct(leaf_table=)"](), fns["predict_puct(endgame_table=)"]()     # the warm-up of both
            counts = ea.puct_search_exact(b, d, params, sims, table, return_leaf_counts=True)[1]
            by_table, by_value = (int(x) for x in counts.sum(0))
            rows = alternated(fns, n, runs)
            print(json.dumps({"board": S, "table": [S, *TABLES[S]], "M": M, "observations": "few cubes", "sims": sims, "launches": n,
                              "leaves_by_table": by_table, "leaves_by_value_head": by_value,
                              "table_share": round(by_table / max(1, by_table + by_value), 4),
                              "same_results": all(torch.equal(x, y) for x, y in zip(one, staged)), "us_per_call_median_min_max": rows,
                              "staged_over_one_launch": round(rows["predict_puct(endgame_table=)"][0] / rows["predict_puct(leaf_table=)"][0], 3)}),
                  flush=True)


def plain(label, runs, launches, sims, batches):
    for S in (5, 7):
        params = params_of(S)
        for M in batches:
            b, d = observations(S, M)
            ea.puct_search(b, d, params, sims)
            print(json.dumps({"tree": label, "board": S, "M": M, "sims": sims,
                              "us": timed(lambda: ea.puct_search(b, d, params, sims), launches_for(M, launches), runs)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024, 16384])
    ap.add_argument("--skip_random", action="store_true")
    ap.add_argument("--skip_few", action="store_true")
    ap.add_argument("--plain", default=None, metavar="LABEL")
    a = ap.parse_args()
    if a.plain is not None:
        return plain(a.plain, a.runs, a.launches, a.sims, a.batches)
    if not a.skip_random:
        random_play(a.runs, a.launches, a.sims, a.batches)
    if not a.skip_few:
        few(a.runs, a.launches, a.sims, a.batches)


if __name__ == "__main__":
    main()
