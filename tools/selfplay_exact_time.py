"""Throughput of whole self-play games with exact endgame leaves, and what the table changes in training.

  python tools/selfplay_exact_time.py --part a|b|d [--runs 5] [--boards 5 7] [--M 1024 16384 65536] [--sims 64]

Part a, the cost of the coverage test: per board and batch, on reset positions (next to no leaf is covered: the share is printed), the
recorded positions per second of selfplay_puct_games_exact against selfplay_puct_games.  --max_plies N cuts the games at N plies:
at 8 no leaf is covered and the records are checked to be the plain call's.
Part b, the gain of whole games: selfplay_puct_games_exact against selfplay_puct(leaf_table=) at chunk 1 024, 4 096 and 16 384 (those
not above M, and M itself), on the same reset positions and on few-cube starts (one to three cubes a side, drawn with numpy).  The
first call of every case is checked against the first case's records, byte for byte.
Each figure of a and b is the median (min, max) of `--runs` timed windows after a warm-up call, a window being one call between two
device events with a synchronisation before and after; the cases of a row are alternated in the same process.
Part d, 5x5: `--updates` updates of PuctSelfPlayTrainer(whole_games=True) and of PuctSelfPlayTrainer(games_table=) from the same seed,
then over `--episodes` episodes the wins of predict_puct(sims=64) on each against minimax(5), with Wilson 95 % intervals.  One run.
Tables: (5, 2, 4) and (7, 2, 3), built once.  Prints one JSON line per row.  No pass bar: nothing here was measured before."""
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
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402
from ewn_gym_amd.distill import PuctSelfPlayTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from tools.distill_time import make_env  # noqa: E402
from tools.selfplay_time import openings, window  # noqa: E402

TABLE = {5: (2, 4), 7: (2, 3)}


def few_cube_starts(S, M, seed=0):
    """M live positions with one to three cubes a side on distinct cells, no agent cube on the last cell, no opposing cube on the first"""
    rng = np.random.default_rng(seed)
    b = np.zeros((M, S * S), np.int8)
    for m in range(M):
        ka, ko = rng.integers(1, 4, 2)
        cells = rng.choice(np.arange(1, S * S - 1), ka + ko, replace=False)
        b[m, cells[:ka]] = rng.choice(np.arange(1, 7), ka, replace=False)
        b[m, cells[ka:]] = -rng.choice(np.arange(1, 7), ko, replace=False)
    d = rng.integers(1, 7, M).astype(np.int8)
    return torch.as_tensor(b.reshape(M, S, S)).cuda(), torch.as_tensor(d).cuda()


def report(row, rates):
    for name, r in rates.items():
        pps = [v[0] for v in r]
        print(json.dumps({**row, "case": name, "positions_per_s_median_min_max": [round(statistics.median(pps)), round(min(pps)), round(max(pps))],
                          "positions_per_call": r[0][1], "seconds_per_call_median": round(statistics.median(v[2] for v in r), 4)}), flush=True)


def alternate(cases, runs, same=True):
    first, rates = None, {k: [] for k in cases}
    for k, fn in cases.items():                                       # warm-up, and (same) the records are the same on every path
        rec = fn()
        first = rec if first is None else first
        assert not same or all(torch.equal(rec[name], first[name]) for name in first), k
    for _ in range(runs):                                             # alternated
        for k, fn in cases.items():
            s, n = window(fn)
            rates[k].append((n / s, n, s))
    return first, rates


def setup(S):
    torch.manual_seed(9)
    return ActorCritic(S, 6).cuda().flat_parameters(), ea.EndgameTable.build(S, *TABLE[S])


def part_a(runs, boards, batches, sims, max_plies):
    for S in boards:
        params, t = setup(S)
        for M in batches:
            b, d = openings(S, M)
            kw = dict(sims=sims, key=3, max_plies=max_plies)
            c = ea.selfplay_puct_games_exact(b, d, params, t, return_leaf_counts=True, **kw)["leaf_counts"].sum(0).tolist()
            cases = {"selfplay_puct_games": lambda: ea.selfplay_puct_games(b, d, params, **kw),
                     "selfplay_puct_games_exact": lambda: ea.selfplay_puct_games_exact(b, d, params, t, **kw)}
            _, rates = alternate(cases, runs, same=c[0] == 0)         # without a table leaf the records are the plain call's
            report({"part": "a", "board": S, "M": M, "sims": sims, "max_plies": max_plies, "starts": "reset", "leaves_by_table": c[0],
                    "leaves_by_value_head": c[1]}, rates)


def part_b(runs, boards, batches, sims):
    for S in boards:
        params, t = setup(S)
        for M in batches:
            for starts, (b, d) in (("reset", openings(S, M)), ("few cubes", few_cube_starts(S, M))):
                cases = {"selfplay_puct_games_exact": lambda b=b, d=d: ea.selfplay_puct_games_exact(b, d, params, t, sims=sims, key=3)}
                for chunk in sorted({min(c, M) for c in (1024, 4096, 16384)}):
                    cases["selfplay_puct(leaf_table=), chunk %d" % chunk] = lambda b=b, d=d, chunk=chunk: ea.selfplay_puct(
                        b, d, params, sims=sims, key=3, chunk=chunk, leaf_table=t)
                first, rates = alternate(cases, runs)
                report({"part": "b", "board": S, "M": M, "sims": sims, "starts": starts, "mean_game_plies": round(float(first["plies"].float().mean()), 2),
                        "longest_game_plies": int(first["plies"].max())}, rates)


def part_d(updates, lanes, train_sims, episodes):
    S = 5
    t = ea.EndgameTable.build(S, *TABLE[S])
    for name, kw in (("whole_games", {"whole_games": True}), ("games_table", {"games_table": t})):
        tr = PuctSelfPlayTrainer(make_env(lanes, S, 1.0), sims=train_sims, learning_rate=1e-3, seed=0, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u in range(updates):
            tr.collect_and_update()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"part": "d", "trainer": name, "updates": updates, "lanes": lanes, "train_sims": train_sims, "positions": tr.num_timesteps,
                          "seconds": round(dt, 1), **{k: round(v, 4) for k, v in tr.stats_dict().items()}}), flush=True)
        r = evaluate({"kind": "mlp_puct", "model": tr.model, "terminal_value": 1.0, "sims": 64}, {"kind": "minimax", "max_depth": 5}, num=episodes,
                     board_size=S)
        print(json.dumps({"part": "d", "trainer": name, "policy": "puct(64)", "opponent": "minimax(5)", "episodes": r["episodes"], "wins": r["wins"],
                          "win_rate": round(r["win_rate"], 4), "ci95": [round(x, 4) for x in r["ci95"]], "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "d"], required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--boards", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 16384, 65536])
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--max_plies", type=int, default=None, help="part a: games cut there (8: no leaf of a reset game is covered yet)")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--train_sims", type=int, default=32)
    ap.add_argument("--episodes", type=int, default=1024)
    a = ap.parse_args()
    if a.part == "d":
        return part_d(a.updates, a.lanes, a.train_sims, a.episodes)
    if a.part == "a":
        return part_a(a.runs, a.boards, a.M, a.sims, a.max_plies)
    part_b(a.runs, a.boards, a.M, a.sims)


if __name__ == "__main__":
    main()
