"""Throughput of the arena: two networks' PUCT searches playing whole games in one launch.

  python tools/arena_time.py [--runs 5] [--boards 5 7] [--M 1024 16384 65536] [--sims 64]

Per board and batch, on reset positions, each start position played once with each network moving first (first[m] = m & 1), no
noise and the most visited move, the recorded positions per second of
  arena_puct_games               the one launch (ewn_puct_arena)
  arena_puct, chunk C            the staged definition at chunk 1 024, 4 096 and 16 384 (those not above M, and M itself)
  selfplay_puct_games            network A against itself on the same positions with noise_eps=0, temp_plies=0: the arena over this
                                 is the cost of the per-phase pack plus the waiting columns (other games, so per position)
The first call of every arena case is checked against the first case's records, byte for byte.  Each figure is the median (min, max)
of `--runs` timed windows after a warm-up call, a window being one call between two device events with a synchronisation before and
after; the cases of a row are alternated in the same process.  Prints one JSON line per case, and per row the two ratios of the
medians.  No pass bar: nothing here was measured before."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402
from tools.selfplay_exact_time import report  # noqa: E402
from tools.selfplay_time import openings, window  # noqa: E402


def network(S, seed):
    torch.manual_seed(seed)
    return ActorCritic(S, 6).cuda().flat_parameters()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--boards", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 16384, 65536])
    ap.add_argument("--sims", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("arena_time: needs a GPU; a time taken anywhere else says nothing")
    for S in a.boards:
        pa, pb = network(S, 9), network(S, 10)
        for M in a.M:
            b, d = openings(S, (M + 1) // 2)
            b, d = b.repeat_interleave(2, 0)[:M].contiguous(), d.repeat_interleave(2, 0)[:M].contiguous()
            first = (torch.arange(M, device="cuda") & 1).to(torch.int8)
            kw = dict(sims=a.sims, key=3)
            cases = {"arena_puct_games": lambda: ea.arena_puct_games(b, d, pa, pb, first, **kw)}
            for chunk in sorted({min(c, M) for c in (1024, 4096, 16384)}):
                cases["arena_puct, chunk %d" % chunk] = lambda chunk=chunk: ea.arena_puct(b, d, pa, pb, first, chunk=chunk, **kw)
            arena_cases = list(cases)
            cases["selfplay_puct_games"] = lambda: ea.selfplay_puct_games(b, d, pa, noise_eps=0.0, temp_plies=0, **kw)
            warm = {k: fn() for k, fn in cases.items()}               # warm-up, and the arena's records are the same on both paths
            rec, own_rec = warm["arena_puct_games"], warm["selfplay_puct_games"]
            assert all(torch.equal(warm[k][name], rec[name]) for k in arena_cases for name in rec), (S, M)
            del warm
            all_rates = {k: [] for k in cases}
            for _ in range(a.runs):                                   # alternated
                for k, fn in cases.items():
                    s, n = window(fn)
                    all_rates[k].append((n / s, n, s))
            rates = {k: all_rates[k] for k in arena_cases}
            own_rates = {"selfplay_puct_games": all_rates["selfplay_puct_games"]}
            row = {"board": S, "M": M, "sims": a.sims, "starts": "reset, each twice", "mean_game_plies": round(float(rec["plies"].float().mean()), 2),
                   "longest_game_plies": int(rec["plies"].max()), "a_wins": int((rec["result_a"] > 0).sum())}
            report(row, rates)
            report(dict(row, mean_game_plies=round(float(own_rec["plies"].float().mean()), 2), longest_game_plies=int(own_rec["plies"].max()),
                        a_wins=None), own_rates)
            med = {k: statistics.median(v[0] for v in r) for k, r in {**rates, **own_rates}.items()}
            staged = max(v for k, v in med.items() if k.startswith("arena_puct, "))
            print(json.dumps({"board": S, "M": M, "sims": a.sims, "one_launch_over_best_staged": round(med["arena_puct_games"] / staged, 3),
                              "arena_over_selfplay_per_position": round(med["arena_puct_games"] / med["selfplay_puct_games"], 3)}), flush=True)


if __name__ == "__main__":
    main()
