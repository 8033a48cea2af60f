"""Throughput and learning of PUCT self-play.

  python tools/selfplay_time.py [--runs 3] [--updates 200] [--lanes 1024] [--train_sims 32] [--episodes 1024] [--skip_timing] [--skip_learning]

Part 1, per board (5x5, 7x7), batch (M = 1 024, 4 096 openings) and budget (sims 16, 64): recorded positions per second of selfplay_puct,
games played to their end.  Each figure is the median (min, max) of `--runs` timed windows after a warm-up call, a window being one
call between two device events with a synchronisation before and after; the configurations are alternated in the same process.
Part 2, per board and budget at M = 1 024: the share of a ply spent in the noise draw (torch._standard_gamma), in the search (begin,
ewn_predict_policy, the advances) and in ewn_puct_play.  A window is the first eight plies through the driver's own calls with a
device event between the stages; median (min, max) of `--runs` windows after a warm-up, the configurations alternated.
Part 3, 5x5: `--updates` updates of PuctSelfPlayTrainer from a fresh network, then over `--episodes` episodes (seeds 0 .. n-1,
MT19937-compat dice) the wins of its argmax policy and of predict_puct(sims=64) on it against RandomAgent and against minimax(5), with
Wilson 95 % intervals (DESIGN.md sets 4m's A2C and SEARCH rows beside them: this tool does not train those again).
With --whole_games only this runs: per board (--boards), batch (--M) and budget (--sims) the recorded positions
per second of selfplay_puct(fused=True) at chunk 1 024, 4 096 and 16 384 (those not above M, and M itself) and of selfplay_puct_games
at every --tile (0: the library's choice) and --blocks, all alternated in one process, windows as in part 1.  The first call of every
case is checked against the first case's records, byte for byte.
Prints one JSON line per row.  No pass bar: nothing here was measured before."""
import argparse
import ctypes as C
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
from ewn_gym_amd._args import _ptr, _stream  # noqa: E402
from ewn_gym_amd.search import _puct_search  # noqa: E402
from tools.distill_time import make_env  # noqa: E402


def openings(S, M):
    env = ea.VecEWN(M, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=M, philox_key=7)
    b, d = env.reset(seeds=(np.arange(M, dtype=np.uint64) + 9487).astype(np.uint32))
    return b.clone(), d.clone()


def window(fn):
    """one call between two device events -> (seconds, recorded positions)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    rec = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1000.0, int(rec["live"].sum())


def part1(runs):
    cases = {}
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in (1024, 4096):
            b, d = openings(S, M)
            for sims in (16, 64):
                cases[(S, M, sims)] = lambda b=b, d=d, params=params, sims=sims: ea.selfplay_puct(b, d, params, sims=sims, key=3)
    rates = {k: [] for k in cases}
    for k, fn in cases.items():                                       # warm-up
        window(fn)
    for _ in range(runs):                                             # alternated
        for k, fn in cases.items():
            s, n = window(fn)
            rates[k].append((n / s, n, s))
    for (S, M, sims), r in rates.items():
        pps = [x[0] for x in r]
        print(json.dumps({"board": S, "M": M, "sims": sims, "positions_per_s_median_min_max": [round(statistics.median(pps)), round(min(pps)), round(max(pps))],
                          "positions_per_call": r[0][1], "seconds_per_call_median": round(statistics.median(x[2] for x in r), 3)}), flush=True)


def part_games(runs, boards, batches, budgets, tiles, blocks):
    for S in boards:
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in batches:
            b, d = openings(S, M)
            for sims in budgets:
                cases = {}
                for chunk in sorted({min(c, M) for c in (1024, 4096, 16384)}):
                    cases[("fused", chunk, 0)] = lambda chunk=chunk: ea.selfplay_puct(b, d, params, sims=sims, key=3, fused=True, chunk=chunk)
                for tile in tiles:
                    cases[("whole_games", tile, blocks)] = lambda tile=tile: ea.selfplay_puct_games(b, d, params, sims=sims, key=3, tile=tile or None,
                                                                                                    blocks=blocks or None)
                first, rates = None, {k: [] for k in cases}
                for k, fn in cases.items():                           # warm-up, and the records are the same on every path
                    rec = fn()
                    first = rec if first is None else first
                    assert all(torch.equal(rec[name], first[name]) for name in first), k
                for _ in range(runs):                                 # alternated
                    for k, fn in cases.items():
                        s, n = window(fn)
                        rates[k].append((n / s, n, s))
                # the whole-games path draws the noise of all max_plies plies up front, the ply loop only the plies it plays
                T = ea.search.SELFPLAY_MAX_PLIES[S]
                draw = [window(lambda: {"live": torch.stack([ea.selfplay_noise(M, 1.0, 3, 0, t) for t in range(T)])[0, :, 0] > 0})[0] for _ in range(runs + 1)][1:]
                print(json.dumps({"board": S, "M": M, "sims": sims, "noise_of_all_%d_plies_seconds_median_min_max" % T:
                                  [round(statistics.median(draw), 5), round(min(draw), 5), round(max(draw), 5)],
                                  "longest_game_plies": int(first["plies"].max()), "mean_game_plies": round(float(first["plies"].float().mean()), 2)}), flush=True)
                for (path, x, y), r in rates.items():
                    pps = [v[0] for v in r]
                    print(json.dumps({"board": S, "M": M, "sims": sims, "path": path, **({"chunk": x} if path == "fused" else {"tile": x, "blocks": y}),
                                      "positions_per_s_median_min_max": [round(statistics.median(pps)), round(min(pps)), round(max(pps))],
                                      "positions_per_call": r[0][1], "seconds_per_call_median": round(statistics.median(v[2] for v in r), 4)}), flush=True)


def part2(runs):
    cases = {}
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        M = 1024
        b0, d0 = openings(S, M)
        lib, st = ea._lib.load(), _stream()
        cp, tv = C.c_float(1.5), C.c_float(1.0)
        for sims in (16, 64):
            nb = int(lib.ewn_puct_tree_bytes(S, 3, sims))
            scratch = (torch.empty((M, nb), dtype=torch.uint8, device="cuda"), torch.empty((M, S, S), dtype=torch.int8, device="cuda"),
                       torch.empty(M, dtype=torch.int8, device="cuda"), torch.empty((M, 2), dtype=torch.int8, device="cuda"),
                       torch.empty((M, 5), device="cuda"), torch.empty(M, device="cuda"))
            rec = {"board": torch.zeros((M, S, S), dtype=torch.int8, device="cuda"), "dice": torch.zeros(M, dtype=torch.int8, device="cuda"),
                   "visits": torch.zeros((M, 6), dtype=torch.int32, device="cuda"), "value": torch.zeros(M, device="cuda"),
                   "action": torch.zeros((M, 2), dtype=torch.int8, device="cuda"), "live": torch.zeros(M, dtype=torch.int8, device="cuda")}

            def eight_plies(S=S, sims=sims, params=params, b0=b0, d0=d0, scratch=scratch, rec=rec):
                """a window: the first eight plies through the driver's own calls, a device event between the stages -> us per ply"""
                cb, cd = b0.clone(), d0.clone()
                game = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
                t = {"noise": 0.0, "search": 0.0, "play": 0.0}
                for ply in range(8):
                    marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    torch.cuda.synchronize()
                    marks[0].record()
                    noise = ea.selfplay_noise(M, 1.0, 3, 0, ply)
                    marks[1].record()
                    _puct_search(lib, S, 3, M, sims, cb, cd, params, cp, tv, None, scratch, st, noise, 0.25)
                    marks[2].record()
                    lib.ewn_puct_play(S, 3, M, _ptr(scratch[0]), _ptr(cb), _ptr(cd), _ptr(game), 8, C.c_uint64(3), C.c_int64(0),
                                      *[_ptr(rec[k]) for k in ("board", "dice", "visits", "value", "action", "live")], st)
                    marks[3].record()
                    torch.cuda.synchronize()
                    for name, e0, e1 in zip(t, marks, marks[1:]):
                        t[name] += e0.elapsed_time(e1) * 1000.0 / 8
                return t
            cases[(S, sims)] = eight_plies
    for fn in cases.values():                                         # warm-up
        fn()
    got = {k: [] for k in cases}
    for _ in range(runs):                                             # alternated
        for k, fn in cases.items():
            got[k].append(fn())
    for (S, sims), ws in got.items():
        mmm = lambda xs: [round(statistics.median(xs), 1), round(min(xs), 1), round(max(xs), 1)]  # noqa: E731
        share = lambda name: [w[name] / sum(w.values()) for w in ws]  # noqa: E731
        print(json.dumps({"board": S, "M": 1024, "sims": sims, "us_per_ply_median_min_max": {k: mmm([w[k] for w in ws]) for k in ws[0]},
                          "play_share_median_min_max": [round(x, 4) for x in (statistics.median(share("play")), min(share("play")), max(share("play")))],
                          "noise_share_median_min_max": [round(x, 4) for x in (statistics.median(share("noise")), min(share("noise")),
                                                                               max(share("noise")))]}), flush=True)


def part3(updates, lanes, train_sims, episodes):
    S = 5
    tr = PuctSelfPlayTrainer(make_env(lanes, S, 1.0), sims=train_sims, learning_rate=1e-3, seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for u in range(updates):
        tr.collect_and_update()
        if u % max(1, updates // 8) == 0 or u == updates - 1:
            print(json.dumps({"update": u, "positions": tr.num_timesteps, **{k: round(v, 4) for k, v in tr.stats_dict().items()}}), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"updates": updates, "lanes": lanes, "train_sims": train_sims, "positions": tr.num_timesteps, "seconds": round(dt, 1),
                      "positions_per_s": round(tr.num_timesteps / dt)}), flush=True)
    agents = [("argmax", {"kind": "mlp", "model": tr.model}), ("puct(64)", {"kind": "mlp_puct", "model": tr.model, "terminal_value": 1.0, "sims": 64})]
    for opp in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
        for name, agent in agents:
            r = evaluate(agent, opp, num=episodes, board_size=S)
            print(json.dumps({"policy": name, "opponent": opp["kind"] + ("(5)" if opp["kind"] == "minimax" else ""), "updates": updates,
                              "episodes": r["episodes"], "wins": r["wins"], "win_rate": round(r["win_rate"], 4),
                              "ci95": [round(x, 4) for x in r["ci95"]], "avg_length": round(r["avg_length"], 2), "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--train_sims", type=int, default=32)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_learning", action="store_true")
    ap.add_argument("--whole_games", action="store_true", help="only the comparison of selfplay_puct(fused=True) with selfplay_puct_games")
    ap.add_argument("--boards", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--M", type=int, nargs="+", default=[1024, 4096, 16384, 65536])
    ap.add_argument("--sims", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--tile", type=int, nargs="+", default=[0, 4, 8, 16, 32], help="--whole_games: columns per block, 0 the library's choice")
    ap.add_argument("--blocks", type=int, default=256, help="--whole_games: blocks, 0 the library's choice")
    a = ap.parse_args()
    if a.whole_games:
        return part_games(a.runs, a.boards, a.M, a.sims, a.tile, a.blocks)
    if not a.skip_timing:
        part1(a.runs)
        part2(a.runs)
    if not a.skip_learning:
        part3(a.updates, a.lanes, a.train_sims, a.episodes)


if __name__ == "__main__":
    main()
