"""Timing and playing strength of the lookahead on the trained critic (DESIGN.md sections 4k and 4l).

  python tools/lookahead_time.py [--runs 5] [--updates 600] [--episodes 1024] [--plies 2]

Part 1, per board (5x5, 7x7) and batch (M = 1, 1 024, 65 536): predict_lookahead (ewn_predict_lookahead, actions only) beside
predict_policy on the same observations, alternated in the same process.  Each figure is the median of `--runs` timed windows after
warm-up, a window being `launches` back-to-back calls between two device events with a synchronisation before and after; microseconds
per call.  With it the mean number of leaf columns (distinct non-terminal reply positions x 6 dice) per observation, counted on the host
from the rules on the first 1 024 observations.

Part 2, 5x5: a FusedA2CTrainer trained as tools/eval_policy_time.py trains its model (shaped env, reward 10, RandomAgent, `--updates`
updates), then over `--episodes` episodes (seeds 0 .. n-1, MT19937-compat dice) the win rate of its raw argmax policy and of its lookahead
policy (terminal_value = the reward it was trained on) against RandomAgent and against minimax(5), with Wilson 95 % intervals.
Prints one JSON line per row.  No pass bar: nothing here was measured before.

--plies 2 (section 4l): part 1 becomes predict_lookahead(plies=2) beside predict_lookahead(plies=1) at M = 1 and 1 024, alternated in the
same process, with the two stage calls (lookahead_expand, lookahead_reduce at leaf_width 6) timed alone; part 2 gains a lookahead(2) row
per opponent: the same model, seeds, dice and terminal_value.

--endgame_table PATH (section 4p; a table written by EndgameTable.save): instead of the parts above, per batch (M = 1, 1 024, 65 536)
on the table's board predict_lookahead(endgame_table=) beside the plain predict_lookahead on the same observations, alternated in the
same process, actions only.  The observations are every observation of a `--rollout_steps`-step random-agent rollout of 4 096 games with
auto-reset, long enough that games reach their endgames (the step count is printed), repeated up to M; with them the share of leaf
tuples that the table values, from leaf_counts."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic, FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402


def find_cube(present, d, larger):
    if d in present:
        return d
    up = [k for k in range(d + 1, 7) if k in present]
    dn = [k for k in range(d - 1, 0, -1) if k in present]
    return ((up or dn) if larger else (dn or up))[0]


def targets(board, k, sign):
    """[(x, y, nx, ny)] of the moves of cube sign * k that stay on the board"""
    S = board.shape[0]
    x, y = (int(v) for v in np.argwhere(board == sign * k)[0])
    return [(x, y, x + sign * dx, y + sign * dy) for dx, dy in ((0, 1), (1, 0), (1, 1)) if 0 <= x + sign * dx < S and 0 <= y + sign * dy < S]


def leaf_columns(board, d):
    """6 x the number of distinct non-terminal positions after (agent move, reply): what the kernel runs the value net on"""
    if board[0, 0] < 0 or board[-1, -1] > 0 or not (board > 0).any() or not (board < 0).any():
        return 0
    mine = {int(v) for v in board.flat if v > 0}
    n = 0
    for c in {find_cube(mine, d, False), find_cube(mine, d, True)}:
        for x, y, nx, ny in targets(board, c, 1):
            b1 = board.copy()
            b1[x, y], b1[nx, ny] = 0, c
            if b1[-1, -1] > 0 or not (b1 < 0).any():
                continue
            for k in {-int(v) for v in b1.flat if v < 0}:
                for x1, y1, nx1, ny1 in targets(b1, k, -1):
                    b2 = b1.copy()
                    b2[x1, y1], b2[nx1, ny1] = 0, -k
                    n += not (b2[0, 0] < 0 or not (b2 > 0).any())
    return 6 * n


def exact_leaves(t, steps, runs):
    S, N = t.board_size, 4096
    torch.manual_seed(9)
    params = ActorCritic(S, 6).cuda().flat_parameters()
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=7)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 9487).astype(np.uint32))
    traj = env.alloc_rollout(steps)
    env.rollout(steps, agent="random", traj=traj)
    for M in (1, 1024, 65536):
        idx = (torch.arange(M, device="cuda") * 7919) % (steps * N)       # spread over the steps, so that a small M sees every stage of a game
        b, d = traj["board"].reshape(-1, S, S)[idx].contiguous(), traj["dice"].reshape(-1)[idx].contiguous()
        counts = ea.predict_lookahead(b, d, params, endgame_table=t, return_leaf_counts=True)[1].sum(0).tolist()
        fns = {"predict_lookahead endgame_table": lambda: ea.predict_lookahead(b, d, params, endgame_table=t),
               "predict_lookahead": lambda: ea.predict_lookahead(b, d, params)}
        launches = 200 if M <= 1024 else 20
        for fn in fns.values():                                           # warm-up
            for _ in range(5):
                fn()
        rows = {}
        for _ in range(2):                                                # alternate the two, keep the later pass
            for name, fn in fns.items():
                rows[name] = timed(fn, launches, runs)
        print(json.dumps({"board": S, "M": M, "table": [S, t.max_cubes, t.max_total], "rollout_steps": steps, "us_per_call_median_min_max": rows,
                          "covered_roots_share": round(float(t.lookup(b, d)[1].float().mean()), 4), "leaf_tuples_by_table_by_critic": counts,
                          "share_of_leaf_tuples_by_table": round(counts[0] / max(1, counts[0] + counts[1]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=1, choices=(1, 2))
    ap.add_argument("--endgame_table", default=None)
    ap.add_argument("--rollout_steps", type=int, default=64)
    a = ap.parse_args()
    if a.endgame_table is not None:
        return exact_leaves(ea.EndgameTable.load(a.endgame_table), a.rollout_steps, a.runs)
    for S in (5, 7) if a.plies == 2 else ():
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in (1, 1024):
            b, d = observations(S, M)
            lb, ld, kind = ea.lookahead_expand(b, d)
            lq = ea.predict_lookahead(lb.reshape(-1, S, S), ld.reshape(-1), params, return_q=True)[1].reshape(M, 648, 6)
            fns = {"predict_lookahead plies=2": lambda: ea.predict_lookahead(b, d, params, plies=2),
                   "predict_lookahead plies=1": lambda: ea.predict_lookahead(b, d, params),
                   "lookahead_expand": lambda: ea.lookahead_expand(b, d), "lookahead_reduce width 6": lambda: ea.lookahead_reduce(b, d, kind, lq)}
            launches = 200 if M == 1 else 20
            for fn in fns.values():                                       # warm-up
                for _ in range(3):
                    fn()
            rows = {}
            for _ in range(2):                                            # alternate them, keep the later pass
                for name, fn in fns.items():
                    rows[name] = timed(fn, launches, a.runs)
            print(json.dumps({"board": S, "M": M, "us_per_call_median_min_max": rows,
                              "leaf_rows_per_observation": round(float((kind == 2).sum()) * 6 / M, 1)}), flush=True)
    for S in (5, 7) if a.plies == 1 else ():
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in (1, 1024, 65536):
            b, d = observations(S, M)
            hb, hd = b[:1024].cpu().numpy(), d[:1024].cpu().numpy()
            cols = float(np.mean([leaf_columns(hb[m], int(hd[m])) for m in range(hb.shape[0])]))
            fns = {"predict_lookahead": lambda: ea.predict_lookahead(b, d, params), "predict_policy": lambda: ea.predict_policy(b, d, params)}
            launches = 200 if M <= 1024 else 20
            for fn in fns.values():                                       # warm-up
                for _ in range(5):
                    fn()
            rows = {}
            for _ in range(2):                                            # alternate the two, keep the later pass
                for name, fn in fns.items():
                    rows[name] = timed(fn, launches, a.runs)
            print(json.dumps({"board": S, "M": M, "us_per_call_median_min_max": rows, "mean_leaf_columns_per_observation": round(cols, 1)}), flush=True)

    S, N, reward = 5, 4096, 10.0
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=reward, illegal_move_tolerance=10,
                    autoreset=True, shaped_refresh_on_reset=True, philox_key=1)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    tr = FusedA2CTrainer(env, n_steps=5, learning_rate=1e-3, seed=0)
    for _ in range(a.updates):
        tr.collect_and_update()
    torch.cuda.synchronize()
    for opp in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
        for name, agent in (("argmax", {"kind": "mlp", "model": tr.model}),
                            ("lookahead", {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": reward}),
                            ("lookahead(2)", {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": reward, "plies": 2}))[:a.plies + 1]:
            r = evaluate(agent, opp, num=a.episodes, board_size=S)
            print(json.dumps({"policy": name, "opponent": opp["kind"] + ("(5)" if opp["kind"] == "minimax" else ""), "updates": a.updates,
                              "episodes": r["episodes"], "wins": r["wins"], "win_rate": round(r["win_rate"], 4),
                              "ci95": [round(x, 4) for x in r["ci95"]], "avg_length": round(r["avg_length"], 2), "engine": r["engine"]}), flush=True)


if __name__ == "__main__":
    main()
