"""Build and lookup times of the endgame table, and what it says about the critic and the search.

  python tools/endgame_time.py [--runs 5] [--updates 600] [--episodes 1024] [--skip_big] [--skip_strength]

Part (a): ewn_endgame_build of (5, 2, 4), (7, 2, 4) and (5, 3, 5) between two device events, with the table's size; `--runs` builds of
the first, one of each of the others (--skip_big leaves those two out: they need 5.3 and 24.2 GB).
Part (b), 5x5 on the (5, 2, 4) table: EndgameTable.lookup (actions and covered only) beside predict_policy on the same observations at
M = 1, 1 024 and 65 536, alternated in the same process; the median, minimum and maximum of `--runs` windows, microseconds per call.
Part (c), 5x5: a SearchDistillTrainer and a FusedA2CTrainer trained as tools/distill_time.py part (b) trains them.  Then, on the
agent-to-move observations of a 64-step rollout of each model's own policy on 4 096 lanes: the share the table covers, and on the covered
ones the critic's |V / terminal_value - max q_exact|, the one-move and the two-move lookahead's |Q / terminal_value - q_exact| over the
moves that stay on the board (mean and maximum), and how often the argmax policy, the critic-free lookaheads' actions are exact-optimal
(their q_exact equals the row's maximum).
With the (5, 3, 5) table built (not --skip_big, and at least 32 GiB of device memory free), also DESIGN.md section 4p's figure: on
the rows that (5, 3, 5) covers and (5, 2, 4) does not, the one-move and two-move |Q / terminal_value - q_exact| against the large
table's q_exact, with the critic alone at the leaves and with the (5, 2, 4) table's exact values at the leaves it covers.
Part (d): over `--episodes` episodes (seeds 0 .. n-1, MT19937-compat dice) the wins of EndgameAgent(table, fallback=ValueSearchAgent)
and of ValueSearchAgent(endgame_table=table), the lookahead with exact leaves (4p), beside the bare ValueSearchAgent, against
RandomAgent and minimax(5), Wilson 95 % intervals.
One JSON line per row.  No pass bar: nothing here was measured before."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic, FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.distill import SearchDistillTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from tools.distill_time import make_env  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402


def build_ms(S, K, T, runs):
    n = ea.EndgameTable.table_bytes(S, K, T) // 4
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t = ea.EndgameTable.build(S, K, T, out=out)
        b.record()
        torch.cuda.synchronize()
        times.append(round(a.elapsed_time(b), 2))
    print(json.dumps({"table": [S, K, T], "bytes": 4 * n, "levels": t.levels, "build_ms": times}), flush=True)
    return t


def part_b(t, runs):
    S = t.board_size
    torch.manual_seed(9)
    params = ActorCritic(S, 6).cuda().flat_parameters()
    for M in (1, 1024, 65536):
        b, d = observations(S, M)
        fns = {"endgame lookup": lambda: t.lookup(b, d), "predict_policy": lambda: ea.predict_policy(b, d, params)}
        launches = 200 if M <= 1024 else 50
        for fn in fns.values():
            for _ in range(10):
                fn()
        rows = {}
        for _ in range(2):                                            # alternate the two, keep the later pass
            for name, fn in fns.items():
                rows[name] = timed(fn, launches, runs)
        print(json.dumps({"board": S, "M": M, "us_per_call_median_min_max": rows, "covered_share": round(float(t.lookup(b, d)[1].float().mean()), 4)}),
              flush=True)


def against_the_table(name, tr, tv, tables):
    """the model's own policy rollout, and its critic and lookaheads against q_exact on the rows the first table covers"""
    S, N, K = 5, 4096, 64
    env = make_env(N, S)
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, tr.params, traj=traj, noise_key=3)
    b = traj["obs_board"][:K].reshape(K * N, S, S).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    row = {"trained": name, "observations": K * N}
    for t in tables:
        row["covered_share (%d, %d, %d)" % (t.board_size, t.max_cubes, t.max_total)] = round(float(t.lookup(b, d)[1].float().mean()), 4)
    t = tables[0]
    _, cov, qe = t.lookup(b, d, return_q=True)
    b, d, qe = b[cov].contiguous(), d[cov].contiguous(), qe[cov].reshape(-1, 6)
    best = qe.max(1).values
    on = torch.isfinite(qe)
    act, value = ea.predict_policy(b, d, tr.params, return_value=True)
    ev = (value / tv - best).abs()
    row.update({"covered": int(cov.sum()), "critic_abs_err_mean_max": [round(float(ev.mean()), 4), round(float(ev.max()), 4)]})

    def optimal(a):
        return round(float((qe.gather(1, (a[:, 0].long() * 3 + a[:, 1].long())[:, None])[:, 0] == best).float().mean()), 4)
    row["argmax_policy_optimal"] = optimal(act)
    for plies in (1, 2):
        a, q = ea.predict_lookahead(b, d, tr.params, terminal_value=tv, return_q=True, plies=plies)
        e = (q.reshape(-1, 6) / tv - qe).abs()[on]
        row["lookahead(%d)_abs_err_mean_max" % plies] = [round(float(e.mean()), 4), round(float(e.max()), 4)]
        row["lookahead(%d)_optimal" % plies] = optimal(a)
    print(json.dumps(row), flush=True)
    if len(tables) > 1:
        exact_leaves(name, tr, tv, tables[0], tables[1], traj, K * N)


def exact_leaves(name, tr, tv, small, big, traj, M):
    """the positions the exact leaves are for: covered by `big`, not by `small`; Q with the critic at every leaf and with `small`'s
    exact values at the leaves it covers, against `big`'s q_exact"""
    S = small.board_size
    b = traj["obs_board"][:-1].reshape(M, S, S).contiguous()
    d = traj["obs_dice"][:-1].reshape(M).contiguous()
    _, cov_big, qe = big.lookup(b, d, return_q=True)
    rows = cov_big & ~small.lookup(b, d)[1]
    b, d, qe = b[rows].contiguous(), d[rows].contiguous(), qe[rows].reshape(-1, 6)
    on, best = torch.isfinite(qe), qe.max(1).values
    counts = ea.predict_lookahead(b, d, tr.params, terminal_value=tv, endgame_table=small, return_leaf_counts=True)[1].sum(0).tolist()
    row = {"trained": name, "rows covered by %s and not by %s" % ((big.board_size, big.max_cubes, big.max_total), (S, small.max_cubes, small.max_total)):
           int(rows.sum()), "leaf_tuples_by_table_by_critic": counts}
    for plies in (1, 2):
        for label, t in (("critic leaves", None), ("exact leaves", small)):
            a, q = ea.predict_lookahead(b, d, tr.params, terminal_value=tv, return_q=True, plies=plies, endgame_table=t)
            e = (q.reshape(-1, 6) / tv - qe).abs()[on]
            opt = (qe.gather(1, (a[:, 0].long() * 3 + a[:, 1].long())[:, None])[:, 0] == best).float().mean()
            row["lookahead(%d) %s: abs_err_mean_max, optimal" % (plies, label)] = [round(float(e.mean()), 4), round(float(e.max()), 4), round(float(opt), 4)]
    print(json.dumps(row), flush=True)


def strength(name, tr, tv, t, episodes):
    for opp in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
        bare = {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": tv}
        for pol, agent in (("lookahead", bare), ("endgame+lookahead", {"kind": "endgame", "table": t, "fallback": bare}),
                           ("lookahead+exact leaves", dict(bare, endgame_table=t))):
            r = evaluate(agent, opp, num=episodes, board_size=5)
            print(json.dumps({"trained": name, "policy": pol, "opponent": opp["kind"] + ("(5)" if opp["kind"] == "minimax" else ""),
                              "episodes": r["episodes"], "wins": r["wins"], "win_rate": round(r["win_rate"], 4),
                              "ci95": [round(x, 4) for x in r["ci95"]], "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--skip_big", action="store_true")
    ap.add_argument("--skip_strength", action="store_true")
    a = ap.parse_args()
    tables = [build_ms(5, 2, 4, a.runs)]
    part_b(tables[0], a.runs)
    if not a.skip_big and torch.cuda.mem_get_info()[0] < 32 << 30:
        print(json.dumps({"skipped": "(7, 2, 4) and (5, 3, 5): less than 32 GiB of device memory free"}), flush=True)
        a.skip_big = True
    if not a.skip_big:
        t7 = build_ms(7, 2, 4, 1)
        del t7
        torch.cuda.empty_cache()
        tables.append(build_ms(5, 3, 5, 1))
    if a.skip_strength:
        return
    S, N, reward = 5, 4096, 10.0
    trainers = {"SEARCH": SearchDistillTrainer(make_env(N, S, reward), n_steps=5, learning_rate=1e-3, seed=0),
                "A2C": FusedA2CTrainer(make_env(N, S, reward), n_steps=5, learning_rate=1e-3, seed=0)}
    for name, tr in trainers.items():
        for _ in range(a.updates):
            tr.collect_and_update()
        torch.cuda.synchronize()
        tv = 1.0 if name == "SEARCH" else reward      # the scale its critic was trained on
        against_the_table(name, tr, tv, tables)
        strength(name, tr, tv, tables[0], a.episodes)


if __name__ == "__main__":
    main()
