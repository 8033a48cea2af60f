"""Timing and playing strength of the PUCT search on the trained actor-critic.

  python tools/puct_time.py [--runs 5] [--updates 600] [--episodes 1024] [--sims 16 64 256] [--skip_timing] [--skip_strength]

Part 1, per board (5x5, 7x7) and batch (M = 1, 1 024): predict_puct (actions only) at each budget beside predict_lookahead at plies 1
and 2 on the same observations, alternated in the same process.  Each figure is the median (min, max) of `--runs` timed windows after
warm-up, a window being `launches` back-to-back calls between two device events with a synchronisation before and after; microseconds
per call.  With it, per budget, one search driven by hand with a device event between the stages: the microseconds inside the tree
kernels (begin, the advances, result) and inside ewn_predict_policy, and the tree kernels' share of their sum.

Part 2, 5x5: the FusedA2CTrainer model of tools/lookahead_time.py (4k's: shaped env, reward 10, RandomAgent, `--updates` updates), then
over `--episodes` episodes (seeds 0 .. n-1, MT19937-compat dice) the wins of its argmax policy, its lookaheads and its PUCT search at each
budget (terminal_value = the reward it was trained on) against RandomAgent and against minimax(5), with Wilson 95 % intervals.

Part 3: on the observations of a 64-step rollout of the model's own policy that EndgameTable (5, 2, 4) covers (4n's rows), the share
of actions with the maximal q_exact: argmax, the lookaheads, PUCT at each budget.
Prints one JSON line per row.  No pass bar: nothing here was measured before."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic, FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from tools.distill_time import make_env  # noqa: E402
from tools.predict_policy_time import observations, timed  # noqa: E402


def stage_split(S, b, d, params, sims):
    """one search by hand, a device event between the stages -> microseconds in the tree kernels, in ewn_predict_policy"""
    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e
    marks = [("", ev())]
    tree, lb, ld = ea.puct_begin(b, d, sims)
    marks.append(("tree", ev()))
    for _ in range(sims + 1):
        _, logits, value = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        marks.append(("policy", ev()))
        ea.puct_advance(tree, logits, value, lb, ld, sims)
        marks.append(("tree", ev()))
    ea.puct_result(tree, S, sims)
    marks.append(("tree", ev()))
    torch.cuda.synchronize()
    t = {"tree": 0.0, "policy": 0.0}
    for (_, e0), (name, e1) in zip(marks, marks[1:]):
        t[name] += e0.elapsed_time(e1) * 1000.0
    return t


def part1(runs, budgets):
    for S in (5, 7):
        torch.manual_seed(9)
        params = ActorCritic(S, 6).cuda().flat_parameters()
        for M in (1, 1024):
            b, d = observations(S, M)
            fns = {"predict_lookahead plies=1": (lambda: ea.predict_lookahead(b, d, params), 200),
                   "predict_lookahead plies=2": (lambda: ea.predict_lookahead(b, d, params, plies=2), 20)}
            for sims in budgets:
                fns["predict_puct sims=%d" % sims] = (lambda sims=sims: ea.predict_puct(b, d, params, sims=sims), max(2, 400 // (sims + 1)))
            for fn, _ in fns.values():                                    # warm-up
                for _ in range(3):
                    fn()
            rows = {}
            for _ in range(2):                                            # alternate them, keep the later pass
                for name, (fn, launches) in fns.items():
                    rows[name] = timed(fn, launches, runs)
            print(json.dumps({"board": S, "M": M, "us_per_call_median_min_max": rows}), flush=True)
            for sims in budgets:
                stage_split(S, b, d, params, sims)
                t = stage_split(S, b, d, params, sims)
                _, visits = ea.predict_puct(b, d, params, sims=sims, return_visits=True)
                print(json.dumps({"board": S, "M": M, "sims": sims, "tree_kernels_us": round(t["tree"], 1),
                                  "predict_policy_us": round(t["policy"], 1), "tree_share": round(t["tree"] / (t["tree"] + t["policy"]), 3),
                                  "tree_KB": ea._lib.load().ewn_puct_tree_bytes(S, 3, sims) // 1024,
                                  "mean_max_visit_share": round(float((visits.reshape(M, 6).max(1).values.float() / sims).mean()), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--sims", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_strength", action="store_true")
    a = ap.parse_args()
    if not a.skip_timing:
        part1(a.runs, a.sims)
    if a.skip_strength:
        return
    S, N, reward = 5, 4096, 10.0
    tr = FusedA2CTrainer(make_env(N, S, reward), n_steps=5, learning_rate=1e-3, seed=0)
    for _ in range(a.updates):
        tr.collect_and_update()
    torch.cuda.synchronize()
    agents = [("argmax", {"kind": "mlp", "model": tr.model}),
              ("lookahead", {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": reward}),
              ("lookahead(2)", {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": reward, "plies": 2})]
    agents += [("puct(%d)" % s, {"kind": "mlp_puct", "model": tr.model, "terminal_value": reward, "sims": s}) for s in a.sims]
    for opp in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
        for name, agent in agents:
            r = evaluate(agent, opp, num=a.episodes, board_size=S)
            print(json.dumps({"policy": name, "opponent": opp["kind"] + ("(5)" if opp["kind"] == "minimax" else ""), "updates": a.updates,
                              "episodes": r["episodes"], "wins": r["wins"], "win_rate": round(r["win_rate"], 4),
                              "ci95": [round(x, 4) for x in r["ci95"]], "avg_length": round(r["avg_length"], 2), "engine": r["engine"]}), flush=True)
    # part 3: against the exact values, on 4n's rows
    K = 64
    env = make_env(N, S, reward)
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, tr.params, traj=traj, noise_key=3)
    b = traj["obs_board"][:K].reshape(K * N, S, S).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    table = ea.EndgameTable.build(S, 2, 4)
    _, cov, qe = table.lookup(b, d, return_q=True)
    b, d, qe = b[cov].contiguous(), d[cov].contiguous(), qe[cov].reshape(-1, 6)
    best = qe.max(1).values

    def optimal(act):
        return round(float((qe.gather(1, (act[:, 0].long() * 3 + act[:, 1].long())[:, None])[:, 0] == best).float().mean()), 4)
    row = {"observations": K * N, "covered": int(cov.sum()), "argmax_optimal": optimal(ea.predict_policy(b, d, tr.params))}
    for plies in (1, 2):
        row["lookahead(%d)_optimal" % plies] = optimal(ea.predict_lookahead(b, d, tr.params, terminal_value=reward, plies=plies))
    for s in a.sims:
        act, q, value = ea.predict_puct(b, d, tr.params, sims=s, terminal_value=reward, return_q=True, return_value=True)
        row["puct(%d)_optimal" % s] = optimal(act)
        ev = (value - best).abs()
        row["puct(%d)_root_value_abs_err_mean_max" % s] = [round(float(ev.mean()), 4), round(float(ev.max()), 4)]
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
