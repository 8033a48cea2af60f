"""Timing and playing strength of search distillation.

  python tools/distill_time.py [--runs 5] [--updates 600] [--episodes 1024] [--lanes 65536] [--skip_strength]

Part (a), 5x5 and 7x7, `--lanes` lanes x 5 steps (M = 327 680 at the default): device-event times of one SearchDistillTrainer update
split into rollout (ewn_step_k_policy and the packing of its observations), lookahead (ewn_predict_lookahead with q), targets
(ewn_lookahead_targets), gradient (ewn_sup_grad: rows, value pass, policy pass, reduce) and apply (ewn_a2c_apply); the median, minimum
and maximum of `--runs` windows of one update each, microseconds.  Then ewn_sup_grad on those M samples alternated in the same process
with ewn_a2c_grad on the same number of samples (the same lanes, K = 5: the parent's kernel on the same step body), and their ratio.

Part (b), 5x5: a SearchDistillTrainer and a FusedA2CTrainer trained on the same shaped env for the same number of env steps (`--updates`
updates of 4 096 lanes x 5 steps, RandomAgent opponent, lr 1e-3 as tools/lookahead_time.py trains its model), then over `--episodes`
episodes (seeds 0 .. n-1, MT19937-compat dice) the wins of each model's argmax policy and of its one-move lookahead against RandomAgent
and against minimax(5), with Wilson 95 % intervals.  One JSON line per row.  No pass bar: nothing here was measured before."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd._lib import EwnA2cHyper, check  # noqa: E402
from ewn_gym_amd.a2c import FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.distill import SearchDistillTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402
from ewn_gym_amd._args import _ptr, _stream  # noqa: E402
from tools.predict_policy_time import timed  # noqa: E402


def make_env(N, S, reward=10.0):
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=reward, illegal_move_tolerance=10,
                    autoreset=True, shaped_refresh_on_reset=True, philox_key=1)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    return env


def split_update(tr):
    """one update of `tr` stage by stage between device events -> microseconds per stage"""
    env, K, N, S = tr.env, tr.n_steps, tr.env.N, tr.env.S
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    torch.cuda.synchronize()
    ev[0].record()
    env.rollout_policy(K, tr.params, traj=tr.traj, noise_key=tr.noise_key)
    tr._boards.view(K, N, S, S).copy_(tr.traj["obs_board"][:K])
    tr._dice.view(K, N).copy_(tr.traj["obs_dice"][:K])
    ev[1].record()
    _, q = ea.predict_lookahead(tr._boards, tr._dice, tr.params, terminal_value=tr.terminal_value, return_q=True, plies=tr.plies)
    ev[2].record()
    tp, tv, w = ea.lookahead_targets(q, tr.temperature)
    ev[3].record()
    ea.sup_grad(tr._boards, tr._dice, tp, tv, tr.params, weight=w, pi_coef=tr.pi_coef, vf_coef=tr.vf_coef, out=tr.grad, scratch=tr.scratch)
    ev[4].record()
    check(tr.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(tr.params), _ptr(tr.sq_avg), _ptr(tr.grad), C.byref(tr.hyper), _ptr(tr.grad_norm),
                               _stream()), "ewn_a2c_apply")
    ev[5].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) * 1000.0 for i in range(5)], (tp, tv, w)


def part_a(a):
    for S in (5, 7):
        env = make_env(a.lanes, S)
        tr = SearchDistillTrainer(env, n_steps=5, seed=0)
        for _ in range(3):
            tr.collect_and_update()
        rows = [split_update(tr)[0] for _ in range(a.runs)]
        names = ("rollout", "lookahead", "targets", "gradient", "apply")
        stat = {n: [round(f([r[i] for r in rows]), 1) for f in (statistics.median, min, max)] for i, n in enumerate(names)}
        print(json.dumps({"board": S, "lanes": a.lanes, "n_steps": 5, "us_median_min_max": stat,
                          "update_us_median": round(statistics.median([sum(r) for r in rows]), 1)}), flush=True)
        # ewn_sup_grad beside ewn_a2c_grad on the same number of samples
        _, (tp, tv, w) = split_update(tr)
        hp = EwnA2cHyper(0.99, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
        nscr = check(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), 5))
        scr = torch.zeros(int(nscr), dtype=torch.uint8, device="cuda")
        grad2 = torch.zeros_like(tr.grad)
        fns = {"ewn_sup_grad": lambda: ea.sup_grad(tr._boards, tr._dice, tp, tv, tr.params, weight=w, out=tr.grad, scratch=tr.scratch),
               "ewn_a2c_grad": lambda: check(env.lib.ewn_a2c_grad(C.byref(env.cfg), 5, _ptr(tr.traj["record"]), _ptr(tr.traj["reward"]),
                                                                  _ptr(tr.params), C.byref(hp), _ptr(grad2), _ptr(scr), _stream()))}
        for fn in fns.values():
            for _ in range(3):
                fn()
        out = {}
        for _ in range(2):                                            # alternate the two, keep the later pass
            for name, fn in fns.items():
                out[name] = timed(fn, 10, a.runs)
        print(json.dumps({"board": S, "samples": 5 * a.lanes, "us_per_call_median_min_max": out,
                          "ratio_sup_over_a2c": round(out["ewn_sup_grad"][0] / out["ewn_a2c_grad"][0], 3)}), flush=True)


def part_b(a):
    S, N, reward = 5, 4096, 10.0
    trainers = {"SEARCH": SearchDistillTrainer(make_env(N, S, reward), n_steps=5, learning_rate=1e-3, seed=0),
                "A2C": FusedA2CTrainer(make_env(N, S, reward), n_steps=5, learning_rate=1e-3, seed=0)}
    for name, tr in trainers.items():
        for _ in range(a.updates):
            tr.collect_and_update()
        torch.cuda.synchronize()
        st = tr.stats_dict()
        print(json.dumps({"trained": name, "updates": a.updates, "env_steps": tr.num_timesteps,
                          **{k: round(float(v), 4) for k, v in st.items()}}), flush=True)
        tv = 1.0 if name == "SEARCH" else reward      # the scale its critic was trained on
        for opp in ({"kind": "random"}, {"kind": "minimax", "max_depth": 5}):
            for pol, agent in (("argmax", {"kind": "mlp", "model": tr.model}),
                               ("lookahead", {"kind": "mlp_lookahead", "model": tr.model, "terminal_value": tv})):
                r = evaluate(agent, opp, num=a.episodes, board_size=S)
                print(json.dumps({"trained": name, "policy": pol, "opponent": opp["kind"] + ("(5)" if opp["kind"] == "minimax" else ""),
                                  "episodes": r["episodes"], "wins": r["wins"], "win_rate": round(r["win_rate"], 4),
                                  "ci95": [round(x, 4) for x in r["ci95"]], "engine": r["engine"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--skip_strength", action="store_true")
    a = ap.parse_args()
    part_a(a)
    if not a.skip_strength:
        part_b(a)


if __name__ == "__main__":
    main()
