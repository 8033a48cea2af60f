"""Wall time of the trainer's per-epoch evaluation (train.py:66-117): a trained policy's argmax vs minimax(5), MT19937-compat dice,
seeds 0..n-1, on both paths -- in the engine (ewn_policy_eval, K steps per launch) and per step (model.act + ewn_step per ply).

    python tools/eval_policy_time.py [--board_size 5] [--nums 256 1024] [--reps 5]
    python tools/eval_policy_time.py --opponent mcts [--num_simulations 10] [--num_env_copies 5]

--opponent mcts: the same two paths against the flat Monte-Carlo opponent (eval_A2C.py --opponent_policy mcts): ewn_policy_eval_mcts
against evaluate(use_rollout=False), and the per-episode results of the two must be equal -- except for an episode on whose per-step
trajectory some head's two best logits lie within 2e-5 of each other (the engine's bf16 x 3 logits agree with torch's to 1e-5, so such
a step may be decided either way, and the episode goes another way from there).

--opponent model: a second trained policy as the opponent (both sides play their argmax): ewn_policy_eval_vs against the only other way
to play it, a ply-by-ply loop written here from vec_env.apply_action / legal_actions and torch forwards (one host sync per ply, like
the per-step path).  The loop draws its dice from torch, so the two paths play different games: their win rates agree statistically.

The policy is a FusedA2CTrainer trained briefly against RandomAgent (an untrained one forfeits at its first move).  EWN_EVAL_NT=64 / 256
in the environment forces the evaluation kernel's block size.  One JSON line per (path, episodes): median of --reps calls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate  # noqa: E402


NEAR_TIE = 2e-5


def min_gaps(model, opp, num, S):
    """the smallest top-two logit gap (either head) each episode meets on the per-step path: evaluate()'s env and loop, watched"""
    env = ea.VecEWN(num, board_size=S, opponent_policy=opp["kind"], num_simulations=opp["num_simulations"],
                    num_env_copies=opp["num_env_copies"], rng="mt19937", autoreset=False, philox_key=12345 ^ 0x5DEECE66D)
    env.reset(seeds=torch.arange(num, dtype=torch.int32))
    gap = torch.full((num,), float("inf"), device="cuda")
    for _ in range(400):
        alive = env.done == 0
        if not bool(alive.any()):
            break
        with torch.no_grad():
            l0, l1, _ = model(env.board, env.dice)
        for lg in (l0, l1):
            top = lg.topk(2, dim=1).values
            gap = torch.where(alive, torch.minimum(gap, top[:, 0] - top[:, 1]), gap)
        env.step(torch.stack([l0.argmax(1), l1.argmax(1)], 1).to(torch.int8))
    return gap


def ply_by_ply(agent, opp, num, S, seed=0):
    """model against model without the engine's step: envs/ewn.py:436-486 from the stateless calls, torch dice"""
    from ewn_gym_amd import vec_env as ve
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    roll = lambda: torch.randint(1, 7, (num,), device="cuda", generator=g).to(torch.int8)   # noqa: E731
    env = ea.VecEWN(1, board_size=S, opponent_policy="random", rng="philox")
    env.reset(seeds=torch.zeros(1, dtype=torch.int32))
    board, dice = env.board[0][None].repeat(num, 1, 1).contiguous(), roll()
    alive = torch.ones(num, dtype=torch.bool, device="cuda")
    score = torch.zeros(num, dtype=torch.float64, device="cuda")
    length = torch.zeros(num, dtype=torch.int32, device="cuda")
    for _ in range(400):
        if not bool(alive.any()):
            break
        with torch.no_grad():
            l0, l1, _ = agent(board, dice)
        nb, valid = ve.apply_action(board, dice, torch.stack([l0.argmax(1), l1.argmax(1)], 1).to(torch.int8), player=1)
        inval = alive & (valid == 0)
        won = alive & ~inval & (ve.legal_actions(nb, dice, player=2)[4] != 0)
        reply = alive & ~inval & ~won
        od = roll()
        view = (-nb.reshape(num, -1).flip(1)).reshape(num, S, S).contiguous()
        with torch.no_grad():
            o0, o1, _ = opp(view, od)
        nb2, valid2 = ve.apply_action(nb, od, torch.stack([o0.argmax(1), o1.argmax(1)], 1).to(torch.int8), player=2)
        oinval = reply & (valid2 == 0)
        lost = reply & ~oinval & (ve.legal_actions(nb2, od, player=1)[4] != 0)
        score = torch.where(won, torch.ones_like(score), torch.where(inval | lost, -torch.ones_like(score), score))
        length += alive.to(torch.int32)
        go = reply & ~oinval & ~lost
        board = torch.where(go[:, None, None], nb2, board)
        dice = torch.where(go, roll(), dice)
        alive = go
    wins = int((score > 0).sum())
    return {"engine": "ply_by_ply", "win_rate": wins / num, "avg_length": float(length.float().mean()), "scores": score, "lengths": length}


def model_vs_model(a):
    S, N = a.board_size, 4096
    models = []
    for seed, updates in ((0, a.updates), (1, a.updates // 2)):
        env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=10,
                        autoreset=True, shaped_refresh_on_reset=True, philox_key=1 + seed)
        env.reset(seeds=torch.arange(N, dtype=torch.int32))
        tr = FusedA2CTrainer(env, n_steps=5, learning_rate=1e-3, seed=seed)
        for _ in range(updates):
            tr.collect_and_update()
        torch.cuda.synchronize()
        models.append(tr.model)
    agent, opp = models
    paths = (("ewn_policy_eval_vs", lambda num: evaluate({"kind": "mlp", "model": agent}, {"kind": "mlp", "model": opp}, num=num, board_size=S)),
             ("ply_by_ply", lambda num: ply_by_ply(agent, opp, num, S)))
    for num in a.nums:
        for name, fn in paths:
            fn(num)
            ts, r = [], None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn(num)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert r["engine"] == name, (r["engine"], name)
            ts.sort()
            print(json.dumps({"path": name, "episodes": num, "board_size": S, "opponent": "model", "median_s": ts[len(ts) // 2], "min_s": ts[0],
                              "max_s": ts[-1], "win_rate": r["win_rate"], "avg_length": r["avg_length"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board_size", type=int, default=5)
    ap.add_argument("--nums", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=600)
    ap.add_argument("--max_depth", type=int, default=5)
    ap.add_argument("--opponent", default="minimax", choices=["minimax", "mcts", "model"])
    ap.add_argument("--num_simulations", type=int, default=10)
    ap.add_argument("--num_env_copies", type=int, default=5)
    a = ap.parse_args()
    if a.opponent == "model":
        return model_vs_model(a)
    S, N = a.board_size, 4096
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=10,
                    autoreset=True, shaped_refresh_on_reset=True, philox_key=1)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    tr = FusedA2CTrainer(env, n_steps=5, learning_rate=1e-3, seed=0)
    for _ in range(a.updates):
        tr.collect_and_update()
    torch.cuda.synchronize()
    mcts = a.opponent == "mcts"
    opp = {"kind": "minimax", "max_depth": a.max_depth}
    paths = (("ewn_policy_eval", {"kind": "mlp", "model": tr.model}, {}), ("ewn_step", tr.policy_fn(True), {}))
    if mcts:
        opp = {"kind": "mcts", "num_simulations": a.num_simulations, "num_env_copies": a.num_env_copies}
        paths = (("ewn_policy_eval_mcts", {"kind": "mlp", "model": tr.model}, {}),
                 ("ewn_step", {"kind": "mlp", "model": tr.model}, {"use_rollout": False}))
    for num in a.nums:
        results = {}
        for name, agent, kw in paths:
            evaluate(agent, opp, num=num, board_size=S, **kw)           # warm-up: tables, kernels, allocator
            ts, r = [], None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = evaluate(agent, opp, num=num, board_size=S, **kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert r["engine"] == name, (r["engine"], name)
            ts.sort()
            results[name] = r
            if mcts:   # max_s: the spread of the calls decides whether one path is faster than the other
                row = {"path": name, "episodes": num, "board_size": S, "opponent": "mcts", "num_simulations": a.num_simulations,
                       "num_env_copies": a.num_env_copies, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1],
                       "win_rate": r["win_rate"], "avg_length": r["avg_length"]}
            else:      # the minimax rows as they have always been printed
                row = {"path": name, "episodes": num, "board_size": S, "opponent_depth": a.max_depth,
                       "eval_nt": os.environ.get("EWN_EVAL_NT", "auto"), "median_s": ts[len(ts) // 2], "min_s": ts[0],
                       "win_rate": r["win_rate"], "avg_length": r["avg_length"]}
            print(json.dumps(row), flush=True)
        if mcts:
            e, p = results["ewn_policy_eval_mcts"], results["ewn_step"]
            differ = (e["scores"] != p["scores"]) | (e["lengths"] != p["lengths"])
            n_differ = int(differ.sum())
            if n_differ:
                gap = min_gaps(tr.model, opp, num, S)
                assert bool((gap[differ] <= NEAR_TIE).all()), ("episodes differ between the paths without a near-tie on their way",
                                                               torch.nonzero(differ & (gap > NEAR_TIE)).reshape(-1).tolist())
            print(json.dumps({"episodes": num, "board_size": S, "episodes_differing_at_a_near_tie": n_differ}), flush=True)


if __name__ == "__main__":
    main()
