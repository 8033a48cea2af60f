#!/usr/bin/env python3
"""Supplement to gen_golden.py: the UNMODIFIED reference on the positions and configurations the deep search kernels are tested on
-> tests/golden/g15_deep_search.json, g16_deep_traj.json, g17_eval_loop_deep.json, g18_large_boards.json.

 * G15: ExpectiMinimaxAgent.expectiminimax at max_depth 1-6 on make_positions(S, 1024) of tests/test_gpu_search_keys.py (the set
   tests/test_gpu_search_d5.py runs through every kernel form; two thirds mid-game, one third thinned to 1-3 cubes a side), S = 5..8.
   The boards are not stored: the tests regenerate them and compare the sha256 kept here.
 * G16: EinsteinWuerfeltNichtEnv trajectories against a minimax opponent at depth 4-6 on 5x5 .. 8x8, in the format of G6.
 * G17: the evaluation loop of G10 (eval_minimax.py:16-50) with agent depth 4-6 on 5x5 and depth 3 / 5 on 7x7.
 * G18: heuristics, searches and trajectories on 9x9 (cube_layer 3), 10x10 (4) and 11x11 (5), built as G12 / G13 are.

The fixtures are kept small, since they are read with the rest of a change:
 * floats are C99 hex without float.hex()'s trailing zeros ("0x1.8p+1");
 * G15 keeps each board size's distinct root values once ("values") and, per key, the positions as ranges [lo, hi) ("idx") and one
   string of three characters per position ("out"): the action as the digit 3 a0 + a1, then the value's index in base 36;
 * a trajectory step is the row [a0, a1, dice, reward, terminated, truncated, message, [cell, cube, cell, cube, ...]]: the cells of
   the board that the step changed.  expand_traj() of tests/test_oracle_golden_deep.py rebuilds G6's format from it;
 * G18 keeps a board as [cell, cube, ...] of its occupied cells, and its searches point at the evaluated positions ("pos").

Same rules as gen_golden.py: container-only, runs the reference through the import stubs, calls its classes and copies none of its
text, writes data only (floats as C99 hex).  Minimax is deterministic and every random choice here is seeded: running it twice
gives identical bytes.  The work is spread over --jobs processes and assembled in a fixed order: about 5 minutes on 8 of them.

Usage:  python oracle/gen_golden_deep.py [--ref /root/reference] [--out tests/golden] [--jobs 8]
"""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

M_POS = 1024
THIN = 2 * M_POS // 3
SIZES = (5, 6, 7, 8)
OTHER = ("min_dist", "attk", "two_min_dist")
INF = float("inf")
B36 = "0123456789abcdefghijklmnopqrstuvwxyz"

G16 = ((5, 3, 6, "hybrid", 4), (6, 3, 5, "hybrid", 4), (6, 3, 4, "attk", 4), (6, 3, 5, "two_min_dist", 2), (7, 3, 5, "hybrid", 3),
       (7, 3, 4, "two_min_dist", 3), (8, 3, 4, "min_dist", 3), (8, 3, 5, "hybrid", 2), (8, 3, 6, "hybrid", 1))
# board size, agent depth, opponent, opponent depth, episodes
G17 = ((5, 4, "random", None, 32), (5, 5, "random", None, 16), (5, 5, "minimax", 3, 8), (5, 6, "random", None, 4),
       (7, 3, "random", None, 16), (7, 5, "random", None, 4))
G18 = ((9, 3, 9803), (10, 4, 10804), (11, 5, 11805))     # board size, cube_layer, seed of the self-play that makes the positions


def fhex(x):
    m, e = float(x).hex().split("p")        # every value here is finite
    return m.rstrip("0").rstrip(".") + "p" + e


def sparse(board):
    """[cell, cube, cell, cube, ...] of the occupied cells"""
    return [int(x) for c, v in enumerate(board.reshape(-1)) if v for x in (c, v)]


def ranges(idx):
    """[[lo, hi), ...] of an index list made of ascending runs"""
    out = []
    for i in idx:
        if out and out[-1][1] == i:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1])
    return out


def g15_keys():
    """key "depth/heuristic" -> indices into make_positions(S, 1024)"""
    thinned, mid = list(range(THIN, M_POS)), list(range(64))
    keys = {"5/hybrid": list(range(M_POS)), "6/hybrid": mid + thinned}
    for d in (1, 2, 3, 4):
        keys["%d/hybrid" % d] = thinned
    for h in OTHER:
        for d in (3, 4, 5):
            keys["%d/%s" % (d, h)] = mid + list(range(THIN, THIN + 128))
        keys["6/%s" % h] = list(range(THIN + 128, THIN + 176))
    return keys


# ---- what the worker processes share: the reference's modules and the positions, set up in main() before the pool forks
R = {}


def B(env):
    return [int(v) for v in env.board.reshape(-1)]


def search(agent, board, dice, depth):
    """[a0, a1, value] of the reference's search from an observation the agent has not won, cross-checked with predict()"""
    obs = {"board": board, "dice_roll": dice}
    agent.restore_env_with_obs(obs)
    assert not agent.env.check_win()
    val, act = agent.expectiminimax(depth, agent.env.agent_player, None, -INF, INF)
    pact, _ = agent.predict(obs)
    assert list(pact) == list(act)
    return [int(act[0]), int(act[1]), fhex(val)]


def job_g15(task):
    S, key, idx = task
    depth, heur = key.split("/")
    agent = R["cp"].ExpectiMinimaxAgent(int(depth), 3, S, heuristic=heur)
    b, d = R["pos"][S]
    return [search(agent, b[i].astype(int), int(d[i]), int(depth)) for i in idx]


def run_traj(env, seed, rule, max_steps=200):
    np = R["np"]
    obs, _ = env.reset(seed=seed)
    rec = {"seed": seed, "board0": B(env), "dice0": int(obs["dice_roll"]), "steps": []}
    t, done, before = 0, False, rec["board0"]
    while not done and t < max_steps:
        a = rule(env, t)
        obs, r, term, trunc, info = env.step(np.array(a))
        after = B(env)
        changed = [x for c, (u, v) in enumerate(zip(before, after)) if u != v for x in (c, v)]
        rec["steps"].append([int(a[0]), int(a[1]), int(obs["dice_roll"]), fhex(r), bool(term), bool(trunc), info.get("message"), changed])
        before = after
        done = term
        t += 1
    return rec


def rule_kth(seed):
    def rule(env, t):
        acts = env.get_legal_actions(env.current_player)
        return acts[(seed + t) % len(acts)]
    return rule


def rule_kth_or_raw(seed):
    """as gen_golden_maxboard.py: now and then a raw, possibly illegal action"""
    def rule(env, t):
        acts = env.get_legal_actions(env.current_player)
        return acts[(seed + t) % len(acts)] if (seed + t) % 11 else [int(t % 2), int((seed + t) % 3)]
    return rule


def job_g16(task):
    S, L, depth, heur, seed = task
    env = R["envs"].EinsteinWuerfeltNichtEnv(board_size=S, cube_layer=L, opponent_policy=R["Policy"].minimax, max_depth=depth, heuristic=heur)
    rec = run_traj(env, seed, rule_kth(seed))
    rec.update({"S": S, "L": L, "rule": "kth", "opp": "minimax", "depth": depth, "heuristic": heur})
    return rec


def job_g17(task):
    S, adepth, opp, odepth, nseed = task
    kw = {} if odepth is None else {"max_depth": odepth}
    env = R["envs"].EinsteinWuerfeltNichtEnv(board_size=S, cube_layer=3, opponent_policy=getattr(R["Policy"], opp), **kw)
    model = R["cp"].ExpectiMinimaxAgent(adepth, 3, S)
    scores, lengths = [], []
    for seed in range(nseed):
        obs, info = env.reset(seed=seed)
        done, n, reward = False, 0, 0
        while not done:
            action, _ = model.predict(obs, deterministic=True)
            obs, reward, done, _, info = env.step(action)
            n += 1
        scores.append(float(reward))
        lengths.append(n)
    return {"S": S, "agent_depth": adepth, "opp": opp, "opp_depth": odepth, "scores": scores, "lengths": lengths}


def job_g18(task):
    S, L, seed = task
    np, envs, cp, Player, Policy = R["np"], R["envs"], R["cp"], R["Player"], R["Policy"]
    gen = np.random.Generator(np.random.PCG64(seed))
    positions, picked = [], []      # every third position of the self-play, and the won position each game ends in
    for g in range(4):
        env = envs.MinimaxEnv(board_size=S, cube_layer=L)
        env.reset(seed=int(gen.integers(0, 2**31)))
        player, plies = Player.TOP_LEFT, 0
        while not env.check_win() and plies < 90:
            dice = int(gen.integers(1, 7))      # the search's dice loop runs 1..6 whatever the cube count: predict() handles no other
            env.set_dice_roll(dice)
            if len(positions) % 3 == 0:
                picked.append(len(positions))
            positions.append((env.board.copy(), dice, player))
            acts = env.get_legal_actions(player)
            env.make_simulated_action(player, acts[int(gen.integers(0, len(acts)))])
            player = Player.get_opponent(player)
            plies += 1
        if env.check_win():     # every won position: heuristics only
            picked.append(len(positions))
            positions.append((env.board.copy(), int(gen.integers(1, 7)), player))
    keys = [(d, h) for d in (1, 2, 3) for h in ("hybrid", "attk")] + [(4, "hybrid")]
    agents = {k: cp.ExpectiMinimaxAgent(k[0], L, S, heuristic=k[1]) for k in keys}
    ev = cp.ExpectiMinimaxAgent(1, L, S)
    # "eval": [cells, hybrid, min_dist, two_min_dist, attk] per position; "minimax": the positions nobody has won, by their index in
    # "eval", their dice and [a0, a1, value] per key -- "4/hybrid" on the first 10 of them only
    grp = {"S": S, "L": L, "eval": [], "minimax": {"pos": [], "dice": [], "res": {"%d/%s" % k: [] for k in keys}}, "traj": []}
    mm = grp["minimax"]
    for board, dice, player in (positions[i] for i in picked):
        if player != Player.TOP_LEFT:
            board = np.rot90(-board, 2).copy()
        ev.restore_env_with_obs({"board": board, "dice_roll": dice})
        grp["eval"].append([sparse(board)] + [fhex(ev.env.evaluate(h)) for h in ("hybrid", "min_dist", "two_min_dist", "attk")])
        if ev.env.check_win():
            continue
        for k in keys if len(mm["pos"]) < 10 else keys[:-1]:
            mm["res"]["%d/%s" % k].append(search(agents[k], board, dice, k[0]))
        mm["pos"].append(len(grp["eval"]) - 1)
        mm["dice"].append(dice)
    for opp, depth, nseed in (("random", None, 4), ("minimax", 2, 2), ("minimax", 3, 2)):
        kw = {} if depth is None else {"max_depth": depth, "heuristic": "hybrid"}
        env = envs.EinsteinWuerfeltNichtEnv(board_size=S, cube_layer=L, opponent_policy=getattr(Policy, opp), **kw)
        for seed in range(nseed):
            rec = run_traj(env, seed, rule_kth_or_raw(seed))
            rec.update({"S": S, "L": L, "opp": opp})
            if depth is not None:
                rec.update({"depth": depth, "heuristic": "hybrid"})
            grp["traj"].append(rec)
    return grp


JOBS = {"g15": job_g15, "g16": job_g16, "g17": job_g17, "g18": job_g18}


def run_job(item):
    kind, task = item
    return JOBS[kind](task)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    if not os.path.isdir(args.ref):
        print("reference not present; nothing to do")
        return 0
    t0 = time.time()
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(HERE, "ref_import_stubs"))
    sys.path.insert(0, args.ref)
    sys.path.append(ROOT)       # behind the reference: `envs`, `classical_policies` and `constants` must be the reference's
    import numpy as np
    import envs
    import classical_policies as cp
    from constants import Player, ClassicalPolicy
    assert os.path.dirname(os.path.abspath(envs.__file__)).startswith(os.path.abspath(args.ref)), envs.__file__
    from tests.test_gpu_search_keys import make_positions
    R.update(np=np, envs=envs, cp=cp, Player=Player, Policy=ClassicalPolicy, pos={S: make_positions(S, M_POS) for S in SIZES})

    # ---- the list of jobs, in the order the results are assembled in: the whole games first (the longest jobs), the searches in chunks
    keys = g15_keys()
    items = [("g17", t) for t in G17]
    items += [("g16", (S, L, depth, heur, seed)) for S, L, depth, heur, nseed in G16 for seed in range(nseed)]
    items += [("g18", t) for t in G18]
    for S in SIZES:
        for key, idx in keys.items():
            step = 32 if key[0] in "56" else 128
            items += [("g15", (S, key, idx[i:i + step])) for i in range(0, len(idx), step)]
    with mp.get_context("fork").Pool(args.jobs) as pool:
        results = pool.map(run_job, items, chunksize=1)
    by_kind = {k: [(it[1], r) for it, r in zip(items, results) if it[0] == k] for k in JOBS}

    os.makedirs(args.out, exist_ok=True)

    def dump(name, obj, what):
        p = os.path.join(args.out, name)
        with open(p, "w") as f:
            json.dump(obj, f, separators=(",", ":"))
        print(name, os.path.getsize(p), "bytes;", what)

    g15 = {"n": M_POS, "thin": THIN, "sizes": {}}
    for S in SIZES:
        b, d = R["pos"][S]
        res = {key: {"idx": ranges(idx), "out": ""} for key, idx in keys.items()}
        values = {}         # a distinct root value -> its index, in the order of first appearance
        for (s, key, idx), out in by_kind["g15"]:
            if s != S:
                continue
            for a0, a1, v in out:
                i = values.setdefault(v, len(values))
                res[key]["out"] += "%d%s%s" % (3 * a0 + a1, B36[i // 36], B36[i % 36])
        assert all(len(keys[key]) * 3 == len(r["out"]) for key, r in res.items()) and len(values) <= 36 * 36
        g15["sizes"][str(S)] = {"sha256": hashlib.sha256(b.astype(np.int8).tobytes() + d.astype(np.int8).tobytes()).hexdigest(),
                                "values": list(values), "res": res}
    dump("g15_deep_search.json", g15, "%d searches" % sum(len(r["out"]) // 3 for s in g15["sizes"].values() for r in s["res"].values()))
    g16 = [r for _, r in by_kind["g16"]]
    dump("g16_deep_traj.json", g16, "%d trajectories, %d steps" % (len(g16), sum(len(r["steps"]) for r in g16)))
    g17 = [r for _, r in by_kind["g17"]]
    dump("g17_eval_loop_deep.json", g17, "%d episodes, %d agent moves" % (sum(len(r["scores"]) for r in g17), sum(sum(r["lengths"]) for r in g17)))
    g18 = [r for _, r in by_kind["g18"]]
    dump("g18_large_boards.json", g18, "%d evaluations, %d search positions, %d trajectories, %d steps" % (
        sum(len(g["eval"]) for g in g18), sum(len(g["minimax"]["pos"]) for g in g18), sum(len(g["traj"]) for g in g18),
        sum(len(r["steps"]) for g in g18 for r in g["traj"])))
    print("wall time %.0f s on %d processes" % (time.time() - t0, args.jobs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
