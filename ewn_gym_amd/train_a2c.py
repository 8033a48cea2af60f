"""Command-line counterpart of the reference's train.py (argument names follow train.py:162-259
where they apply): A2C (or PPO: `python -m ewn_gym_amd.train_a2c PPO ...`; or SEARCH: distillation of the lookahead search,
ewn_gym_amd/distill.py; or SELFPLAY: the PUCT search playing itself, PuctSelfPlayTrainer) on VecEWN lanes instead of SubprocVecEnv workers, per-epoch evaluation
against minimax on the un-shaped env (train.py:66-117), best-model checkpointing.

  python -m ewn_gym_amd.train_a2c --num_envs 4096 --epoch_num 10 --timesteps_per_epoch 200000
  python -m torch.distributed.run --nproc-per-node 8 -m ewn_gym_amd.train_a2c ...   (one process per GPU, RCCL)
"""
import argparse
import json
import os
import time

import torch
import torch.distributed as dist

from .a2c import A2CTrainer, FusedA2CTrainer
from .sharding import all_reduce_counters, lane_range, lane_seeds
from .tournament import evaluate
from .vec_env import VecEWN


def _parser():
    ap = argparse.ArgumentParser(description="Trainer for EWN on VecEWN lanes (counterpart of the reference's train.py)")
    # train.py:174-184 selects the algorithm with a sub-command; A2C is the one built here
    ap.add_argument("algorithm", nargs="?", default="A2C", choices=["A2C", "PPO", "SEARCH", "SELFPLAY"],
                    help="train.py:174-184's sub-command; SEARCH: train toward the lookahead on the model's own critic (SearchDistillTrainer); "
                         "SELFPLAY: games of the PUCT search against itself, policy target the root visits, value target the result "
                         "(PuctSelfPlayTrainer, DESIGN.md 4q)")
    ap.add_argument("--search", default="lookahead", choices=["lookahead", "puct"],
                    help="SEARCH: the expert: the lookahead on the critic, or a PUCT search on both heads whose root visit distribution "
                         "is the policy target (predict_puct)")
    ap.add_argument("--sims", type=int, default=64, help="SEARCH --search puct, SELFPLAY: simulations per observation (0..4096)")
    ap.add_argument("--c_puct", type=float, default=1.5, help="SEARCH --search puct, SELFPLAY: the exploration constant")
    ap.add_argument("--fused", action="store_true",
                    help="SEARCH --search puct, SELFPLAY: the PUCT search in one kernel launch (ewn_puct_search, DESIGN.md 4r) instead of the "
                         "staged launches: the same targets bit for bit; not with --endgame_leaves")
    ap.add_argument("--leaves", type=int, default=1, metavar="N",
                    help="SEARCH --search puct, SELFPLAY: up to N leaves per tree and round in one kernel launch per search "
                         "(ewn_puct_search_wide, DESIGN.md 4u): about sims / N rounds instead of sims + 1, other trees than N = 1; not with "
                         "--endgame_leaves or --whole_games")
    ap.add_argument("--whole_games", action="store_true",
                    help="SELFPLAY: all games of an update in one kernel launch that refills a finished game's column with the next game "
                         "(ewn_puct_selfplay, DESIGN.md 4s): the same records bit for bit; --fused is then not read; not with --endgame_leaves")
    ap.add_argument("--noise_eps", type=float, default=0.25, help="SELFPLAY: the weight of the Dirichlet noise in the root's priors (0: none)")
    ap.add_argument("--noise_alpha", type=float, default=1.0,
                    help="SELFPLAY: the Dirichlet parameter (about 10 / the number of moves, AlphaZero's rule of thumb: a choice, not a measurement)")
    ap.add_argument("--temp_plies", type=int, default=8,
                    help="SELFPLAY: a game's first plies whose move is drawn in proportion to the root's visits; later ones play the most visited move")
    ap.add_argument("--max_plies", type=int, default=None,
                    help="SELFPLAY: record rows per game (default 80 on 5x5, 128 on 7x7: above the longest possible game)")
    ap.add_argument("--plies", type=int, default=1, choices=[1, 2], help="SEARCH: moves the lookahead looks ahead")
    ap.add_argument("--temperature", type=float, default=0.0,
                    help="SEARCH: 0 trains toward the search's action, > 0 toward the softmax of its Q / temperature")
    ap.add_argument("--terminal_value", type=float, default=1.0, help="SEARCH, SELFPLAY: the value of a won (+) or lost (-) position in the search")
    ap.add_argument("--endgame_table", default=None,
                    help="SEARCH: a saved EndgameTable; the search's q is replaced by the exact one wherever the table covers the position")
    ap.add_argument("--endgame_leaves", action="store_true",
                    help="SEARCH with --endgame_table: the search also values every leaf that the table covers by the table (DESIGN.md 4p)")
    ap.add_argument("--puct_table", default=None, metavar="PATH",
                    help="SELFPLAY: a saved EndgameTable; a leaf of the search that it covers is worth its exact value, a ply's search "
                         "stays one kernel launch (ewn_puct_search_eg, DESIGN.md 4w); --fused is then not read; not with --endgame_table, "
                         "--leaves above 1 or --whole_games")
    ap.add_argument("--games_table", default=None, metavar="PATH",
                    help="SELFPLAY: a saved EndgameTable; --puct_table's games with all of them in one kernel launch, finished columns "
                         "refilled (ewn_puct_selfplay_eg, DESIGN.md 4x); --fused and --whole_games are then not read; not with "
                         "--endgame_table, --puct_table or --leaves above 1")
    ap.add_argument("--batch_size", "-b", type=int, default=None,
                    help="PPO: minibatch size in samples of the n_steps x lanes rollout buffer (default: a quarter of it; train.py:178-183)")
    ap.add_argument("--n_epochs", type=int, default=10, help="PPO: passes over the rollout buffer per update (SB3 default)")
    ap.add_argument("--trainer", default="auto", choices=["auto", "fused", "torch"],
                    help="fused: the whole loop in the engine (A2C: ewn_step_k_policy + ewn_a2c_grad / ewn_a2c_apply, five kernel launches per "
                         "update; PPO: ewn_step_k_policy + ewn_ppo_prepare / _shuffle / _grad / _apply, one hipGraph per update); torch: torch "
                         "policy forward per step + ewn_step, autograd update; auto: A2C fused where the engine has it, PPO the torch trainer")
    ap.add_argument("--checkpoint", default=None, help="path of a checkpoint written by this trainer to resume from (train.py:137-139, 248-251)")
    ap.add_argument("--model_seed", type=int, default=None, help="seed of the policy initialisation and sampling (default: --env_seed)")
    ap.add_argument("--num_envs", "-ne", type=int, default=4096, help="lanes per GPU")
    ap.add_argument("--n_steps", "-n", type=int, default=5)
    ap.add_argument("--learning_rate", "-lr", type=float, default=3e-4)
    ap.add_argument("--epoch_num", "-e", type=int, default=10)
    ap.add_argument("--timesteps_per_epoch", "-t", type=int, default=200000)
    ap.add_argument("--eval_episode_num", "-ee", type=int, default=256)
    ap.add_argument("--eval_max_depth", type=int, default=5)
    ap.add_argument("--eval_opponent", default="minimax", choices=["minimax", "mcts", "random"],
                    help="opponent of the per-epoch evaluation (train.py evaluates against minimax; eval_A2C.py takes any of the three)")
    ap.add_argument("--eval_num_simulations", type=int, default=10, help="--eval_opponent mcts: simulations per root move (x 5 env copies)")
    ap.add_argument("--board_size", type=int, default=5)
    ap.add_argument("--cube_layer", type=int, default=3)
    ap.add_argument("--opponent_policy", "-op", default="random",
                    help="random, minimax, mcts; or self-play with the fused trainers: 'self' (a frozen copy of the live parameters) or the "
                         "path of a checkpoint (loaded once)")
    ap.add_argument("--opponent_update_every", type=int, default=100, help="--opponent_policy self: refresh the frozen copy every N updates")
    ap.add_argument("--max_depth", type=int, default=3)
    ap.add_argument("--goal_reward", type=float, default=10.0)
    ap.add_argument("--illegal_move_reward", type=float, default=-1.0)
    ap.add_argument("--illegal_move_tolerance", type=int, default=10)
    ap.add_argument("--reference_quirks", action="store_true",
                    help="reproduce MinimaxEnv's ctor-argument dropping: RandomAgent opponent, reward 1.0 (SURVEY App. D1)")
    ap.add_argument("--seed", "--env_seed", dest="seed", type=int, default=9487)
    ap.add_argument("--save_dir", default="models")
    return ap


def main():
    ap = _parser()
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    if a.algorithm == "SEARCH" and (a.trainer == "torch" or a.batch_size is not None):
        raise SystemExit("SEARCH has one trainer, SearchDistillTrainer, whose update is one full batch in the engine: --trainer torch and "
                         "--batch_size do not apply to it (--n_epochs is PPO's and is not read)")
    if a.algorithm == "SELFPLAY":
        if a.trainer == "torch" or a.batch_size is not None or a.opponent_policy != "random":
            raise SystemExit("SELFPLAY has one trainer, PuctSelfPlayTrainer: the search plays itself and the update is one full batch in the "
                             "engine, so --trainer torch, --batch_size and --opponent_policy do not apply to it")
        unread = [name for name in ("n_steps", "opponent_update_every", "max_depth", "goal_reward", "illegal_move_reward",
                                    "illegal_move_tolerance", "reference_quirks") if getattr(a, name) != ap.get_default(name)]
        if unread:
            raise SystemExit("SELFPLAY plays whole games of the search against itself and trains on their results: it reads no rollout "
                             "length, opponent or reward, so --%s do(es) not apply to it" % ", --".join(unread))
        if (a.endgame_table is None) != (not a.endgame_leaves):
            raise SystemExit("SELFPLAY trains toward visits and results: a table serves it at the search's leaves only, "
                             "--endgame_table PATH --endgame_leaves")
    if a.search != "lookahead" and a.algorithm != "SEARCH":
        raise SystemExit("--search is read by SEARCH only")
    if a.fused and not (a.algorithm == "SELFPLAY" or (a.algorithm == "SEARCH" and a.search == "puct")):
        raise SystemExit("--fused is read by SEARCH --search puct and by SELFPLAY only")
    if a.fused and a.endgame_leaves:
        raise SystemExit("--fused does not go with --endgame_leaves: the exact-leaf substitution is the staged search's")
    if a.leaves != 1 and not (a.algorithm == "SELFPLAY" or (a.algorithm == "SEARCH" and a.search == "puct")):
        raise SystemExit("--leaves is read by SEARCH --search puct and by SELFPLAY only")
    if not 1 <= a.leaves <= 32:
        raise SystemExit("--leaves takes 1..32")
    if a.leaves != 1 and (a.endgame_leaves or a.whole_games):
        raise SystemExit("--leaves %d does not go with --endgame_leaves or --whole_games: both evaluate one leaf per tree and round" % a.leaves)
    if a.whole_games and a.algorithm != "SELFPLAY":
        raise SystemExit("--whole_games is read by SELFPLAY only")
    if a.whole_games and a.endgame_leaves:
        raise SystemExit("--whole_games does not go with --endgame_leaves: the exact-leaf substitution is the staged search's")
    if a.puct_table is not None and a.algorithm != "SELFPLAY":
        raise SystemExit("--puct_table is read by SELFPLAY only")
    if a.puct_table is not None and (a.endgame_table is not None or a.leaves != 1 or a.whole_games):
        raise SystemExit("--puct_table does not go with --endgame_table, --leaves above 1 or --whole_games: it is the one launch of the "
                         "search with exact leaves")
    if a.games_table is not None and a.algorithm != "SELFPLAY":
        raise SystemExit("--games_table is read by SELFPLAY only")
    if a.games_table is not None and (a.endgame_table is not None or a.puct_table is not None or a.leaves != 1):
        raise SystemExit("--games_table does not go with --endgame_table, --puct_table or --leaves above 1: it is the one launch of whole "
                         "games with exact leaves")
    if a.endgame_table is not None and a.algorithm not in ("SEARCH", "SELFPLAY"):
        raise SystemExit("--endgame_table is read by SEARCH and SELFPLAY only")
    if a.endgame_leaves and (a.algorithm not in ("SEARCH", "SELFPLAY") or a.endgame_table is None):
        raise SystemExit("--endgame_leaves goes with SEARCH or SELFPLAY and --endgame_table")
    lo, hi = lane_range(a.num_envs * world, world, rank)
    if a.reference_quirks and a.opponent_policy not in ("random", "minimax", "mcts"):
        raise SystemExit("--reference_quirks drops the opponent (MinimaxEnv plays RandomAgent whatever it is given): it cannot be combined "
                         "with a model opponent, --opponent_policy %s" % a.opponent_policy)
    opp, reward = (("random", 1.0) if a.reference_quirks else (a.opponent_policy, a.goal_reward))
    model_opp = None
    if opp not in ("random", "minimax", "mcts"):   # a model opponent: the rollout kernel plays it, the env's own opponent is not used
        model_opp, opp = opp, "random"
        if a.algorithm != "SEARCH" and (a.trainer == "torch" or (a.algorithm == "PPO" and a.trainer != "fused")):
            raise SystemExit("--opponent_policy %s: a model opponent is played by the fused trainers only (--trainer fused); the torch "
                             "trainers step the env with ewn_step, which has no policy opponent" % model_opp)
    okw = {} if model_opp is None else dict(opponent=model_opp, opponent_update_every=a.opponent_update_every)
    env = VecEWN(a.num_envs, board_size=a.board_size, cube_layer=a.cube_layer, opponent_policy=opp, max_depth=a.max_depth,
                 rng="philox", shaped=True, reward=reward, illegal_move_reward=a.illegal_move_reward,
                 illegal_move_tolerance=a.illegal_move_tolerance, autoreset=True, lane_offset=lo,
                 seed_stride=a.num_envs * world, philox_key=a.seed, shaped_refresh_on_reset=not a.reference_quirks)
    env.reset(seeds=lane_seeds(lo, hi, a.seed).cuda())
    mseed = a.seed if a.model_seed is None else a.model_seed
    if a.algorithm == "PPO":   # train.py:39-49: SB3's PPO with batch_size and learning_rate given, the rest at its defaults (ewn_gym_amd/ppo.py)
        from .ppo import FusedPPOTrainer, PPOTrainer
        cls = FusedPPOTrainer if a.trainer == "fused" else PPOTrainer   # auto keeps the torch trainer for PPO
        trainer = cls(env, n_steps=a.n_steps, batch_size=a.batch_size, n_epochs=a.n_epochs, learning_rate=a.learning_rate, seed=mseed,
                      **okw)
    elif a.algorithm == "SEARCH":
        from .distill import SearchDistillTrainer
        trainer = SearchDistillTrainer(env, n_steps=a.n_steps, learning_rate=a.learning_rate, temperature=a.temperature, plies=a.plies,
                                       terminal_value=a.terminal_value, seed=mseed, endgame_table=a.endgame_table, search=a.search,
                                       sims=a.sims, c_puct=a.c_puct, endgame_leaves=a.endgame_leaves, fused=a.fused, leaves=a.leaves, **okw)
    elif a.algorithm == "SELFPLAY":
        from .distill import PuctSelfPlayTrainer
        trainer = PuctSelfPlayTrainer(env, sims=a.sims, c_puct=a.c_puct, terminal_value=a.terminal_value, noise_eps=a.noise_eps,
                                      noise_alpha=a.noise_alpha, temp_plies=a.temp_plies, max_plies=a.max_plies,
                                      learning_rate=a.learning_rate, seed=mseed, endgame_table=a.endgame_table, fused=a.fused,
                                      whole_games=a.whole_games, leaves=a.leaves, leaf_table=a.puct_table,
                                      games_table=a.games_table)
    elif a.trainer == "fused" or model_opp is not None or (a.trainer == "auto" and env.supports_policy_rollout()):
        trainer = FusedA2CTrainer(env, n_steps=a.n_steps, learning_rate=a.learning_rate, seed=mseed, **okw)
    else:
        trainer = A2CTrainer(env, n_steps=a.n_steps, learning_rate=a.learning_rate, seed=mseed)
    if a.checkpoint is not None:      # train.py:137-139: resume the model (and here the optimiser and the step counter too)
        trainer.load(a.checkpoint)
        if rank == 0:
            print(json.dumps({"resumed_from": a.checkpoint, "timesteps": trainer.num_timesteps * world}), flush=True)
    if rank == 0:
        print(json.dumps({"trainer": type(trainer).__name__, "lanes_per_gpu": a.num_envs, "world": world}), flush=True)
    best = trainer.best_score   # -1 for a fresh run; a resumed one keeps its best model until it is beaten
    for epoch in range(a.epoch_num):
        stats = trainer.learn(a.timesteps_per_epoch // world)   # dict of the last update's statistics
        # train.py:73-81: evaluate on the UN-shaped env against minimax(depth 5) (or --eval_opponent), seeds 0..n-1, deterministic
        # actions (the model's argmax in the engine, ewn_policy_eval / ewn_policy_eval_mcts, where it serves the configuration; else per step)
        n_eval = a.eval_episode_num // world
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eval_opp = {"kind": a.eval_opponent, "max_depth": a.eval_max_depth, "num_simulations": a.eval_num_simulations}
        r = evaluate({"kind": "mlp", "model": trainer.model}, eval_opp, num=n_eval,
                     board_size=a.board_size, cube_layer=a.cube_layer, rng="mt19937", seed_offset=rank * n_eval)
        eval_s = time.perf_counter() - t0    # evaluate() ends on a host sync (its win count)
        c = all_reduce_counters(torch.tensor([r["wins"], r["episodes"]], dtype=torch.int64, device="cuda"))
        win_rate = c[0].item() / max(1, c[1].item())
        if rank == 0:
            print(json.dumps({"epoch": epoch, "timesteps": trainer.num_timesteps * world, "win_rate": win_rate, **stats,
                              "eval_engine": r["engine"], "eval_s": eval_s}), flush=True)
            if win_rate > best:          # train.py:109-112
                best = trainer.best_score = win_rate
                os.makedirs(a.save_dir, exist_ok=True)
                trainer.save(os.path.join(a.save_dir, "best.pt"))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
