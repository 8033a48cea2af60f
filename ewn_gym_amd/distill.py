"""Train on the search: expert iteration with the lookahead on the network's own critic as the expert.

The reference's AlphaZero fork trains a network toward what its search finds; its weights are not vendored, the idea is.  Here the
search is ewn_predict_lookahead (one or two moves ahead on the value net): the policy head is trained toward the
search's action, the critic toward the search's value, which bootstraps from the real terminal values (+-terminal_value) through
its own leaves.  One update:
    rollout with the current policy (ewn_step_k_policy: only the visited observations are used, not the rewards)
    -> predict_lookahead on the n_steps x lanes observations [with the table's exact values at the leaves it covers, 4p]
       [-> the exact q where an endgame table covers the position, 4n]
    -> ewn_lookahead_targets -> ewn_sup_grad
    -> [all-reduce of the flat gradient] -> ewn_a2c_apply (global-norm clip + RMSprop).
search="puct"  puts predict_puct in the search's place and AlphaZero's target in the target's: the policy heads are
trained toward the root's visit distribution (puct_targets), the critic toward the root's value.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._args import _finite, _not_negative, _positive, _ptr, _stream
from ._lib import check
from .a2c import FusedTrainer
from .endgame import EndgameTable, _accept_table
from .games import selfplay_puct_games
from .games_exact import _games_table_alone, selfplay_puct_games_exact
from .search import (SELFPLAY_MAX_PLIES, _leaf_table_alone, _noise_eps, _play_numbers, _puct_numbers, lookahead_targets, predict_lookahead,
                     predict_puct, selfplay_puct, sup_grad)
from .sharding import all_reduce_counters
from .wide import _NO_TABLE, _NO_WHOLE_GAMES, _leaves_alone


def puct_targets(visits, q, value, terminal_value=1.0, one_cube=None):
    """predict_puct's visits, q and value as training targets (plain torch, six numbers per row): visits [M, 2, 3], q float32
    [M, 2, 3], value float32 [M] -> (target_pi float32 [M, 5], target_value float32 [M], weight float32 [M]).  The flag head's target
    is sum_r visits / sum, the direction head's sum_f visits / sum; where both flags name one cube (flag 1 has no action of its own:
    its q row is all -inf) the flag head gets (0.5, 0.5), lookahead_targets' convention.  target_value = terminal_value * value.
    A row without visits (degenerate, or sims=0) gets zeros and weight 0.  q None (self-play records hold no q): one_cube bool [M]
    says where both flags name one cube (both_flags_one_cube)."""
    if q is None and one_cube is None:
        raise ValueError("puct_targets: without q, one_cube must say where both flags name one cube (both_flags_one_cube(boards, dice))")
    v = visits.reshape(-1, 2, 3).to(torch.float32)
    tot = v.sum((1, 2))
    live = tot > 0
    den = torch.where(live, tot, torch.ones_like(tot))[:, None]
    flag, direction = v.sum(2) / den, v.sum(1) / den
    same = live & ((q.reshape(-1, 2, 3)[:, 1] == float("-inf")).all(1) if q is not None else one_cube.reshape(-1))
    flag = torch.where(same[:, None], torch.full_like(flag, 0.5), flag)
    target_pi = torch.cat([flag, direction], 1) * live[:, None]
    target_value = torch.where(live, float(terminal_value) * value.reshape(-1), torch.zeros_like(tot))
    return target_pi.contiguous(), target_value.contiguous(), live.to(torch.float32)


class _SupervisedTrainer(FusedTrainer):
    """What the trainers on ewn_sup_grad share: the checks of the loss coefficients and of the endgame table, the optimiser's state
    and the gradient's scratch, the update on given rows and targets, and the statistics and checkpoint keys that both have.  A
    subclass's `_launch` collects its rows and targets and ends in `_update`."""

    def __init__(self, who, env, *, sims, c_puct, terminal_value, fused, pi_coef, vf_coef, endgame_table, learning_rate, max_grad_norm,
                 rms_alpha, rms_eps, leaves=1, **trainer):
        """who: the subclass, as its errors name it; an endgame_table that is not an EndgameTable is the path of one and is loaded
        onto the env's GPU; trainer: FusedTrainer's arguments after env.  The subclass then calls _size_scratch"""
        self.pi_coef, self.vf_coef = _not_negative(who, "pi_coef", pi_coef), _not_negative(who, "vf_coef", vf_coef)
        if endgame_table is not None:
            if not isinstance(endgame_table, EndgameTable):
                endgame_table = EndgameTable.load(endgame_table, device=env.board.device)
            _accept_table(who, endgame_table, env.S, "the endgame table is for %%dx%%d boards, the env plays %dx%d" % (env.S, env.S))
        self.endgame_table = endgame_table
        super().__init__(env, **trainer)
        self.sq_avg = torch.zeros_like(self.params)
        self.sims, self.c_puct, self.terminal_value, self.fused = int(sims), float(c_puct), float(terminal_value), bool(fused)
        self.leaves = int(leaves)          # > 1: the PUCT search as the one launch of ewn_puct_search_wide (4u), other trees than 1
        # the optimiser step is ewn_a2c_apply: of this struct it reads max_grad_norm, learning_rate, rms_alpha, rms_eps, world_size
        self.hyper = _lib.EwnA2cHyper(0.0, float(vf_coef), 0.0, float(max_grad_norm), float(learning_rate), float(rms_alpha), float(rms_eps),
                                      int(self.world))

    def _size_scratch(self, rows):
        """rows: the observations per lane of one update; they size ewn_sup_grad's scratch and are live_fraction's denominator"""
        self._rows = rows
        nscr = check(self.lib.ewn_sup_scratch_bytes(self.env.S, self.env.L, rows * self.env.N), "ewn_sup_scratch_bytes")
        self.scratch = torch.zeros(int(nscr), dtype=torch.uint8, device=self.device)

    def _update(self, boards, dice, target_pi, target_value, weight):
        """ewn_sup_grad on the rows -> [all-reduce of the flat gradient] -> ewn_a2c_apply"""
        env = self.env
        sup_grad(boards, dice, target_pi, target_value, self.params, weight=weight, pi_coef=self.pi_coef, vf_coef=self.vf_coef,
                 cube_layer=env.L, out=self.grad, scratch=self.scratch)
        self._all_reduce_grad()
        check(self.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(self.params), _ptr(self.sq_avg), _ptr(self.grad), C.byref(self.hyper),
                                     _ptr(self.grad_norm), _stream()), "ewn_a2c_apply")

    def stats_dict(self):
        g = self.grad[-8:].tolist()
        live = g[3]
        per = (lambda x: x / live) if live > 0 else (lambda x: 0.0)
        pl, vl, en = per(g[0]), per(g[4]), per(g[1])
        return {"loss": self.pi_coef * pl + self.vf_coef * vl, "policy_loss": pl, "value_loss": vl, "entropy": en, "agreement": per(g[2]),
                "grad_norm": float(self.grad_norm), "live_fraction": live / float(self._rows * self.env.N * self.world)}

    def _state(self):
        return {"sq_avg": self.sq_avg, "terminal_value": float(self.terminal_value), "sims": int(self.sims), "c_puct": float(self.c_puct),
                "fused_search": bool(self.fused), "leaves": int(self.leaves)}

    def _load_state(self, sd):
        """the keys of _state; a subclass then withdraws `fused` and `leaves` where what it was built with does not allow them"""
        self.sq_avg.copy_(sd["sq_avg"])
        self.terminal_value = float(sd.get("terminal_value", self.terminal_value))
        self.sims, self.c_puct = int(sd.get("sims", self.sims)), float(sd.get("c_puct", self.c_puct))
        self.fused = bool(sd.get("fused_search", self.fused))
        self.leaves = int(sd.get("leaves", self.leaves))


class SearchDistillTrainer(_SupervisedTrainer):
    """a2c.FusedTrainer (flat `params` viewed by `self.model`, collect_and_update, learn, policy_fn, save / load) with the supervised
    search-distillation update, which runs torch operators and allocates: it stays eager, never a captured graph.  The env's rewards
    are not read: the rollout only supplies the state distribution, so the plain or the shaped env serves, against any opponent the
    policy rollout plays (opponent=: PolicyOpponent's model opponents, "self" included)."""

    algorithm = "SEARCH"
    _written_by = "the search-distillation trainer"

    def __init__(self, env, n_steps=5, learning_rate=7e-4, pi_coef=1.0, vf_coef=0.5, temperature=0.0, plies=1, terminal_value=1.0,
                 max_grad_norm=0.5, rms_alpha=0.99, rms_eps=1e-5, seed=None, opponent=None, opponent_update_every=100,
                 opponent_deterministic=False, endgame_table=None, search="lookahead", sims=64, c_puct=1.5, endgame_leaves=False, fused=False,
                 leaves=1):
        who = "SearchDistillTrainer"
        if search not in ("lookahead", "puct"):
            raise ValueError("SearchDistillTrainer: search must be 'lookahead' or 'puct', got %r" % (search,))
        if plies not in (1, 2):
            raise ValueError("SearchDistillTrainer: plies must be 1 or 2, got %r" % (plies,))
        if search == "puct":
            _puct_numbers(who, sims, c_puct, terminal_value)
        self.temperature = _not_negative(who, "temperature", temperature)
        _finite(who, "terminal_value", terminal_value)
        if endgame_leaves and endgame_table is None:
            raise ValueError("SearchDistillTrainer: endgame_leaves=True needs an endgame_table")
        if fused and search != "puct":
            raise ValueError("SearchDistillTrainer: fused=True is the PUCT search in one launch: it needs search='puct'")
        if fused and endgame_leaves:
            raise ValueError("SearchDistillTrainer: fused=True does not take endgame_leaves=True: the exact leaves are the staged path's")
        leaves = _leaves_alone(who, leaves, **{"search=%r" % (search,): (search != "puct", "it is the PUCT search's (search='puct')"),
                                               "endgame_leaves=True": (endgame_leaves, _NO_TABLE)})
        if endgame_table is not None and not float(terminal_value) > 0.0:
            raise ValueError("SearchDistillTrainer: with an endgame table terminal_value must be positive (it scales the exact q), "
                             "got %r" % (terminal_value,))
        # endgame_table None: the search's q alone; else its q is replaced by the exact one on covered rows
        # fused: the PUCT search as the one launch of ewn_puct_search (4r): the same targets bit for bit
        super().__init__(who, env, sims=sims, c_puct=c_puct, terminal_value=terminal_value, fused=fused, pi_coef=pi_coef, vf_coef=vf_coef,
                         endgame_table=endgame_table, learning_rate=learning_rate, max_grad_norm=max_grad_norm, rms_alpha=rms_alpha,
                         rms_eps=rms_eps, leaves=leaves, n_steps=n_steps, seed=seed, use_graph=False, opponent=opponent,
                         opponent_update_every=opponent_update_every, opponent_deterministic=opponent_deterministic)
        self._size_scratch(self.n_steps)
        self.endgame_leaves = bool(endgame_leaves)   # the search itself takes the table: exact values at the leaves it covers (4p)
        self.plies, self.search = int(plies), search
        M, S = self.n_steps * env.N, env.S
        self._boards = torch.zeros((M, S, S), dtype=torch.int8, device=self.device)      # rows 0 .. n_steps - 1 of the observations, packed
        self._dice = torch.zeros(M, dtype=torch.int8, device=self.device)

    def _launch(self):
        env, K, N, S = self.env, self.n_steps, self.env.N, self.env.S
        leaves = {"endgame_table": self.endgame_table} if self.endgame_leaves else {}   # nothing: the calls as they were
        env.rollout_policy(K, self.params, traj=self.traj, noise_key=self.noise_key, **self._opponent_kwargs())
        self._boards.view(K, N, S, S).copy_(self.traj["obs_board"][:K])
        self._dice.view(K, N).copy_(self.traj["obs_dice"][:K])
        if self.search == "puct":
            _, visits, q, value = predict_puct(self._boards, self._dice, self.params, sims=self.sims, c_puct=self.c_puct,
                                               terminal_value=self.terminal_value, return_visits=True, return_q=True, return_value=True,
                                               cube_layer=env.L, fused=self.fused, leaves=self.leaves, **leaves)
            target_pi, target_value, weight = puct_targets(visits, q, value, self.terminal_value)
            if self.endgame_table is not None:     # covered rows: the exact q's targets, as the lookahead's rows get them
                _, covered, q_exact = self.endgame_table.lookup(self._boards, self._dice, return_q=True)
                e_pi, e_value, e_weight = lookahead_targets(self.terminal_value * q_exact, self.temperature)
                target_pi = torch.where(covered[:, None], e_pi, target_pi)
                target_value, weight = torch.where(covered, e_value, target_value), torch.where(covered, e_weight, weight)
        else:
            _, q = predict_lookahead(self._boards, self._dice, self.params, terminal_value=self.terminal_value, return_q=True,
                                     cube_layer=env.L, plies=self.plies, **leaves)
            if self.endgame_table is not None:     # the exact rows have -inf where the search's have: the same moves leave the board
                _, covered, q_exact = self.endgame_table.lookup(self._boards, self._dice, return_q=True)
                q = torch.where(covered[:, None, None], self.terminal_value * q_exact, q)
            target_pi, target_value, weight = lookahead_targets(q, self.temperature)
        self._update(self._boards, self._dice, target_pi, target_value, weight)

    def _state(self):
        return {**super()._state(), "plies": int(self.plies), "search": self.search}

    def _load_state(self, sd):
        super()._load_state(sd)
        self.plies = int(sd.get("plies", self.plies))
        self.search = sd.get("search", self.search)
        self.fused = self.fused and self.search == "puct" and not self.endgame_leaves
        self.leaves = self.leaves if self.search == "puct" and not self.endgame_leaves else 1


def both_flags_one_cube(boards, dice):
    """bool [M]: find_cube_to_move names one cube under both flags (plain torch): the dice's cube is on the board, or the mover's
    cubes all lie on one side of the dice.  boards int8 [M, S, S] seen from the mover, dice [M] (outside 1..6: clamped)."""
    flat = boards.reshape(boards.shape[0], -1)
    d = dice.reshape(-1).clamp(1, 6).to(torch.int64)
    present = torch.stack([(flat == k).any(1) for k in range(1, 7)], 1)
    k = torch.arange(1, 7, device=boards.device)[None, :]
    return present.gather(1, d[:, None] - 1)[:, 0] | ~(present & (k > d[:, None])).any(1) | ~(present & (k < d[:, None])).any(1)


class PuctSelfPlayTrainer(_SupervisedTrainer):
    """AlphaZero's loop on the PUCT search: the search plays itself from fresh openings on the env's lanes
    (selfplay_puct: root noise, moves drawn from the visits for the first temp_plies plies), the policy heads are trained toward the
    roots' visit distributions and the critic toward terminal_value times the result of the game seen from the side to move.  Rows
    past a game's end and rows of games that did not end within max_plies weigh nothing.  One update is one sup_grad over all
    max_plies x lanes record rows and one ewn_a2c_apply; it runs torch operators and stays eager, like the distiller.  The env's
    opponent and rewards are not used: the env supplies the lanes' opening positions."""

    algorithm = "SELFPLAY"
    _written_by = "the PUCT self-play trainer"

    def __init__(self, env, sims=64, c_puct=1.5, terminal_value=1.0, noise_eps=0.25, noise_alpha=1.0, temp_plies=8, max_plies=None,
                 learning_rate=7e-4, pi_coef=1.0, vf_coef=0.5, max_grad_norm=0.5, rms_alpha=0.99, rms_eps=1e-5, seed=None,
                 endgame_table=None, chunk=1024, fused=False, whole_games=False, leaves=1, games_table=None, leaf_table=None):
        who = "PuctSelfPlayTrainer"
        _puct_numbers(who, sims, c_puct, terminal_value)
        _noise_eps(who, noise_eps)
        _play_numbers(who, temp_plies, 0, 0)
        _positive(who, "noise_alpha", noise_alpha)
        if max_plies is not None and not (isinstance(max_plies, int) and max_plies >= 1):
            raise ValueError("%s: max_plies must be a positive integer or None, got %r" % (who, max_plies))
        _games_table_alone(who, games_table, endgame_table, leaf_table, leaves)
        if fused and endgame_table is not None:
            raise ValueError("%s: fused=True does not take an endgame_table: the exact-leaf substitution is the staged path's" % who)
        if whole_games and endgame_table is not None:
            raise ValueError("%s: whole_games=True does not take an endgame_table: the exact-leaf substitution is the staged path's" % who)
        leaves = _leaves_alone(who, leaves, endgame_table=(endgame_table is not None, _NO_TABLE),
                               **{"whole_games=True": (whole_games, _NO_WHOLE_GAMES)})
        _leaf_table_alone(who, leaf_table, endgame_table, leaves, whole_games)
        # leaf_table (a table or its path): endgame_table's exact leaves with a ply's search in the one launch of ewn_puct_search_eg (4w);
        # fused is then not read
        # endgame_table: exact values at the leaves the table covers (4p), nothing else
        # fused: a ply's search as the one launch of ewn_puct_search (4r): the same records bit for bit
        # whole_games: all games in the one launch of ewn_puct_selfplay (4s), chunk and fused are then not read: the same records again
        # games_table (a table or its path): leaf_table's records from the one launch of ewn_puct_selfplay_eg (4x); chunk, fused and
        # whole_games are then not read
        super().__init__(who, env, sims=sims, c_puct=c_puct, terminal_value=terminal_value, fused=fused, pi_coef=pi_coef, vf_coef=vf_coef,
                         endgame_table=endgame_table, learning_rate=learning_rate, max_grad_norm=max_grad_norm, rms_alpha=rms_alpha,
                         rms_eps=rms_eps, leaves=leaves, n_steps=1, seed=seed, use_graph=False, opponent=None, opponent_update_every=100,
                         opponent_deterministic=False, policy_rollout=False)
        if leaf_table is not None:
            leaf_table = _accept_table(who, leaf_table, env.S, "the leaf table is for %%dx%%d boards, the env plays %dx%d" % (env.S, env.S),
                                       name="leaf_table", load=lambda path: EndgameTable.load(path, device=env.board.device))
        self.leaf_table = leaf_table
        if games_table is not None:
            games_table = _accept_table(who, games_table, env.S, "the games table is for %%dx%%d boards, the env plays %dx%d" % (env.S, env.S),
                                        name="games_table", load=lambda path: EndgameTable.load(path, device=env.board.device))
        self.games_table = games_table
        self.max_plies = SELFPLAY_MAX_PLIES[env.S] if max_plies is None else int(max_plies)
        self._size_scratch(self.max_plies)
        self.noise_eps, self.noise_alpha, self.temp_plies = float(noise_eps), float(noise_alpha), int(temp_plies)
        self.chunk, self.whole_games = int(chunk), bool(whole_games)
        self.seed_base, self.seed_counter = (0 if seed is None else int(seed)), 0   # the counter: one per update, saved and resumed
        self.records = None                      # the last update's games (selfplay_puct's dict)
        self._games = [0.0, 0.0, 0.0, 0.0]       # live rows, mean plies, share of finished games, the first mover's share of them

    def fresh_positions(self):
        """the lanes reset on seeds no rank and no earlier update has used: counter x all lanes + the global lane id -> (board, dice,
        the first lane's global game number)"""
        env = self.env
        first = self.seed_counter * env.N * self.world + int(env.cfg.lane_offset)
        seeds = (self.seed_base + first + np.arange(env.N, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
        self.seed_counter += 1
        board, dice = env.reset(seeds=seeds.astype(np.uint32))
        return board, dice, first

    def _launch(self):
        env = self.env
        board, dice, first = self.fresh_positions()
        if self.games_table is not None:
            rec = selfplay_puct_games_exact(board, dice, self.params, self.games_table, sims=self.sims, max_plies=self.max_plies,
                                            c_puct=self.c_puct, terminal_value=self.terminal_value, noise_eps=self.noise_eps,
                                            noise_alpha=self.noise_alpha, temp_plies=self.temp_plies, key=self.noise_key, game_offset=first,
                                            cube_layer=env.L)
        elif self.whole_games:
            rec = selfplay_puct_games(board, dice, self.params, sims=self.sims, max_plies=self.max_plies, c_puct=self.c_puct,
                                      terminal_value=self.terminal_value, noise_eps=self.noise_eps, noise_alpha=self.noise_alpha,
                                      temp_plies=self.temp_plies, key=self.noise_key, game_offset=first, cube_layer=env.L)
        else:
            rec = selfplay_puct(board, dice, self.params, sims=self.sims, max_plies=self.max_plies, c_puct=self.c_puct,
                                terminal_value=self.terminal_value, noise_eps=self.noise_eps, noise_alpha=self.noise_alpha,
                                temp_plies=self.temp_plies, key=self.noise_key, game_offset=first, chunk=self.chunk,
                                endgame_table=self.endgame_table, cube_layer=env.L, fused=self.fused, leaves=self.leaves,
                                leaf_table=self.leaf_table)
        self.records = rec
        R, S = self.max_plies * env.N, env.S
        b, d = rec["board"].reshape(R, S, S), rec["dice"].reshape(R).clamp(min=1)         # rows past a game's end hold dice 0
        target_pi, _, _ = puct_targets(rec["visits"].reshape(R, 2, 3), None, rec["value"].reshape(R), self.terminal_value,
                                       one_cube=both_flags_one_cube(b, d))
        target_value = (self.terminal_value * rec["z"]).reshape(R).contiguous()
        self._update(b, d, target_pi, target_value, rec["weight"].reshape(R))

    def collect_and_update(self):
        self._launch()
        self._after_update()
        rec = self.records
        # Games differ in length from rank to rank, and learn() loops on num_timesteps: the counts are summed over the ranks, so that
        # every rank adds the same number and leaves the loop after the same update (a rank alone in the gradient's all-reduce hangs)
        counts = all_reduce_counters(torch.stack([rec["live"].sum(), rec["plies"].sum(), (rec["winner"] != 0).sum(),
                                                  (rec["winner"] == 1).sum()]).to(torch.int64)).tolist()   # the update's one host read
        games = self.env.N * self.world
        self._games = [counts[0], counts[1] / games, counts[2] / games, counts[3] / max(1, counts[2])]
        self.num_timesteps += counts[0] // self.world                                    # recorded positions, this rank's share
        return self.grad

    def stats_dict(self):
        return {**super().stats_dict(), "mean_game_length": self._games[1], "finished_fraction": self._games[2],
                "first_mover_win_fraction": self._games[3]}

    def _state(self):
        return {**super()._state(), "noise_eps": float(self.noise_eps), "noise_alpha": float(self.noise_alpha),
                "temp_plies": int(self.temp_plies), "max_plies": int(self.max_plies), "seed_counter": int(self.seed_counter),
                "whole_games": bool(self.whole_games), "leaf_table_used": self.leaf_table is not None,   # that one was used, not its bytes
                "games_table_used": self.games_table is not None}

    def _load_state(self, sd):
        super()._load_state(sd)
        self.noise_eps, self.noise_alpha = float(sd.get("noise_eps", self.noise_eps)), float(sd.get("noise_alpha", self.noise_alpha))
        self.temp_plies, self.seed_counter = int(sd.get("temp_plies", self.temp_plies)), int(sd.get("seed_counter", self.seed_counter))
        self.fused = self.fused and self.endgame_table is None
        self.whole_games = bool(sd.get("whole_games", self.whole_games)) and self.endgame_table is None and self.leaf_table is None
        self.leaves = self.leaves if self.endgame_table is None and self.leaf_table is None and not self.whole_games else 1
        if int(sd.get("max_plies", self.max_plies)) != self.max_plies:
            raise ValueError("the checkpoint's games have at most %d plies, this trainer's %d: the update's scratch is sized by it" % (
                int(sd["max_plies"]), self.max_plies))
