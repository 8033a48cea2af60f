"""VecEWN: N independent EinStein-wuerfelt-nicht games stepped on one MI355X.

Host side is plumbing only: torch owns the device buffers and the stream, every
rule, dice draw and search runs in libewn_hip.so (include/ewn_hip.h).  The class is
the batched counterpart of the reference's EinsteinWuerfeltNichtEnv /
MiniMaxHeuristicEnv (envs/ewn.py, envs/training_ewn.py): the single-game drop-in
classes in the top-level `envs` package are N=1 views of it.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import AGENT, AGENT_MCTS, HEUR, OPP, RNG, EwnAgent, EwnConfig, EwnOpponentPolicy, EwnPolicy, EwnRolloutOut, EwnState, EwnStepOut, check


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise _lib.EwnError("ewn_gym_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device(device)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _describe(t):
    if not isinstance(t, torch.Tensor):
        return type(t).__name__
    return "%s %s on %s%s" % (t.dtype, list(t.shape), t.device, "" if t.is_contiguous() else " (not contiguous)")


def _is_buffer(t, dtype):
    return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous()


def _check_buffer(who, name, t, dtype, lead, shape):
    """ValueError unless t is a contiguous device tensor of `dtype` and shape [>= lead, *shape] (lead None: exactly `shape`)"""
    if not (_is_buffer(t, dtype) and (tuple(t.shape) == shape if lead is None else
                                      t.dim() == 1 + len(shape) and t.shape[0] >= lead and tuple(t.shape[1:]) == shape)):
        dims = ([] if lead is None else [">= %d" % lead]) + [str(x) for x in shape]
        raise ValueError("%s: %s must be a contiguous %s device tensor of shape [%s], got %s" % (
            who, name, str(dtype).replace("torch.", ""), ", ".join(dims), _describe(t)))


_TOTALS = {"return_sum": torch.float64, "n_steps": torch.int32, "n_episodes": torch.int32, "n_wins": torch.int32}


def _no_initial_obs(traj):
    if "obs_board" in traj:
        raise ValueError("this trajectory was allocated with initial_obs=True (K + 1 record rows, the step views start at row 1): that "
                         "layout belongs to rollout_policy; ewn_step_k writes rows 0 .. K - 1, so rollout() would read every column one "
                         "step late.  Allocate it with alloc_rollout(K, layout='record') instead")


_TABLES = {}


def search_tables(board_size, cube_layer, device):
    """Device copy of the depth-3 search tables (built on the host by ewn_build_tables), or None."""
    key = (int(board_size), int(cube_layer), str(device))
    if key not in _TABLES:
        lib = _lib.load()
        n = int(lib.ewn_tables_bytes(key[0], key[1]))
        t = None
        if n > 0:
            host = np.zeros(n, dtype=np.uint8)
            check(lib.ewn_build_tables(key[0], key[1], host.ctypes.data_as(C.c_void_p)), "ewn_build_tables")
            t = torch.zeros(n, dtype=torch.uint8, device=device)   # torch.zeros: the guard-zone test wraps this allocator
            t.copy_(torch.from_numpy(host))
        _TABLES[key] = t
    return _TABLES[key]


class VecEWN:
    def __init__(self, n_lanes, board_size=5, cube_layer=3, opponent_policy="random", max_depth=3, heuristic="hybrid",
                 num_simulations=10, num_env_copies=5, rng="mt19937", shaped=False, reward=1.0,
                 illegal_move_reward=-1.0, illegal_move_tolerance=10, autoreset=False, shaped_refresh_on_reset=False,
                 lane_offset=0, seed_stride=None, philox_key=0, mt_window=0, want_terminal_obs=False, device="cuda",
                 use_tables=True, want_random_action=False):
        self.lib = _lib.load()
        self._opp_model = None     # set_opponent_model: (params, EwnOpponentPolicy for step(), deterministic, noise_key, action buffer)
        opp = str(opponent_policy)
        if opp not in OPP:
            raise _lib.EwnError("opponent policy %r is not supported by the HIP engine (random, minimax, mcts); a trained model as the "
                                "opponent is served by rollout_policy(..., opponent_params=) and eval_policy(..., opponent_params=) "
                                "(ewn_step_k_selfplay / ewn_policy_eval_vs), by tournament.evaluate(opponent={'kind': 'mlp', ...}) and by "
                                "the fused trainers' opponent=, not by step()" % opp)
        if heuristic not in HEUR:
            raise _lib.EwnError("heuristic %r is not supported (hybrid, min_dist, two_min_dist, attk, sim_winrate)" % heuristic)
        self.N, self.S, self.L = int(n_lanes), int(board_size), int(cube_layer)
        self.cube_num = self.L * (self.L + 1) // 2
        self.cfg = EwnConfig(self.S, self.L, self.N, OPP[opp], int(max_depth), HEUR[heuristic], int(num_simulations),
                             int(num_env_copies), RNG[rng], int(bool(shaped)), int(illegal_move_tolerance),
                             int(bool(autoreset)), int(bool(shaped_refresh_on_reset)), int(lane_offset),
                             (self.N if seed_stride is None else int(seed_stride)) & 0xFFFFFFFF, int(mt_window),
                             float(reward), float(illegal_move_reward), int(philox_key) & 0xFFFFFFFFFFFFFFFF)
        words = check(self.lib.ewn_rng_words(C.byref(self.cfg)), "ewn_rng_words")  # validates the whole config
        self.device = _require_gpu(device)
        dev, N, S = self.device, self.N, self.S
        self.board = torch.zeros((N, S, S), dtype=torch.int8, device=dev)
        self.dice = torch.zeros(N, dtype=torch.int8, device=dev)
        self.done = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.rng_state = torch.zeros((N, words), dtype=torch.int32, device=dev)
        self.prev_score = torch.zeros(N, dtype=torch.float64, device=dev) if shaped else None
        self.tolerance = torch.zeros(N, dtype=torch.int32, device=dev) if shaped else None
        self.reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self.terminated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.info = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.terminal_board = torch.zeros((N, S, S), dtype=torch.int8, device=dev) if want_terminal_obs else None
        self.terminal_dice = torch.zeros(N, dtype=torch.int8, device=dev) if want_terminal_obs else None
        # RandomAgent.predict on the post-step observation, fused into ewn_step (ewn_step_out.random_action)
        self.random_action = torch.zeros((N, 2), dtype=torch.int8, device=dev) if want_random_action else None
        nscr = check(self.lib.ewn_step_scratch_bytes(C.byref(self.cfg)), "ewn_step_scratch_bytes")
        self.scratch = torch.zeros(max(int(nscr), 8), dtype=torch.uint8, device=dev)
        self._actions = torch.zeros((N, 2), dtype=torch.int8, device=dev)
        self.tables = search_tables(self.S, self.L, dev) if use_tables else None
        self._st = EwnState(_ptr(self.board), _ptr(self.dice), _ptr(self.done), _ptr(self.rng_state),
                            _ptr(self.prev_score), _ptr(self.tolerance), _ptr(self.tables))
        self._out = EwnStepOut(_ptr(self.reward), _ptr(self.terminated), _ptr(self.truncated), _ptr(self.info),
                               _ptr(self.terminal_board), _ptr(self.terminal_dice), _ptr(self.random_action))
        check(self.lib.ewn_init_aux(C.byref(self.cfg), C.byref(self._st), _stream()), "ewn_init_aux")

    # -- reset(seed) for the lanes selected by mask (envs/ewn.py:488-494)
    def reset(self, seeds=None, mask=None):
        if seeds is not None:
            if not isinstance(seeds, torch.Tensor):  # uint32 seeds: keep the bit pattern (np.random.seed takes 0..2**32-1)
                seeds = torch.from_numpy(np.asarray(seeds, dtype=np.uint32).reshape(-1).view(np.int32).copy())
            seeds = seeds.to(self.device).to(torch.int32).contiguous()
            assert seeds.numel() == self.N
        if mask is not None:
            mask = torch.as_tensor(mask).to(self.device).to(torch.uint8).contiguous()
            assert mask.numel() == self.N
        check(self.lib.ewn_reset(C.byref(self.cfg), C.byref(self._st), _ptr(seeds), _ptr(mask), _stream()), "ewn_reset")
        return self.board, self.dice

    # -- roll_dice() (envs/ewn.py:90-92): one draw from each selected lane's dice stream
    def roll_dice(self, mask=None):
        if mask is not None:
            mask = torch.as_tensor(mask).to(self.device).to(torch.uint8).contiguous()
            assert mask.numel() == self.N
        check(self.lib.ewn_roll_dice(C.byref(self.cfg), C.byref(self._st), _ptr(mask), _stream()), "ewn_roll_dice")
        return self.dice

    # -- step(actions) (envs/ewn.py:436-486 / envs/training_ewn.py:43-99)
    def step(self, actions):
        if not _is_buffer(actions, torch.int8):
            actions = self._actions.copy_(torch.as_tensor(actions).reshape(self.N, 2))
        assert actions.numel() == 2 * self.N
        if self._opp_model is not None:
            check(self.lib.ewn_step_vs(C.byref(self.cfg), C.byref(self._st), _ptr(actions), C.byref(self._opp_model[1]),
                                       C.byref(self._out), _stream()), "ewn_step_vs")
            return self.board, self.dice, self.reward, self.terminated, self.truncated, self.info
        check(self.lib.ewn_step(C.byref(self.cfg), C.byref(self._st), _ptr(actions), C.byref(self._out), _ptr(self.scratch),
                                _stream()), "ewn_step")
        return self.board, self.dice, self.reward, self.terminated, self.truncated, self.info

    # -- a trained policy as this env's opponent (the reference's `opponent_policy=<path>`, envs/ewn.py:265-296)
    def supports_step_vs(self):
        """step() / rollout() against a model are served (ewn_step_vs / ewn_step_k_vs): cube_layer 3 on 5x5 and 7x7, Philox dice or
        MT19937-compat dice without auto-reset.  The env's own opponent settings do not matter to it."""
        return self.tables is not None and self.lib.ewn_step_vs_supported(C.byref(self.cfg)) == 1

    def set_opponent_model(self, params, deterministic=True, noise_key=0, opponent_action=None):
        """Make the actor-critic whose flat fp32 device vector is `params` (a2c.ActorCritic.flat_parameters() order) this env's
        opponent: it sees np.rot90(-board, 2) with its own dice and plays its argmax (deterministic=False: a Gumbel-max sample under
        noise_key); a move that leaves the board or asks for a missing cube ends the episode with reward 0 ("Invalid move for
        opponent!").  While a model is set step() runs ewn_step_vs, rollout() ewn_step_k_vs, rollout_policy() / eval_policy() take it as
        their default opponent_params, and agent_rollout() raises.  opponent_action: optional int8 [N, 3] that step() fills with the
        opponent's {dice, flag, dir} ({0, 0, 0}: it did not move).  params=None gives the env its own opponent back.  The vector is
        read at every call, not copied: keep it alive and unchanged while it plays."""
        if params is None:
            if opponent_action is not None:
                raise ValueError("set_opponent_model: opponent_action needs params")
            self._opp_model = None
            return
        act3 = None
        if opponent_action is not None:
            _check_buffer("set_opponent_model", "opponent_action", opponent_action, torch.int8, None, (self.N, 3))
            act3 = opponent_action.unsqueeze(0)
        st = self._opponent_struct("set_opponent_model", 1, params, deterministic, noise_key, act3)
        if not self.supports_step_vs():
            raise _lib.EwnError("set_opponent_model: ewn_step_vs does not serve this env (cube_layer 3 on 5x5 / 7x7 with the search "
                                "tables; MT19937-compat dice only without auto-reset)")
        if self.random_action is not None:
            raise _lib.EwnError("set_opponent_model: want_random_action=True is ewn_step's fused RandomAgent; against a model use "
                                "rollout(K, agent='random') or sample_legal_actions()")
        self._opp_model = (params, st, bool(deterministic), int(noise_key), opponent_action)

    def _model_opponent(self, what, K, action):
        """the set model as the ewn_opponent_policy of a K-step call"""
        params, _, det, nk, _ = self._opp_model
        return self._opponent_struct(what, K, params, det, nk, action)

    # -- RandomAgent as a stateless device policy (classical_policies/random_policy.py:11-15)
    def sample_legal_actions(self, step, out=None, step_tensor=None):
        """step_tensor: optional int32 device scalar added to `step` on the device (lets a captured graph advance)"""
        out = self._actions if out is None else out
        check(self.lib.ewn_predict_random(self.S, self.L, self.N, _ptr(self.board), _ptr(self.dice),
                                          C.c_uint64(self.cfg.philox_key), C.c_uint32(int(step) & 0xFFFFFFFF),
                                          _ptr(step_tensor), int(self.cfg.lane_offset), _ptr(out), _stream()),
              "ewn_predict_random")
        return out

    def rng_overflow(self):
        """uint8 [N]: lanes whose current episode has consumed more MT19937 draws than the closed form covers (454; see
        DESIGN.md section 3) -- from then on their dice are NOT numpy's.  Always zero for the Philox kind."""
        if self.cfg.rng_kind != RNG["mt19937"]:
            return torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        return (self.rng_state.view(-1)[3:4 * self.N:4] & 1).to(torch.uint8)

    def check_rng(self):
        """Raise if any lane ran past the MT19937-compat stream (one device reduction + sync: call it where a host sync
        happens anyway -- the N=1 drop-in env does so every step, tournament.evaluate once per evaluation)."""
        if self.cfg.rng_kind == RNG["mt19937"] and bool(self.rng_overflow().any()):
            lanes = torch.nonzero(self.rng_overflow()).reshape(-1)[:8].tolist()
            raise _lib.EwnError("MT19937-compat dice stream exhausted (>= 454 draws in one episode) on lanes %s: results are no "
                                "longer bit-identical to numpy's stream; use rng='philox' for such long games" % lanes)

    # -- K env steps per launch with an in-engine agent (ewn_step_k; eval_minimax.py:16-50's loop on the device)
    def supports_rollout(self, agent="random", agent_max_depth=3):
        """True when ewn_step_k (with a model set: ewn_step_k_vs) exists for this configuration and agent"""
        if agent not in AGENT:
            return False
        if self._opp_model is not None:
            return self.tables is not None and self.lib.ewn_step_k_vs_supported(C.byref(self.cfg), AGENT[agent], int(agent_max_depth)) == 1
        if self.tables is None and int(self.lib.ewn_tables_bytes(self.S, self.L)) > 0:
            return False           # use_tables=False on a table geometry (geometries WITHOUT a table image run the generic K-step kernel)
        return self.lib.ewn_step_k_supported(C.byref(self.cfg), AGENT[agent], int(agent_max_depth)) == 1

    def alloc_rollout(self, K, board=True, layout="columns", initial_obs=False):
        """Trajectory buffers for rollout(K, traj=...): dict of [K, N, ...] tensors (the observation column is optional).
        layout="record": ONE 16-byte aligned record per lane-step (ewn_rollout_out.record: board | dice | action | terminated |
        truncated | info | padding; 32 bytes for 5x5) plus the f64 reward column; the dict's board / dice / action / flag entries
        are then strided VIEWS into the records."""
        dev, N, S = self.device, self.N, self.S
        if layout == "record":
            C2 = S * S
            stride = (C2 + 6 + 15) & ~15
            # initial_obs (rollout_policy(record_initial_obs=True)): one more row in front, the observation before step 0; the
            # per-step views below then start at row 1 and "obs_board" / "obs_dice" are the K + 1 observations s_0 .. s_K
            full = torch.zeros((K + (1 if initial_obs else 0), N, stride), dtype=torch.uint8, device=dev)
            rec = full[1:] if initial_obs else full
            t = {"record": full, "reward": torch.zeros((K, N), dtype=torch.float64, device=dev),
                 "board": rec[:, :, :C2].view(torch.int8).unflatten(2, (S, S)), "dice": rec[:, :, C2].view(torch.int8),
                 "action": rec[:, :, C2 + 1:C2 + 3].view(torch.int8), "terminated": rec[:, :, C2 + 3],
                 "truncated": rec[:, :, C2 + 4], "info": rec[:, :, C2 + 5]}
            if initial_obs:
                t["obs_board"] = full[:, :, :C2].view(torch.int8).unflatten(2, (S, S))
                t["obs_dice"] = full[:, :, C2].view(torch.int8)
            return t
        assert layout == "columns"
        t = {"dice": torch.zeros((K, N), dtype=torch.int8, device=dev),
             "action": torch.zeros((K, N, 2), dtype=torch.int8, device=dev),
             "reward": torch.zeros((K, N), dtype=torch.float64, device=dev),
             "terminated": torch.zeros((K, N), dtype=torch.uint8, device=dev),
             "truncated": torch.zeros((K, N), dtype=torch.uint8, device=dev),
             "info": torch.zeros((K, N), dtype=torch.uint8, device=dev)}
        if board:
            t["board"] = torch.zeros((K, N, S, S), dtype=torch.int8, device=dev)
        return t

    def alloc_totals(self):
        """Per-lane accumulators for rollout(..., totals=...): return_sum, n_steps, n_episodes, n_wins (rollout ADDS to them)"""
        dev, N = self.device, self.N
        return {"return_sum": torch.zeros(N, dtype=torch.float64, device=dev), "n_steps": torch.zeros(N, dtype=torch.int32, device=dev),
                "n_episodes": torch.zeros(N, dtype=torch.int32, device=dev), "n_wins": torch.zeros(N, dtype=torch.int32, device=dev)}

    def _check_traj(self, who, K, traj):
        """traj as alloc_rollout() makes it (either layout, without the initial-observation row), at least K steps long"""
        if not isinstance(traj, dict):
            raise ValueError("%s: traj must be the dict of alloc_rollout(), got %s" % (who, type(traj).__name__))
        _no_initial_obs(traj)
        N, S = self.N, self.S
        cols = {"board": (torch.int8, (N, S, S)), "dice": (torch.int8, (N,)), "action": (torch.int8, (N, 2)),
                "reward": (torch.float64, (N,)), "terminated": (torch.uint8, (N,)), "truncated": (torch.uint8, (N,)),
                "info": (torch.uint8, (N,)), "record": (torch.uint8, (N, (S * S + 6 + 15) & ~15))}
        for name, t in traj.items():
            if name not in cols:
                raise ValueError("%s: unknown trajectory entry %r" % (who, name))
            if "record" not in traj or name in ("record", "reward"):   # the record layout's column entries are views, not buffers
                _check_buffer(who, "traj[%r]" % name, t, cols[name][0], K, cols[name][1])

    def _check_totals(self, who, totals, required=False):
        """totals as alloc_totals() makes it; required: all four entries, else any subset"""
        if not isinstance(totals, dict):
            raise ValueError("%s: totals must be the dict of alloc_totals(), got %s" % (who, type(totals).__name__))
        for name in (_TOTALS if required else totals):
            if name not in _TOTALS:
                raise ValueError("%s: unknown totals entry %r" % (who, name))
            _check_buffer(who, "totals[%r]" % name, totals.get(name), _TOTALS[name], None, (self.N,))

    @staticmethod
    def _rollout_out(traj, totals):
        col = (lambda k: None) if "record" in traj else traj.get   # record layout: the column entries are views, not buffers
        return EwnRolloutOut(_ptr(col("board")), _ptr(col("dice")), _ptr(col("action")), _ptr(traj.get("reward")),
                             _ptr(col("terminated")), _ptr(col("truncated")), _ptr(col("info")),
                             _ptr(totals.get("return_sum")), _ptr(totals.get("n_steps")), _ptr(totals.get("n_episodes")),
                             _ptr(totals.get("n_wins")), _ptr(traj.get("record")))

    def rollout(self, K, agent="random", agent_max_depth=3, traj=None, totals=None, opponent_action=None):
        """Play K steps of every lane in one launch, the agent being RandomAgent ("random"), ExpectiMinimaxAgent(agent_max_depth)
        ("minimax") or env.action_space.sample() ("sample": all six actions, illegal ones included).
        traj: dict from alloc_rollout (first dimension >= K) or None; totals: dict from alloc_totals or None.
        With a model set (set_opponent_model) the opponent is the model (ewn_step_k_vs); opponent_action: optional int8 [>= K, N, 3],
        its {dice, flag, dir} per step."""
        traj, totals = traj or {}, totals or {}
        if opponent_action is not None and self._opp_model is None:
            raise ValueError("rollout: opponent_action needs a model opponent (set_opponent_model)")
        self._check_traj("rollout", K, traj)
        self._check_totals("rollout", totals)
        out = self._rollout_out(traj, totals)
        if self._opp_model is not None:
            opp = self._model_opponent("rollout", K, opponent_action)
            check(self.lib.ewn_step_k_vs(C.byref(self.cfg), C.byref(self._st), int(K), AGENT[agent], int(agent_max_depth), C.byref(opp),
                                         C.byref(out), _stream()), "ewn_step_k_vs")
            return self.board, self.dice
        check(self.lib.ewn_step_k(C.byref(self.cfg), C.byref(self._st), int(K), AGENT[agent], int(agent_max_depth), C.byref(out),
                                  _stream()), "ewn_step_k")
        return self.board, self.dice

    def bind_rollout(self, K, agent="random", agent_max_depth=3, traj=None, totals=None):
        """rollout(K, ...) with its arguments marshalled ONCE: returns a zero-argument callable that enqueues the launch (for loops that
        repeat the same call: one C-ABI call per invocation, a few microseconds of host time instead of the ~20 of building the structs).
        The buffers of traj / totals must stay alive as long as the callable is used."""
        if self._opp_model is not None:
            raise _lib.EwnError("bind_rollout: a model opponent is set; use rollout() (ewn_step_k_vs)")
        traj, totals = traj or {}, totals or {}
        self._check_traj("bind_rollout", K, traj)
        self._check_totals("bind_rollout", totals)
        out = self._rollout_out(traj, totals)
        fn, cfg, st, outp = self.lib.ewn_step_k, C.byref(self.cfg), C.byref(self._st), C.byref(out)
        k, a, d = int(K), AGENT[agent], int(agent_max_depth)
        keep = (out, traj, totals)

        def call():
            rc = fn(cfg, st, k, a, d, outp, _stream())
            if rc != 0:
                check(rc, "ewn_step_k")
            return keep and None
        return call

    # -- K env steps per launch with the trained policy as the agent (ewn_step_k_policy; train.py:134, 148's rollout collection)
    def policy_param_count(self):
        return int(check(self.lib.ewn_policy_param_count(self.S, self.L), "ewn_policy_param_count"))

    def supports_policy_rollout(self):
        return self.tables is not None and self.lib.ewn_step_k_supported(C.byref(self.cfg), AGENT["mlp"], 0) == 1

    def supports_selfplay_rollout(self, value=False):
        """rollout_policy(..., opponent_params=) is served (ewn_step_k_selfplay; value: with the value output).  The env's own opponent
        settings do not matter to it."""
        pol = EwnPolicy(None, 0, 0, 0, None, 1 if value else None, None)
        return self.tables is not None and self.lib.ewn_step_k_selfplay_supported(C.byref(self.cfg), C.byref(pol)) == 1

    def supports_policy_eval_vs(self):
        """eval_policy(..., opponent_params=) is served (ewn_policy_eval_vs)"""
        return self.tables is not None and self.lib.ewn_policy_eval_vs_supported(C.byref(self.cfg)) == 1

    def _opponent_struct(self, what, K, opponent_params, deterministic, noise_key, action):
        _check_buffer(what, "opponent_params", opponent_params, torch.float32, None, (self.policy_param_count(),))
        if action is not None:
            _check_buffer(what, "opponent_action", action, torch.int8, K, (self.N, 3))
        return EwnOpponentPolicy(_ptr(opponent_params), int(bool(deterministic)), int(noise_key) & 0xFFFFFFFFFFFFFFFF, _ptr(action))

    def _resolve_opponent(self, what, K, opponent_params, deterministic, noise_key, action):
        """the opponent of a policy-driven K-step call: the set model, as set_opponent_model configured it; else opponent_params; else
        None (the env's own opponent)"""
        if opponent_params is not None:
            return self._opponent_struct(what, K, opponent_params, deterministic, noise_key, action)
        if self._opp_model is not None:
            return self._model_opponent(what, K, action)
        if action is not None:
            raise ValueError("%s: opponent_action needs opponent_params" % what)
        return None

    def rollout_policy(self, K, params, traj=None, totals=None, deterministic=False, noise_key=0, logits=None, value=None, noise=None,
                       opponent_params=None, opponent_deterministic=False, opponent_noise_key=0, opponent_action=None):
        """Play K steps of every lane in one launch, actions sampled from the actor-critic whose flat fp32 parameter vector is
        `params` (a2c.ActorCritic.flat order).  traj: dict from alloc_rollout (a record layout allocated with initial_obs=True gets
        K + 1 rows); logits [K, N, 5] / value [K, N] / noise [K, N, 5] float32: optional per-step outputs of the policy.  Buffers of the
        wrong shape, dtype or layout raise ValueError before anything is launched.
        opponent_params: a second parameter vector (may be `params` itself) that plays the opponent instead of the env's own
        (ewn_step_k_selfplay): sampled unless opponent_deterministic, noise under opponent_noise_key; opponent_action: optional int8
        [>= K, N, 3], the opponent's {dice, flag, dir} per step ({0, 0, 0}: it did not move)."""
        traj, totals = traj or {}, totals or {}
        assert params.dtype == torch.float32 and params.is_contiguous() and params.numel() == self.policy_param_count()
        N = self.N
        opp = self._resolve_opponent("rollout_policy", K, opponent_params, opponent_deterministic, opponent_noise_key, opponent_action)
        for name, t, shape in (("logits", logits, (N, 5)), ("value", value, (N,)), ("noise", noise, (N, 5))):
            if t is not None:
                _check_buffer("rollout_policy", name, t, torch.float32, K, shape)
        rec0 = 0
        if "record" in traj:
            rec0 = 1 if "obs_board" in traj else 0
            assert traj["record"].shape[0] >= K + rec0
        for name, t in traj.items():
            if name == "record" or name.startswith("obs_"):
                continue
            if t.shape[0] < K or t.shape[1] != N or ("record" not in traj and not t.is_contiguous()):
                raise ValueError("rollout_policy: traj[%r] must have shape [>= %d, %d, ...]%s, got %s" % (
                    name, K, N, "" if "record" in traj else " and be contiguous", _describe(t)))
        out = self._rollout_out(traj, totals)
        pol = EwnPolicy(_ptr(params), int(bool(deterministic)), rec0, int(noise_key) & 0xFFFFFFFFFFFFFFFF, _ptr(logits), _ptr(value), _ptr(noise))
        if opp is not None:
            check(self.lib.ewn_step_k_selfplay(C.byref(self.cfg), C.byref(self._st), int(K), C.byref(pol), C.byref(opp), C.byref(out),
                                               _stream()), "ewn_step_k_selfplay")
            return self.board, self.dice
        check(self.lib.ewn_step_k_policy(C.byref(self.cfg), C.byref(self._st), int(K), C.byref(pol), C.byref(out), _stream()),
              "ewn_step_k_policy")
        return self.board, self.dice

    # -- K env steps per launch with the trained policy's argmax as the agent, one episode per lane (ewn_policy_eval; train.py:66-117)
    def supports_policy_eval(self):
        return self.tables is not None and self.lib.ewn_policy_eval_supported(C.byref(self.cfg)) == 1

    def supports_policy_eval_mcts(self):
        """the same against this env's flat Monte-Carlo opponent (ewn_policy_eval_mcts; no table image needed)"""
        return self.lib.ewn_policy_eval_mcts_supported(C.byref(self.cfg)) == 1

    def eval_policy(self, K, params, totals, action=None, opponent_params=None, opponent_action=None, opponent_deterministic=True,
                    opponent_noise_key=0):
        """Play K steps of every lane in one launch, the agent playing the argmax of the actor-critic whose flat fp32 parameter vector
        is `params` (a2c.ActorCritic.parameters() order), on the un-shaped env without auto-reset.  totals: dict from alloc_totals
        (required, ADDED to); action: optional int8 [>= K, N, 2] (row k of a lane is written only if the lane played step k).
        Buffers of the wrong shape, dtype or layout raise ValueError before anything is launched.  An env whose opponent is MCTS is
        served by ewn_policy_eval_mcts, every other by ewn_policy_eval: the same arguments, the same contract.
        opponent_params: a second parameter vector that plays the opponent instead of the env's own (ewn_policy_eval_vs; its argmax
        unless opponent_deterministic=False); opponent_action: optional int8 [>= K, N, 3], the opponent's {dice, flag, dir} of the steps a
        lane plays ({0, 0, 0}: it did not move)."""
        opp = self._resolve_opponent("eval_policy", K, opponent_params, opponent_deterministic, opponent_noise_key, opponent_action)
        _check_buffer("eval_policy", "params", params, torch.float32, None, (self.policy_param_count(),))
        self._check_totals("eval_policy", totals, required=True)
        if action is not None:
            _check_buffer("eval_policy", "action", action, torch.int8, K, (self.N, 2))
        out = self._rollout_out({"action": action}, totals)
        if opp is not None:
            check(self.lib.ewn_policy_eval_vs(C.byref(self.cfg), C.byref(self._st), int(K), _ptr(params), C.byref(opp), C.byref(out),
                                              _stream()), "ewn_policy_eval_vs")
        elif self.cfg.opponent_kind == OPP["mcts"]:
            check(self.lib.ewn_policy_eval_mcts(C.byref(self.cfg), C.byref(self._st), int(K), _ptr(params), C.byref(out), _stream()),
                  "ewn_policy_eval_mcts")
        else:
            check(self.lib.ewn_policy_eval(C.byref(self.cfg), C.byref(self._st), int(K), _ptr(params), C.byref(out), _stream()),
                  "ewn_policy_eval")
        return self.board, self.dice

    # -- K env steps per launch with an MCTS agent, or a minimax agent against the MCTS opponent (ewn_step_k_agent; eval_pairs.py:10-35)
    def _agent_struct(self, agent, step_base=0, key=0):
        """tournament-style agent spec {"kind": "mcts"|"minimax", ...} -> EwnAgent, or None for kinds this path never takes"""
        kind = agent.get("kind") if isinstance(agent, dict) else None
        if kind == "mcts":
            return EwnAgent(AGENT_MCTS, 0, 0, int(agent.get("num_simulations", 10)), int(agent.get("num_env_copies", 5)),
                            int(step_base) & 0xFFFFFFFF, int(key) & 0xFFFFFFFFFFFFFFFF)
        if kind == "minimax":
            heur = agent.get("heuristic", "hybrid")
            if heur not in HEUR:
                return None
            return EwnAgent(AGENT["minimax"], int(agent.get("max_depth", 3)), HEUR[heur], 0, 0, 0, 0)
        return None

    def supports_agent_rollout(self, agent):
        """True when ewn_step_k_agent serves this configuration and agent (an MCTS agent against RandomAgent, minimax or MCTS; a
        minimax agent against MCTS); decided on the host"""
        a = self._agent_struct(agent)
        if a is None or self._opp_model is not None:
            return False
        if self.tables is None and (a.kind == AGENT["minimax"] or self.cfg.opponent_kind == OPP["minimax"]):
            return False           # use_tables=False: the minimax side searches from its table image
        return self.lib.ewn_step_k_agent_supported(C.byref(self.cfg), C.byref(a)) == 1

    def agent_rollout(self, K, agent, step_base=0, key=0, traj=None, totals=None):
        """Play K steps of every lane in one launch, the agent being the tournament spec `agent` (MctsAgent or ExpectiMinimaxAgent).
        The MCTS agent's playouts at step k of this call are those of predict_mcts(board, dice, key=key_t, obs_id=lane_offset + lane),
        key_t = key + 0x9E3779B97F4A7C15 * (step_base + k + 1) mod 2^64: tournament.evaluate's per-step loop at t = step_base + k.
        traj: dict from alloc_rollout (columns or record layout, first dimension >= K) or None; totals: dict from alloc_totals or None
        (ADDED to).  Buffers of the wrong shape, dtype or layout raise ValueError before anything is launched."""
        if self._opp_model is not None:
            raise _lib.EwnError("agent_rollout: a model opponent is set and ewn_step_k_agent has none; step the MCTS agent ply by ply "
                                "(predict_mcts + step), or use rollout() for the random / minimax agents")
        a = self._agent_struct(agent, step_base, key)
        if a is None:
            raise ValueError("agent_rollout: agent must be {\"kind\": \"mcts\"|\"minimax\", ...} with a known heuristic, got %r" % (agent,))
        traj, totals = traj or {}, totals or {}
        self._check_traj("agent_rollout", K, traj)
        self._check_totals("agent_rollout", totals)
        out = self._rollout_out(traj, totals)
        check(self.lib.ewn_step_k_agent(C.byref(self.cfg), C.byref(self._st), int(K), C.byref(a), C.byref(out), _stream()),
              "ewn_step_k_agent")
        return self.board, self.dice

    def set_obs(self, boards, dice):
        """Overwrite the observation of every lane (agent = TOP_LEFT to move); RNG state is kept."""
        self.board.copy_(torch.as_tensor(boards).reshape(self.N, self.S, self.S))
        self.dice.copy_(torch.as_tensor(dice).reshape(self.N))
        self.done.zero_()

    def state_dict(self):
        """Checkpoint of the env (the reference never checkpoints env state)."""
        keys = ("board", "dice", "done", "rng_state", "scratch", "prev_score", "tolerance")  # scratch: the MT refill queue
        return {k: getattr(self, k).clone() for k in keys if getattr(self, k) is not None}

    def load_state_dict(self, sd):
        for k, v in sd.items():
            getattr(self, k).copy_(v)


# ---------------------------------------------------------------- stateless batched queries

def _prep(boards, dice=None, device="cuda"):
    dev = _require_gpu(device)
    b = torch.as_tensor(boards)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    M, S = b.shape[0], b.shape[1]
    b = b.to(dev).to(torch.int8).contiguous()
    d = None
    if dice is not None:
        d = torch.as_tensor(dice).reshape(-1).to(dev).to(torch.int8).contiguous()
        assert d.numel() == M
    return b, d, M, S, dev


def legal_actions(boards, dice, player=1, cube_layer=3):
    """get_legal_actions / find_cube_to_move / check_win on M boards -> (acts[M,6,2], n[M], cube_small[M], cube_large[M], win[M])"""
    lib = _lib.load()
    b, d, M, S, dev = _prep(boards, dice)
    acts = torch.full((M, 6, 2), -1, dtype=torch.int8, device=dev)
    n = torch.zeros(M, dtype=torch.int8, device=dev)
    cs = torch.zeros(M, dtype=torch.int8, device=dev)
    cl = torch.zeros(M, dtype=torch.int8, device=dev)
    win = torch.zeros(M, dtype=torch.uint8, device=dev)
    check(lib.ewn_legal_actions(S, cube_layer, M, _ptr(b), _ptr(d), int(player), _ptr(acts), _ptr(n), _ptr(cs), _ptr(cl),
                                _ptr(win), _stream()), "ewn_legal_actions")
    return acts, n, cs, cl, win


def apply_action(boards, dice, actions, player=1, cube_layer=3):
    """make_simulated_action on M positions -> (new boards int8 [M,S,S], valid uint8 [M])"""
    lib = _lib.load()
    b, d, M, S, dev = _prep(boards, dice)
    a = torch.as_tensor(actions).reshape(M, 2).to(dev).to(torch.int8).contiguous()
    nb = torch.zeros_like(b)
    valid = torch.zeros(M, dtype=torch.uint8, device=dev)
    check(lib.ewn_apply_action(S, cube_layer, M, _ptr(b), _ptr(d), int(player), _ptr(a), _ptr(nb), _ptr(valid), _stream()),
          "ewn_apply_action")
    return nb, valid


def playout_wins(boards, first_player, n_sims=100, key=0, cube_layer=3):
    """MinimaxEnv.simulate on M positions -> int32 [M] playouts won by TOP_LEFT out of n_sims"""
    lib = _lib.load()
    b, _, M, S, dev = _prep(boards)
    wins = torch.zeros(M, dtype=torch.int32, device=dev)
    check(lib.ewn_playout_wins(S, cube_layer, M, _ptr(b), int(first_player), int(n_sims), C.c_uint64(key), _ptr(wins), _stream()),
          "ewn_playout_wins")
    return wins


def evaluate(boards, heuristic="hybrid", cube_layer=3):
    lib = _lib.load()
    if heuristic not in HEUR:
        raise _lib.EwnError("heuristic %r is not supported" % heuristic)
    b, _, M, S, dev = _prep(boards)
    out = torch.zeros(M, dtype=torch.float64, device=dev)
    check(lib.ewn_evaluate(S, cube_layer, M, _ptr(b), HEUR[heuristic], _ptr(out), _stream()), "ewn_evaluate")
    return out


def predict_minimax(boards, dice, max_depth, heuristic="hybrid", cube_layer=3, use_tables=True, key=0, obs_id=None):
    """ExpectiMinimaxAgent.predict on M observations -> (actions int8 [M,2], root values f64 [M]).  key / obs_id select the
    playouts' randomness of the 'sim_winrate' heuristic (ignored otherwise)."""
    lib = _lib.load()
    if heuristic not in HEUR:
        raise _lib.EwnError("heuristic %r is not supported" % heuristic)
    b, d, M, S, dev = _prep(boards, dice)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    vals = torch.zeros(M, dtype=torch.float64, device=dev)
    if heuristic == "sim_winrate":
        ids = None
        if obs_id is not None:
            ids = torch.from_numpy(np.asarray(obs_id, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(dev)
        check(lib.ewn_predict_minimax_sim(S, cube_layer, M, _ptr(b), _ptr(d), int(max_depth), C.c_uint64(key), _ptr(ids), _ptr(acts),
                                          _ptr(vals), _stream()), "ewn_predict_minimax_sim")
        return acts, vals
    tables = search_tables(S, cube_layer, dev) if use_tables else None
    check(lib.ewn_predict_minimax(S, cube_layer, M, _ptr(b), _ptr(d), int(max_depth), HEUR[heuristic], _ptr(acts),
                                  _ptr(vals), _ptr(tables), _stream()), "ewn_predict_minimax")
    return acts, vals


def predict_random(boards, dice, key=0, step=0, lane_offset=0, cube_layer=3):
    lib = _lib.load()
    b, d, M, S, dev = _prep(boards, dice)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    check(lib.ewn_predict_random(S, cube_layer, M, _ptr(b), _ptr(d), C.c_uint64(key), C.c_uint32(step), None,
                                 int(lane_offset), _ptr(acts), _stream()), "ewn_predict_random")
    return acts


def predict_mcts(boards, dice, num_simulations=10, num_env_copies=5, key=0, obs_id=None, cube_layer=3):
    lib = _lib.load()
    b, d, M, S, dev = _prep(boards, dice)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    wins = torch.zeros((M, 6), dtype=torch.int32, device=dev)
    ids = None
    if obs_id is not None:
        ids = torch.from_numpy(np.asarray(obs_id, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(dev)
    check(lib.ewn_predict_mcts(S, cube_layer, M, _ptr(b), _ptr(d), int(num_simulations), int(num_env_copies),
                               C.c_uint64(key), _ptr(ids), _ptr(acts), _ptr(wins), _stream()), "ewn_predict_mcts")
    return acts, wins


def _policy_input(name, x, dtype, shape, dev, who="predict_policy"):
    """a tensor is taken as it is and must already be what the kernel reads; anything else (numpy, lists) is copied to the device"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x)).to(dtype).reshape(shape)
        return x if dev.type != "cuda" else x.to(dev)
    if x.dtype != dtype or x.numel() != math.prod(shape) or not x.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of %s elements, got %s" % (
            who, name, str(dtype).replace("torch.", ""), " x ".join(map(str, shape)), _describe(x)))
    return x.reshape(shape)


def predict_policy(boards, dice, params, deterministic=True, key=0, obs_id=None, uniforms=None, return_logits=False, return_value=False,
                   cube_layer=3):
    """The trained actor-critic's predict on M observations (ewn_predict_policy; model.predict(obs, deterministic=True) upstream):
    boards [S, S] or [M, S, S], dice [M], params the flat fp32 device vector of a2c.ActorCritic.flat_parameters() -> actions int8
    [M, 2], or the tuple (actions, logits float32 [M, 5] if return_logits, value float32 [M] if return_value).  The network is the
    rollout kernel's: a rollout_policy step replayed on its observation with its recorded noise row as `uniforms` returns the recorded
    logits, value and action bit for bit.  deterministic=False samples (Gumbel-max): from `uniforms` (float32 [M, 5] in (0, 1)) when
    given, else from a hash of (key, obs_id[m]) -- obs_id None: m.  Tensors are read in place and must be contiguous device tensors of
    the kernel's dtype (int8 observations, float32 params / uniforms, int32 or uint32 obs_id); host arrays are copied over.  Anything
    else raises ValueError before a launch."""
    who = "predict_policy"
    lib = _lib.load()
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    dev = _policy_params(who, params, P, S)
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev)
    d = _policy_input("dice", dice, torch.int8, (M,), dev)
    u = None if uniforms is None else _policy_input("uniforms", uniforms, torch.float32, (M, 5), dev)
    ids = None
    if obs_id is not None:
        if isinstance(obs_id, torch.Tensor) and obs_id.dtype == torch.uint32:
            obs_id = obs_id.view(torch.int32)
        if not isinstance(obs_id, torch.Tensor):
            obs_id = np.asarray(obs_id).astype(np.uint32).view(np.int32)
        ids = _policy_input("obs_id", obs_id, torch.int32, (M,), dev)
    _same_gpu(who, dev, "params", (("params", params), ("boards", b), ("dice", d), ("uniforms", u), ("obs_id", ids)))
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    logits = torch.zeros((M, 5), dtype=torch.float32, device=dev) if return_logits else None
    value = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    with torch.cuda.device(dev):
        check(lib.ewn_predict_policy(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(params), int(bool(deterministic)),
                                     C.c_uint64(int(key) & 0xFFFFFFFFFFFFFFFF), _ptr(ids), _ptr(u), _ptr(acts), _ptr(logits), _ptr(value),
                                     _stream()), "ewn_predict_policy")
    out = (acts,) + ((logits,) if return_logits else ()) + ((value,) if return_value else ())
    return out[0] if len(out) == 1 else out


def _lookahead_shape(who, boards, cube_layer=None):
    """(M, S, P) of boards [S, S] or [M, S, S], P the policy network's parameter count; ValueError where there is no policy network for
    the geometry.  cube_layer None: any board size, P None"""
    shp = tuple(boards.shape) if isinstance(boards, torch.Tensor) else np.asarray(boards).shape
    if len(shp) == 2:
        shp = (1,) + tuple(shp)
    if len(shp) != 3 or shp[1] != shp[2]:
        raise ValueError("%s: boards must have shape [S, S] or [M, S, S], got %s" % (who, list(shp)))
    M, S = int(shp[0]), int(shp[1])
    P = None if cube_layer is None else _lib.load().ewn_policy_param_count(S, int(cube_layer))
    if P is not None and P < 0:
        raise ValueError("%s: no policy network for %dx%d boards with cube_layer %d (served: cube_layer 3 on 5x5 and 7x7)" % (
            who, S, S, cube_layer))
    return M, S, P


def _policy_params(who, params, P, S):
    """params is the flat fp32 vector of the SxS actor-critic, P elements -> its device, where everything else has to live"""
    if not (isinstance(params, torch.Tensor) and params.dtype == torch.float32 and params.is_contiguous() and params.numel() == P):
        raise ValueError("%s: params must be a contiguous float32 tensor of %d elements (the %dx%d actor-critic), got %s" % (
            who, P, S, S, _describe(params)))
    return params.device


def _same_gpu(who, dev, holder, named):
    """every tensor of named = [(name, tensor or None)] lives on dev, a GPU: the one that holds `holder`"""
    for name, t in named:
        if t is not None and not (t.is_cuda and t.device == dev):
            raise ValueError("%s: %s must live on the GPU that holds %s (%s), got %s" % (who, name, holder, dev, _describe(t)))


def _stage_inputs(who, named, cube_layer):
    """the inputs of a lookahead stage, checked as predict_lookahead checks its own: named = [(name, x, dtype, shape of (M, S))], boards
    first.  The device is the first tensor's (host arrays are copied there), and it must be a GPU."""
    M, S, _ = _lookahead_shape(who, named[0][1], cube_layer)
    if M * LA_ROWS > 2 ** 31 - 1:
        raise ValueError("%s: %d observations are %d leaf rows, more than 2^31 - 1: call in chunks" % (who, M, M * LA_ROWS))
    first = next((x for _, x, _, _ in named if isinstance(x, torch.Tensor)), None)
    dev = first.device if first is not None else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")
    out = [_policy_input(name, x, dtype, shape(M, S), dev, who=who) for name, x, dtype, shape in named]
    _same_gpu(who, dev, named[0][0], [(name, t) for (name, _, _, _), t in zip(named, out)])
    return M, S, dev, out


def lookahead_expand(boards, dice, cube_layer=3):
    """The leaves of predict_lookahead's tree as observations (ewn_lookahead_expand): boards [S, S] or [M, S, S], dice [M]
    -> (leaf_boards int8 [M, 648, S, S], leaf_dice int8 [M, 648], kind int8 [M, 108]).  Tuple t = 18 (3 f + r) + 3 (cube - 1) + direction
    is the agent's move (f, r) followed by the reply of the opponent's cube in that direction; kind[m, t] is 0 where there is no such
    reply (or the root leaves the board, wins, or repeats roots 0..2), 1 where the reply wins for the opponent, 2 for a leaf.  Row
    6 t + d2 - 1 holds the board after both moves and the dice d2 where kind is 2, a zero board and d2 elsewhere.  predict_lookahead's
    argument checks."""
    M, S, dev, (b, d) = _stage_inputs("lookahead_expand", [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                                           ("dice", dice, torch.int8, lambda M, S: (M,))], cube_layer)
    lb = torch.empty((M, LA_ROWS, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty((M, LA_ROWS), dtype=torch.int8, device=dev)
    kind = torch.empty((M, LA_TUPLES), dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_expand(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(lb), _ptr(ld), _ptr(kind), _stream()),
              "ewn_lookahead_expand")
    return lb, ld, kind


def lookahead_reduce(boards, dice, kind, leaf, terminal_value=1.0, return_q=False, cube_layer=3):
    """Leaf values folded back into Q and the action (ewn_lookahead_reduce): boards, dice as lookahead_expand took them,
    kind as it returned it, leaf float32 [M, 648] (a value per leaf row) or [M, 648, 6] (a q row per leaf row: its maximum is the
    row's value) -> actions int8 [M, 2], with return_q the float32 [M, 2, 3] Q as well.  The arithmetic is predict_lookahead's: with
    leaf = predict_policy(leaf rows, return_value=True)'s values the result is predict_lookahead's, bit for bit."""
    who = "lookahead_reduce"
    if not math.isfinite(float(terminal_value)):
        raise ValueError("%s: terminal_value must be finite, got %r" % (who, terminal_value))
    shp = tuple(leaf.shape) if isinstance(leaf, torch.Tensor) else np.asarray(leaf).shape
    if not (len(shp) in (2, 3) and shp[1] == LA_ROWS and (len(shp) == 2 or shp[2] == 6)):
        raise ValueError("%s: leaf must have shape [M, 648] or [M, 648, 6], got %s" % (who, list(shp)))
    width = 6 if len(shp) == 3 else 1
    M, S, dev, (b, d, k, lf) = _stage_inputs(who, [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                                  ("dice", dice, torch.int8, lambda M, S: (M,)),
                                                  ("kind", kind, torch.int8, lambda M, S: (M, LA_TUPLES)),
                                                  ("leaf", leaf, torch.float32, lambda M, S: (M, LA_ROWS, width))], cube_layer)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_reduce(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(k), _ptr(lf), width,
                                               C.c_float(float(terminal_value)), _ptr(acts), _ptr(q), _stream()), "ewn_lookahead_reduce")
    return (acts, q) if return_q else acts


def _leaf_table(who, table, M, S):
    """endgame_table= of a search on M SxS boards: None, or an EndgameTable for that size, else ValueError (EndgameTable.lookup's
    texts); that it lives on the GPU of the rest is the caller's _same_gpu"""
    from .endgame import EndgameTable
    if table is None:
        return None
    if not isinstance(table, EndgameTable):
        raise ValueError("%s: endgame_table must be an EndgameTable, got %s" % (who, type(table).__name__))
    if table.board_size != S:
        raise ValueError("%s: boards of shape %s, the table is for %dx%d" % (who, [M, S, S], table.board_size, table.board_size))
    return table


def predict_lookahead(boards, dice, params, terminal_value=1.0, return_q=False, cube_layer=3, plies=1, chunk=1024, endgame_table=None,
                      return_leaf_counts=False):
    """What the trained actor-critic plays when it looks one move ahead with its own value net (ewn_predict_lookahead):
    per observation and env action (f, r), Q = -inf for a move that leaves the board, +terminal_value for one that wins, otherwise the
    mean over the opponent's dice of its best (minimal) reply, a reply being worth -terminal_value if it wins for the opponent and
    else the mean over the agent's next dice of the value net there.  Plain expectiminimax, no pruning.  boards [S, S] or [M, S, S],
    dice [M] (outside 1..6: clamped), params as predict_policy takes them -> actions int8 [M, 2] (the first maximum of Q), and with
    return_q the float32 [M, 2, 3] Q as well.  A row that is already over, or has no agent cube, gets (0, 0) and six -inf.  The same
    argument checks as predict_policy: anything the kernel cannot read in place raises ValueError before a launch.
    plies=2 looks two moves ahead: the same tree with each leaf V(b2, d2) replaced by the maximum of the one-move Q at
    (b2, d2) -- lookahead_expand, ewn_predict_lookahead on the 648 leaf rows per observation, lookahead_reduce -- `chunk` observations
    at a time on scratch allocated once per call (about 49 KB per observation of the chunk at 7x7).
    endgame_table (an EndgameTable of the boards' size on the same GPU): a leaf b2 that the table covers is worth
    terminal_value * E(b2), exactly, instead of the critic's mean there (ewn_predict_lookahead_eg); with plies=2 the table goes to the
    inner call on the 648 leaf rows.  return_leaf_counts (plies=1 with a table): the int16 [M, 2] counts of leaf tuples valued by the
    table and by the critic are returned last."""
    lib = _lib.load()
    if plies not in (1, 2):
        raise ValueError("predict_lookahead: plies must be 1 or 2, got %r" % (plies,))
    if int(chunk) < 1:
        raise ValueError("predict_lookahead: chunk must be at least 1, got %r" % (chunk,))
    if return_leaf_counts and plies != 1:
        raise ValueError("predict_lookahead: return_leaf_counts is the one-move call's (plies=1), got plies=%r" % (plies,))
    if return_leaf_counts and endgame_table is None:
        raise ValueError("predict_lookahead: return_leaf_counts needs an endgame_table")
    who = "predict_lookahead"
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    table = _leaf_table(who, endgame_table, M, S)
    dev = _policy_params(who, params, P, S)
    if not math.isfinite(float(terminal_value)):
        raise ValueError("predict_lookahead: terminal_value must be finite, got %r" % (terminal_value,))
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
    d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
    _same_gpu(who, dev, "params", (("params", params), ("boards", b), ("dice", d), ("the table", None if table is None else table.table)))
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    if plies == 2:
        return _predict_lookahead2(lib, S, int(cube_layer), M, b, d, params, float(terminal_value), acts, q, int(chunk), table)
    if table is None:
        with torch.cuda.device(dev):
            check(lib.ewn_predict_lookahead(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(params), C.c_float(float(terminal_value)),
                                            _ptr(acts), _ptr(q), _stream()), "ewn_predict_lookahead")
        return (acts, q) if return_q else acts
    counts = torch.zeros((M, 2), dtype=torch.int16, device=dev) if return_leaf_counts else None
    with torch.cuda.device(dev):
        check(lib.ewn_predict_lookahead_eg(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(params), C.c_float(float(terminal_value)),
                                           table.max_cubes, table.max_total, _ptr(table.table), _ptr(acts), _ptr(q), _ptr(counts),
                                           _stream()), "ewn_predict_lookahead_eg")
    out = (acts,) + tuple(t for t in (q, counts) if t is not None)
    return out[0] if len(out) == 1 else out


def _predict_lookahead2(lib, S, L, M, b, d, params, tv, acts, q, chunk, table=None):
    """predict_lookahead(plies=2) on checked inputs: per chunk of c observations expand -> ewn_predict_lookahead with q on the 648 c
    leaf rows (ewn_predict_lookahead_eg where there is a table) -> reduce at leaf_width 6; the scratch is one allocation per call,
    every row of it rewritten per chunk"""
    dev = params.device
    c = max(1, min(chunk, M, (2 ** 31 - 1) // LA_ROWS))  # a chunk's 648 c leaf rows are counted in an int
    lb = torch.empty((c * LA_ROWS, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty(c * LA_ROWS, dtype=torch.int8, device=dev)
    kind = torch.empty((c, LA_TUPLES), dtype=torch.int8, device=dev)
    la = torch.empty((c * LA_ROWS, 2), dtype=torch.int8, device=dev)
    lq = torch.empty((c * LA_ROWS, 6), dtype=torch.float32, device=dev)
    tvf = C.c_float(tv)
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            bi, di, ai, qi = b[i:i + n], d[i:i + n], acts[i:i + n], None if q is None else q[i:i + n]
            check(lib.ewn_lookahead_expand(S, L, n, _ptr(bi), _ptr(di), _ptr(lb), _ptr(ld), _ptr(kind), st), "ewn_lookahead_expand")
            if table is None:
                check(lib.ewn_predict_lookahead(S, L, LA_ROWS * n, _ptr(lb), _ptr(ld), _ptr(params), tvf, _ptr(la), _ptr(lq), st), "ewn_predict_lookahead")
            else:
                check(lib.ewn_predict_lookahead_eg(S, L, LA_ROWS * n, _ptr(lb), _ptr(ld), _ptr(params), tvf, table.max_cubes, table.max_total,
                                                   _ptr(table.table), _ptr(la), _ptr(lq), None, st), "ewn_predict_lookahead_eg")
            check(lib.ewn_lookahead_reduce(S, L, n, _ptr(bi), _ptr(di), _ptr(kind), _ptr(lq), 6, tvf, _ptr(ai), _ptr(qi), st),
                  "ewn_lookahead_reduce")
    return acts if q is None else (acts, q)


def lookahead_targets(q, temperature=0.0):
    """predict_lookahead's Q as training targets (ewn_lookahead_targets): q float32 [M, 2, 3] or [M, 6] on the GPU ->
    (target_pi float32 [M, 5], target_value float32 [M], weight float32 [M]).  A row of six -inf (a finished observation) gets zeros
    and weight 0; any other row weight 1 and its maximum as the value.  temperature 0: the search's action one-hot on both heads
    ((0.5, 0.5) on the flag head when both flags move the same cube); temperature > 0: the softmax of q / temperature over the
    moves that stay on the board, summed per head."""
    who = "lookahead_targets"
    t = float(temperature)
    if not math.isfinite(t) or t < 0.0:
        raise ValueError("%s: temperature must be finite and not negative, got %r" % (who, temperature))
    shp = tuple(q.shape) if isinstance(q, torch.Tensor) else np.asarray(q).shape
    if not (len(shp) in (2, 3) and math.prod(shp[1:]) == 6 and (len(shp) == 2 or shp[1:] == (2, 3))):
        raise ValueError("%s: q must have shape [M, 2, 3] or [M, 6], got %s" % (who, list(shp)))
    M = int(shp[0])
    dev = q.device if isinstance(q, torch.Tensor) else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")
    qq = _policy_input("q", q, torch.float32, (M, 6), dev, who=who)
    if not qq.is_cuda:
        raise ValueError("%s: q must live on the GPU, got %s" % (who, _describe(qq)))
    pi = torch.zeros((M, 5), dtype=torch.float32, device=dev)
    val = torch.zeros(M, dtype=torch.float32, device=dev)
    w = torch.zeros(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_targets(M, _ptr(qq), C.c_float(t), _ptr(pi), _ptr(val), _ptr(w), _stream()), "ewn_lookahead_targets")
    return pi, val, w


def sup_grad(boards, dice, target_pi, target_value, params, weight=None, pi_coef=1.0, vf_coef=0.5, cube_layer=3, out=None, scratch=None):
    """The gradient of a supervised loss on M given observations (ewn_sup_grad):
        loss = mean_m w_m (pi_coef * CE(target_pi[m], policy heads) + vf_coef * (V - target_value[m])^2)
    boards [S, S] or [M, S, S], dice [M], target_pi float32 [M, 5] (entries 0-1 the flag head, 2-4 the direction head; a head whose
    entries are all zero is masked), target_value [M], weight [M] or None (ones), params as predict_policy takes them -> float32
    [P + 8]: the gradient in the params layout, then the sums over the samples with weight > 0 of {w CE, w entropy, agreement
    count, w, w (V - v*)^2, 0, 0, 0}.  A row whose weight is 0 is skipped altogether (its targets may be NaN or infinite).  out: a
    float32 [P + 8] device tensor to write into; scratch: a 4-byte aligned uint8 device tensor of at least ewn_sup_scratch_bytes.  predict_policy's
    argument checks: anything the kernels cannot read in place raises ValueError before a launch.  The step is ewn_a2c_apply."""
    who = "sup_grad"
    lib = _lib.load()
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    if M < 1:
        raise ValueError("%s: needs at least one observation (a mean over nothing is undefined)" % who)
    dev = _policy_params(who, params, P, S)
    for name, v in (("pi_coef", pi_coef), ("vf_coef", vf_coef)):
        if not math.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError("%s: %s must be finite and not negative, got %r" % (who, name, v))
    named = [("boards", _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)),
             ("dice", _policy_input("dice", dice, torch.int8, (M,), dev, who=who)),
             ("target_pi", _policy_input("target_pi", target_pi, torch.float32, (M, 5), dev, who=who)),
             ("target_value", _policy_input("target_value", target_value, torch.float32, (M,), dev, who=who)),
             ("weight", None if weight is None else _policy_input("weight", weight, torch.float32, (M,), dev, who=who))]
    nscr = int(lib.ewn_sup_scratch_bytes(S, int(cube_layer), M))
    if out is not None:
        named.append(("out", _policy_input("out", out, torch.float32, (P + 8,), dev, who=who)))
    if scratch is not None and not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.uint8 and scratch.is_contiguous()
                                    and scratch.numel() >= nscr and scratch.data_ptr() % 4 == 0):
        raise ValueError("%s: scratch must be a contiguous, 4-byte aligned uint8 tensor of at least %d elements, got %s%s" % (
            who, nscr, _describe(scratch), " at an address that is %d past a multiple of 4" % (scratch.data_ptr() % 4)
            if isinstance(scratch, torch.Tensor) and scratch.data_ptr() % 4 else ""))
    _same_gpu(who, dev, "params", [("params", params)] + named + [("scratch", scratch)])
    b, d, tp, tv, w = (t for _, t in named[:5])
    grad = out if out is not None else torch.zeros(P + 8, dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.zeros(nscr, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.ewn_sup_grad(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(tp), _ptr(tv), _ptr(w), _ptr(params), C.c_float(float(pi_coef)),
                               C.c_float(float(vf_coef)), _ptr(grad), _ptr(scratch), _stream()), "ewn_sup_grad")
    return grad


LA_TUPLES = 108        # (agent move, reply) tuples per observation of the lookahead tree (csrc/ewn_lookahead.hpp)
LA_ROWS = 648          # its leaf rows: a tuple under each of the six d2
PUCT_LAYOUT = 1        # the version of a PUCT tree's layout (csrc/ewn_puct.hip); begin writes it into every header
PUCT_MAX_SIMS = 4096
PUCT_FUSED_TILE = 32          # the most trees a block of ewn_puct_search holds at a time (csrc/ewn_puct_fused.hip) ...
PUCT_FUSED_MAX_BLOCKS = 256   # ... and its grid's cap: more tiles are walked grid-stride


def _puct_sections(S, sims):
    """a PUCT tree's sections: ({name: (byte offset, dtype, shape per tree)}, bytes of one tree)"""
    N = sims + 1
    secs, o = {}, 0
    for name, dt, shape in (("hdr", torch.int32, (8,)), ("n", torch.int32, (N, 6)), ("w", torch.float32, (N, 6)),
                            ("p", torch.float32, (N, 6)), ("child", torch.int16, (N, 6, 6)), ("cn", torch.int16, (N, 6, 6)),
                            ("parent", torch.int16, (N, 4)), ("kind", torch.int8, (N, 6)), ("dice", torch.int8, (N,)),
                            ("board", torch.int8, (N, S, S))):
        secs[name] = (o, dt, shape)
        o += (math.prod(shape) * dt.itemsize + 3) // 4 * 4
    return secs, o


def _puct_numbers(who, sims, c_puct=0.0, terminal_value=1.0):
    if not (isinstance(sims, (int, np.integer)) and 0 <= int(sims) <= PUCT_MAX_SIMS):
        raise ValueError("%s: sims must be an integer in 0..%d, got %r" % (who, PUCT_MAX_SIMS, sims))
    if not math.isfinite(float(c_puct)) or float(c_puct) < 0.0:
        raise ValueError("%s: c_puct must be finite and not negative, got %r" % (who, c_puct))
    if not math.isfinite(float(terminal_value)) or not float(terminal_value) > 0.0:
        raise ValueError("%s: terminal_value must be finite and positive, got %r" % (who, terminal_value))
    return int(sims)


def _puct_tree(who, tree, S, sims, cube_layer=3):
    """the checked tree buffer: a contiguous uint8 device tensor [M, tree_bytes] at a 4-byte aligned address -> (M, tree_bytes)"""
    nb = int(_lib.load().ewn_puct_tree_bytes(int(S), int(cube_layer), sims))
    if nb < 0:
        raise ValueError("%s: no policy network for %dx%d boards with cube_layer %d (served: cube_layer 3 on 5x5 and 7x7)" % (
            who, S, S, cube_layer))
    if not (isinstance(tree, torch.Tensor) and tree.dtype == torch.uint8 and tree.dim() == 2 and tree.shape[1] == nb
            and tree.is_contiguous() and tree.data_ptr() % 4 == 0):
        raise ValueError("%s: tree must be a contiguous, 4-byte aligned uint8 tensor [M, %d] (puct_begin's, for sims=%d on %dx%d), got %s" % (
            who, nb, sims, S, S, _describe(tree)))
    return int(tree.shape[0]), nb


def puct_tree_views(tree, board_size, sims):
    """Tensor views onto the sections of puct_begin's trees (uint8 [M, tree_bytes]; layout PUCT_LAYOUT), nothing is
    copied: count, done, pending, degenerate int32 [M]; n int32, w, p float32 [M, sims + 1, 6] per node and edge a = 3 f + r;
    child, cn int16 [M, sims + 1, 6, 6] per node, edge and dice d' - 1; parent int16 [M, sims + 1, 4] (node, edge, dice, 0; the
    root: -1, 0, 0, 0); kind int8 [M, sims + 1, 6]; dice int8 [M, sims + 1]; board int8 [M, sims + 1, S, S].  Rows of nodes
    count .. sims are as puct_begin left them: zeros, child -1."""
    sims = _puct_numbers("puct_tree_views", sims)
    S = int(board_size)
    secs, nb = _puct_sections(S, sims)
    if not (isinstance(tree, torch.Tensor) and tree.dtype == torch.uint8 and tree.dim() == 2 and tree.shape[1] == nb
            and tree.stride(1) == 1 and tree.stride(0) % 4 == 0 and tree.storage_offset() % 4 == 0):
        raise ValueError("puct_tree_views: tree must be a uint8 tensor [M, %d] (puct_begin's, for sims=%d on %dx%d), got %s" % (
            nb, sims, S, S, _describe(tree)))
    out = {}
    for name, (o, dt, shape) in secs.items():
        out[name] = tree[:, o:o + math.prod(shape) * dt.itemsize].view(dt).unflatten(1, shape)
    hdr = out.pop("hdr")
    out.update(count=hdr[:, 0], done=hdr[:, 1], pending=hdr[:, 2], degenerate=hdr[:, 3])
    return out


def puct_begin(boards, dice, sims, cube_layer=3):
    """The trees of a PUCT search on M observations (ewn_puct_begin): boards [S, S] or [M, S, S], dice [M] (outside
    1..6: clamped) -> (tree uint8 [M, tree_bytes], leaf_boards int8 [M, S, S], leaf_dice int8 [M]).  Every byte of the trees is
    written; the root is the pending leaf and the leaf row its observation, except where the observation is already over or a side
    has no cube: that tree is degenerate and its leaf row a zero board with dice 1.  predict_lookahead's argument checks."""
    who = "puct_begin"
    sims = _puct_numbers(who, sims)
    M, S, dev, (b, d) = _stage_inputs(who, [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                            ("dice", dice, torch.int8, lambda M, S: (M,))], cube_layer)
    lib = _lib.load()
    nb = int(lib.ewn_puct_tree_bytes(S, int(cube_layer), sims))
    tree = torch.empty((M, nb), dtype=torch.uint8, device=dev)
    lb = torch.empty((M, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty(M, dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(lib.ewn_puct_begin(S, int(cube_layer), M, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()), "ewn_puct_begin")
    return tree, lb, ld


def _noise_eps(who, noise_eps):
    if not (math.isfinite(float(noise_eps)) and 0.0 <= float(noise_eps) <= 1.0):
        raise ValueError("%s: noise_eps must be a finite number in [0, 1], got %r" % (who, noise_eps))
    return float(noise_eps)


def puct_advance(tree, logits, value, leaf_boards, leaf_dice, sims, c_puct=1.5, terminal_value=1.0, board_size=None, cube_layer=3,
                 root_noise=None, noise_eps=0.25):
    """One round of the search (ewn_puct_advance): logits float32 [M, 5] and value float32 [M] are predict_policy's on
    the leaf rows.  Per tree the pending leaf is evaluated (priors from the logits, v = value / terminal_value clamped to [-1, 1])
    and backed up; then, while fewer than `sims` simulations have begun, one more walks down to a new leaf, or ends at once on a
    winning move.  tree, leaf_boards and leaf_dice are updated in place (a tree without a pending leaf: a zero board with dice 1) and
    returned.  board_size: taken from leaf_boards [M, S, S] when None.  sims + 1 rounds after puct_begin complete the search.
    root_noise (float32 [M, 2, 3] or [M, 6], un-normalised weights, e.g. Gamma variates): ewn_puct_advance_noise
    instead -- where the leaf evaluated is the root, its priors become (1 - noise_eps) P + noise_eps eta / sum(eta) over the legal
    edges with a finite positive weight.  None: exactly the plain call, noise_eps is not looked at."""
    who = "puct_advance"
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = None if root_noise is None else _noise_eps(who, noise_eps)
    for name, t in (("tree", tree), ("leaf_boards", leaf_boards), ("leaf_dice", leaf_dice)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s is updated in place and must be a tensor, got %s" % (who, name, _describe(t)))
    if board_size is not None and not (leaf_boards.dim() == 3 and leaf_boards.shape[1] == int(board_size)):
        raise ValueError("%s: leaf_boards must have shape [M, %d, %d], got %s" % (who, int(board_size), int(board_size), list(leaf_boards.shape)))
    M, S, dev, (lb, lg, v, ld) = _stage_inputs(who, [("leaf_boards", leaf_boards, torch.int8, lambda M, S: (M, S, S)),
                                                    ("logits", logits, torch.float32, lambda M, S: (M, 5)),
                                                    ("value", value, torch.float32, lambda M, S: (M,)),
                                                    ("leaf_dice", leaf_dice, torch.int8, lambda M, S: (M,))], cube_layer)
    Mt, _ = _puct_tree(who, tree, S, sims, cube_layer)
    if Mt != M or not (tree.is_cuda and tree.device == dev):
        raise ValueError("%s: tree must hold %d trees on %s, got %s" % (who, M, dev, _describe(tree)))
    if root_noise is not None:
        rn = _policy_input("root_noise", root_noise, torch.float32, (M, 6), dev, who=who)
        _same_gpu(who, dev, "leaf_boards", (("root_noise", rn),))
        with torch.cuda.device(dev):
            check(_lib.load().ewn_puct_advance_noise(S, int(cube_layer), M, sims, C.c_float(float(c_puct)), C.c_float(float(terminal_value)),
                                                     _ptr(tree), _ptr(lg), _ptr(v), _ptr(rn), C.c_float(eps), _ptr(lb), _ptr(ld), _stream()),
                  "ewn_puct_advance_noise")
        return tree, leaf_boards, leaf_dice
    with torch.cuda.device(dev):
        check(_lib.load().ewn_puct_advance(S, int(cube_layer), M, sims, C.c_float(float(c_puct)), C.c_float(float(terminal_value)), _ptr(tree),
                                           _ptr(lg), _ptr(v), _ptr(lb), _ptr(ld), _stream()), "ewn_puct_advance")
    return tree, leaf_boards, leaf_dice


def puct_result(tree, board_size, sims, return_visits=False, return_q=False, return_value=False, cube_layer=3):
    """What the search found at the roots (ewn_puct_result) -> actions int8 [M, 2], or the tuple (actions, visits int32
    [M, 2, 3] if return_visits, q float32 [M, 2, 3] if return_q, value float32 [M] if return_value).  The action is the first root
    move that wins if there is one, else the first maximum of the visits over the searched moves; q is -inf where (f, r) is no
    action, +1 where it wins, else W / N (0 unvisited), value sum W / sum N, both in units of the terminal value.  A degenerate row:
    (0, 0), zero visits, six -inf, 0."""
    who = "puct_result"
    sims = _puct_numbers(who, sims)
    S = int(board_size)
    M, _ = _puct_tree(who, tree, S, sims, cube_layer)
    if not tree.is_cuda:
        raise ValueError("%s: tree must live on the GPU, got %s" % (who, _describe(tree)))
    dev = tree.device
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    with torch.cuda.device(dev):
        check(_lib.load().ewn_puct_result(S, int(cube_layer), M, _ptr(tree), _ptr(acts), _ptr(visits), _ptr(q), _ptr(val), _stream()),
              "ewn_puct_result")
    out = (acts,) + tuple(t for t in (visits, q, val) if t is not None)
    return out[0] if len(out) == 1 else out


def _fused_table(who, fused, endgame_table):
    if fused and endgame_table is not None:
        raise ValueError("%s: fused=True does not take an endgame_table: the exact-leaf substitution is the staged path's (fused=False)" % who)


def _puct_scratch(c, nb, S, dev, fused):
    """a search's scratch for c observations: (tree, leaf boards, leaf dice, leaf actions, logits, value); fused: the tree alone"""
    tree = torch.empty((c, nb), dtype=torch.uint8, device=dev)
    if fused:
        return (tree, None, None, None, None, None)
    return (tree, torch.empty((c, S, S), dtype=torch.int8, device=dev), torch.empty(c, dtype=torch.int8, device=dev),
            torch.empty((c, 2), dtype=torch.int8, device=dev), torch.empty((c, 5), dtype=torch.float32, device=dev),
            torch.empty(c, dtype=torch.float32, device=dev))


def puct_search(boards, dice, params, sims, c_puct=1.5, terminal_value=1.0, root_noise=None, noise_eps=0.25, rounds=None, cube_layer=3,
                out=None):
    """The whole PUCT search of M observations in one launch (ewn_puct_search) -> tree uint8 [M, tree_bytes]: byte for
    byte what puct_begin and then `rounds` rounds of predict_policy on the leaf rows and puct_advance leave (the first round with
    root_noise and noise_eps when root_noise is given: float32 [M, 2, 3] or [M, 6], puct_advance's).  rounds None: all sims + 1;
    an integer: min(rounds, sims + 1), 0 is puct_begin alone.  puct_result, puct_play and puct_tree_views read the tree.  out: a
    contiguous, 4-byte aligned uint8 tensor [M, tree_bytes] to write into (what it held does not matter).  predict_puct's argument
    checks."""
    who = "puct_search"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = 0.0 if root_noise is None else _noise_eps(who, noise_eps)
    if rounds is not None and not (isinstance(rounds, (int, np.integer)) and int(rounds) >= 0):
        raise ValueError("%s: rounds must be None or an integer that is not negative, got %r" % (who, rounds))
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    L = int(cube_layer)
    dev = _policy_params(who, params, P, S)
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
    d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
    rn = None if root_noise is None else _policy_input("root_noise", root_noise, torch.float32, (M, 6), dev, who=who)
    _same_gpu(who, dev, "params", (("params", params), ("boards", b), ("dice", d), ("root_noise", rn)))
    if out is None:
        out = torch.empty((M, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    else:
        Mt, _ = _puct_tree(who, out, S, sims, cube_layer)
        if Mt != M or not (out.is_cuda and out.device == dev):
            raise ValueError("%s: out must hold %d trees on %s, got %s" % (who, M, dev, _describe(out)))
    with torch.cuda.device(dev):
        check(lib.ewn_puct_search(S, L, M, sims, -1 if rounds is None else min(int(rounds), sims + 1), C.c_float(float(c_puct)),
                                  C.c_float(float(terminal_value)), _ptr(b), _ptr(d), _ptr(params), _ptr(rn), C.c_float(eps), _ptr(out),
                                  _stream()), "ewn_puct_search")
    return out


def _puct_search(lib, S, L, n, sims, b, d, params, cp, tv, table, scratch, st, noise=None, eps=0.0, fused=False):
    """predict_puct's and selfplay_puct's search of n observations on the caller's scratch: begin, then sims + 1 rounds of
    ewn_predict_policy and advance.  noise (float32 [n, 6]): the first round, which evaluates the roots, is the noise instance's.
    fused: the one launch of ewn_puct_search instead -- the same bytes in the tree; of the scratch only the tree is used"""
    tree, lb, ld, la, lg, lv = scratch
    if fused:
        check(lib.ewn_puct_search(S, L, n, sims, -1, cp, tv, _ptr(b), _ptr(d), _ptr(params), _ptr(noise), C.c_float(eps), _ptr(tree), st),
              "ewn_puct_search")
        return
    check(lib.ewn_puct_begin(S, L, n, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), st), "ewn_puct_begin")
    for rnd in range(sims + 1):
        check(lib.ewn_predict_policy(S, L, n, _ptr(lb), _ptr(ld), _ptr(params), 1, C.c_uint64(0), None, None, _ptr(la), _ptr(lg),
                                     _ptr(lv), st), "ewn_predict_policy")
        if table is not None:                                  # a tree without a pending leaf shows a zero board: not covered
            _, covered, q_exact = table.lookup(lb[:n], ld[:n], return_q=True)
            lv[:n] = torch.where(covered, tv.value * q_exact.reshape(n, 6).max(1).values, lv[:n])
        if rnd == 0 and noise is not None:
            check(lib.ewn_puct_advance_noise(S, L, n, sims, cp, tv, _ptr(tree), _ptr(lg), _ptr(lv), _ptr(noise), C.c_float(eps), _ptr(lb),
                                             _ptr(ld), st), "ewn_puct_advance_noise")
        else:
            check(lib.ewn_puct_advance(S, L, n, sims, cp, tv, _ptr(tree), _ptr(lg), _ptr(lv), _ptr(lb), _ptr(ld), st), "ewn_puct_advance")


def predict_puct(boards, dice, params, sims=64, c_puct=1.5, terminal_value=1.0, return_visits=False, return_q=False, return_value=False,
                 cube_layer=3, chunk=1024, endgame_table=None, fused=False):
    """What the trained actor-critic plays after a PUCT search of `sims` simulations on its own two heads: the policy
    head says where to look, the value head what a leaf is worth, a move that wins on the board is worth +1 and is played; the
    opponent's and the agent's later dice are chance nodes sampled in a fixed stratified order, so the search is deterministic.
    boards [S, S] or [M, S, S], dice [M] (outside 1..6: clamped), params as predict_policy takes them -> actions int8 [M, 2], or the
    tuple (actions, visits int32 [M, 2, 3], q float32 [M, 2, 3], value float32 [M]) of what was asked for, as puct_result returns
    them.  sims=0: no search, zero visits, the first legal move unless one wins.  The stages are puct_begin, then sims + 1 rounds of
    ewn_predict_policy on the leaf rows and puct_advance, then puct_result, `chunk` observations at a time on scratch allocated once
    per call (a tree is 256 bytes per simulation at 5x5, 280 at 7x7).  predict_lookahead's argument checks.
    endgame_table (an EndgameTable of the boards' size on the same GPU): a pending leaf that the table covers is worth
    terminal_value * max_a q_exact(leaf board, leaf dice) instead of the value head's output; the logits are the policy head's.
    fused=True: each chunk's search is the one launch of ewn_puct_search -- the same trees byte for byte, so the same
    results bit for bit, and no leaf-row scratch; not together with endgame_table (the exact leaves stay on the staged path)."""
    who = "predict_puct"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    _fused_table(who, fused, endgame_table)
    if int(chunk) < 1:
        raise ValueError("%s: chunk must be at least 1, got %r" % (who, chunk))
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    table = _leaf_table(who, endgame_table, M, S)
    L = int(cube_layer)
    dev = _policy_params(who, params, P, S)
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
    d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
    _same_gpu(who, dev, "params", (("params", params), ("boards", b), ("dice", d), ("the table", None if table is None else table.table)))
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    c = max(1, min(int(chunk), M))
    nb = int(lib.ewn_puct_tree_bytes(S, L, sims))
    scratch = _puct_scratch(c, nb, S, dev, fused)
    tree = scratch[0]
    cp, tv = C.c_float(float(c_puct)), C.c_float(float(terminal_value))
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            sl = slice(i, i + n)
            _puct_search(lib, S, L, n, sims, b[sl], d[sl], params, cp, tv, table, scratch, st, fused=fused)
            check(lib.ewn_puct_result(S, L, n, _ptr(tree), _ptr(acts[sl]), _ptr(None if visits is None else visits[sl]),
                                      _ptr(None if q is None else q[sl]), _ptr(None if val is None else val[sl]), st), "ewn_puct_result")
    out = (acts,) + tuple(t for t in (visits, q, val) if t is not None)
    return out[0] if len(out) == 1 else out


SELFPLAY_MAX_PLIES = {5: 80, 7: 128}   # above the rules' bound on a game's length: 69 / 117 plies
_PLAY_ROWS = (("board", torch.int8, lambda S: (S, S)), ("dice", torch.int8, lambda S: ()), ("visits", torch.int32, lambda S: (2, 3)),
              ("value", torch.float32, lambda S: ()), ("action", torch.int8, lambda S: (2,)), ("live", torch.int8, lambda S: ()))


def _play_numbers(who, temp_plies, key, game_offset):
    if not (isinstance(temp_plies, (int, np.integer)) and 0 <= int(temp_plies) <= 2 ** 31 - 1):
        raise ValueError("%s: temp_plies must be an integer that is not negative, got %r" % (who, temp_plies))
    if not (isinstance(key, (int, np.integer)) and isinstance(game_offset, (int, np.integer)) and -2 ** 63 <= int(game_offset) < 2 ** 63):
        raise ValueError("%s: key and game_offset must be integers, game_offset within 64 bits, got %r and %r" % (who, key, game_offset))
    return int(temp_plies), int(key) & 0xFFFFFFFFFFFFFFFF, int(game_offset)


def puct_play(tree, boards, dice, game, board_size, sims, temp_plies=0, key=0, game_offset=0, out=None, cube_layer=3):
    """One ply of M self-play games off their searched trees (ewn_puct_play; puct_result's checks of the tree).  boards
    int8 [M, S, S], dice int8 [M] and game int32 [M, 4] = (ply, over, winner, 0) are updated in place: the move is the first root
    move that wins, else drawn in proportion to the root's visits while ply < temp_plies (a Philox word of key, game_offset + m and
    ply), else the first maximum of the visits; the next dice is a second word of the same block.  The position played and recorded
    is the tree's root.  A game that is over, or whose tree is degenerate, is left as it is (the latter is then over, without a
    winner).  out: None -> a new record row {board int8 [M, S, S], dice int8 [M], visits int32 [M, 2, 3], value float32 [M], action
    int8 [M, 2], live int8 [M]} is returned; a dict -> the tensors it holds under those names are written (a missing name or None:
    not written) and it is returned."""
    who = "puct_play"
    sims = _puct_numbers(who, sims)
    temp_plies, key, game_offset = _play_numbers(who, temp_plies, key, game_offset)
    S = int(board_size)
    M, _ = _puct_tree(who, tree, S, sims, cube_layer)
    for name, t, dtype, shape in (("boards", boards, torch.int8, (M, S, S)), ("dice", dice, torch.int8, (M,)), ("game", game, torch.int32, (M, 4))):
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("%s: %s is updated in place and must be a contiguous %s tensor of shape %s, got %s" % (
                who, name, str(dtype).replace("torch.", ""), list(shape), _describe(t)))
    if out is not None and (not isinstance(out, dict) or set(out) - {name for name, _, _ in _PLAY_ROWS}):
        raise ValueError("%s: out must be a dict with keys among board, dice, visits, value, action, live, got %r" % (
            who, sorted(out) if isinstance(out, dict) else type(out).__name__))
    if not tree.is_cuda:
        raise ValueError("%s: tree must live on the GPU, got %s" % (who, _describe(tree)))
    dev = tree.device
    _same_gpu(who, dev, "tree", (("boards", boards), ("dice", dice), ("game", game)))
    if out is None:
        out = {name: torch.zeros((M,) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}
    rows = []
    for name, dt, shape in _PLAY_ROWS:
        t = out.get(name)
        if t is not None:
            if isinstance(t, torch.Tensor) and t.dtype == torch.bool and dt == torch.int8:
                t = t.view(torch.int8)
            if not (_is_buffer(t, dt) and t.numel() == M * math.prod(shape(S))):
                raise ValueError("%s: out[%r] must be a contiguous %s device tensor of %s elements, got %s" % (
                    who, name, str(dt).replace("torch.", ""), " x ".join(map(str, (M,) + shape(S))), _describe(t)))
            _same_gpu(who, dev, "tree", ((("out[%r]" % name), t),))
        rows.append(t)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_puct_play(S, int(cube_layer), M, _ptr(tree), _ptr(boards), _ptr(dice), _ptr(game), temp_plies, C.c_uint64(key),
                                        C.c_int64(game_offset), *[_ptr(t) for t in rows], _stream()), "ewn_puct_play")
    return out


def selfplay_outcomes(winner, live):
    """The value targets of self-play records whose games all start at ply 0 in row 0 (plain torch): winner [M] (0 none, +1 the side
    that moves at even plies, -1 the other), live bool [T, M] -> (z float32 [T, M], weight float32 [T, M]).  z[t, m] is the result
    seen from the side to move in row t: winner[m] at even t, -winner[m] at odd t, on live rows; weight is 1 on the live rows of
    finished games.  Everything else is 0."""
    live = live.to(torch.bool)
    w = winner.to(torch.float32)[None, :]
    sign = 1.0 - 2.0 * (torch.arange(live.shape[0], device=live.device) % 2).to(torch.float32)
    counts = live & (w != 0)
    z = torch.where(counts, w * sign[:, None], torch.zeros((), device=live.device))
    return z.contiguous(), counts.to(torch.float32).contiguous()


def selfplay_noise(M, noise_alpha, key, game_offset, ply, device="cuda"):
    """selfplay_puct's root noise of one ply: float32 [M, 6] Gamma(noise_alpha) variates (torch._standard_gamma) on a generator seeded
    from key, game_offset and the ply.  Normalised over the legal edges by the kernel they are Dirichlet(noise_alpha) noise."""
    gen = torch.Generator(device=device)
    gen.manual_seed((int(key) * 0x9E3779B97F4A7C15 + int(game_offset) * 0xD1B54A32D192ED03 + int(ply) * 0x2545F4914F6CDD1D) & (2 ** 63 - 1))
    return torch._standard_gamma(torch.full((int(M), 6), float(noise_alpha), dtype=torch.float32, device=device), generator=gen)


def selfplay_puct(boards, dice, params, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.25, noise_alpha=1.0,
                  temp_plies=8, key=0, game_offset=0, chunk=1024, check_every=8, endgame_table=None, cube_layer=3, fused=False):
    """M games of the PUCT search against itself, from the given positions to the end: per ply puct_begin, sims + 1
    rounds of ewn_predict_policy and advance -- the first with Dirichlet(noise_alpha) noise of weight noise_eps on the root's priors
    (ewn_puct_advance_noise) -- then ewn_puct_play into row t: the move is drawn in proportion to the visits for the first
    temp_plies plies of a game and is the most visited one after that.  boards [S, S] or [M, S, S], dice [M], params as
    predict_policy takes them; they are not changed.  `chunk` games are played at a time, each chunk to its end; every check_every
    plies one host read ends a chunk whose games are all over.  max_plies None: 80 on 5x5, 128 on 7x7 -- a move lowers the mover's
    summed distance to its corner by at least one, so a game lasts at most 69 / 117 plies.  noise_alpha = 1.0 is a choice (about 10
    over the number of moves, AlphaZero's rule of thumb), not a measurement.  endgame_table: predict_puct's, at the leaves.
    fused=True: a ply's search is the one launch of ewn_puct_search, the records are the same bit for bit; not
    together with endgame_table.
    The noise is torch._standard_gamma on a generator seeded from key, game_offset and the ply, drawn once per ply for all M games
    and read by each chunk's rows: a call repeats itself bit for bit, whatever the chunk.  Returns a dict: board int8 [T, M, S, S], dice int8
    [T, M], visits int32 [T, M, 2, 3], value float32 [T, M], action int8 [T, M, 2], live bool [T, M] (T = max_plies; rows past a
    game's end are zero), z and weight float32 [T, M] (selfplay_outcomes), winner int32 [M], plies int32 [M]."""
    who = "selfplay_puct"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    _fused_table(who, fused, endgame_table)
    eps = _noise_eps(who, noise_eps)
    temp_plies, key, game_offset = _play_numbers(who, temp_plies, key, game_offset)
    if not (math.isfinite(float(noise_alpha)) and float(noise_alpha) > 0.0):
        raise ValueError("%s: noise_alpha must be finite and positive, got %r" % (who, noise_alpha))
    if int(chunk) < 1 or int(check_every) < 1:
        raise ValueError("%s: chunk and check_every must be at least 1, got %r and %r" % (who, chunk, check_every))
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    T = SELFPLAY_MAX_PLIES[S] if max_plies is None else max_plies
    if not (isinstance(T, (int, np.integer)) and int(T) >= 1):
        raise ValueError("%s: max_plies must be a positive integer or None, got %r" % (who, max_plies))
    T = int(T)
    table = _leaf_table(who, endgame_table, M, S)
    L = int(cube_layer)
    dev = _policy_params(who, params, P, S)
    b = _policy_input("boards", boards, torch.int8, (M, S, S), dev, who=who)
    d = _policy_input("dice", dice, torch.int8, (M,), dev, who=who)
    _same_gpu(who, dev, "params", (("params", params), ("boards", b), ("dice", d), ("the table", None if table is None else table.table)))
    rec = {name: torch.zeros((T, M) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}
    game = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    c = max(1, min(int(chunk), M))
    nb = int(lib.ewn_puct_tree_bytes(S, L, sims))
    scratch = _puct_scratch(c, nb, S, dev, fused)
    cp, tv = C.c_float(float(c_puct)), C.c_float(float(terminal_value))
    with torch.cuda.device(dev):
        st = _stream()
        drawn = []
        for i in range(0, M, c):
            n = min(c, M - i)
            cb, cd, cg = b[i:i + n].clone(), d[i:i + n].clone(), game[i:i + n]
            for t in range(T):
                noise = None
                if eps > 0.0:
                    if t == len(drawn):                        # a ply's noise is drawn once, for all M games: later chunks read their rows
                        drawn.append(selfplay_noise(M, noise_alpha, key, game_offset, t, dev))
                    noise = drawn[t][i:i + n]
                _puct_search(lib, S, L, n, sims, cb, cd, params, cp, tv, table, scratch, st, noise, eps, fused)
                check(lib.ewn_puct_play(S, L, n, _ptr(scratch[0]), _ptr(cb), _ptr(cd), _ptr(cg), temp_plies, C.c_uint64(key),
                                        C.c_int64(game_offset + i), *[_ptr(rec[name][t, i:i + n]) for name, _, _ in _PLAY_ROWS], st),
                      "ewn_puct_play")
                if (t + 1) % int(check_every) == 0 and bool(cg[:, 1].all()):
                    break
    rec["live"] = rec["live"].view(torch.bool)
    rec["winner"], rec["plies"] = game[:, 2].contiguous(), game[:, 0].contiguous()
    rec["z"], rec["weight"] = selfplay_outcomes(rec["winner"], rec["live"])
    return rec
