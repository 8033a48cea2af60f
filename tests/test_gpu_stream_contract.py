"""The four promises of the first paragraph of include/ewn_hip.h, held against every entry whose last parameter is `void *stream`:
nothing is allocated, freed or synchronised inside a call (so it can be captured into a hipGraph), every launch goes to the caller's
stream, nothing is carried from one call to the next outside the caller's buffers, and calls that share no buffer may run on two
threads.  The values themselves are other modules' business; here every comparison is of all bytes and there is no tolerance.

One table, CASES: an entry, a configuration and a builder that returns the ctypes argument list over preallocated device buffers
together with the role of every buffer (Live, below).  Every case has two valid input sets
A and B (real positions, dice in range, reset states); every input buffer holds one of them at every moment, so a launch that runs at
the wrong time computes the wrong answer and can never read out of bounds.

 (a) captured, nothing runs; replayed, the eager bytes.  E_A / E_B are recorded eagerly (two eager calls on the same inputs must agree:
     the precondition).  The one call is then captured on one stream (capture_error_mode="global"), its return code asserted 0
     inside the capture; after the capture every output still holds its 0xA5 fill and every in-place buffer is unchanged; a replay
     gives E_A.  Stateless entries: the scratch dirtied with 0x5A, B copied into the same buffers, replay -> E_B, A back -> E_A.
     Stateful entries (STATEFUL): three replays from the snapshot equal three eager calls from it, state and outputs after each one;
     then the same B / A swap.  An entry without a device input (ewn_endgame_build): three replays into refilled outputs, with a
     device-to-device copy between them.
 (b) a side stream is honoured, without any graph.  On s = torch.cuda.Stream(), with A in the inputs: a sleep, the copy of B into the
     inputs, the 0xA5 fill of the outputs, the entry, the copy of the outputs.  Only s is synchronised.  The result must be E_B; a
     launch on any other stream reads A behind the sleep's back and has its outputs overwritten by the fill.  E_A != E_B is required
     of every case that has a device input (ewn_endgame_build has none: the fill alone decides there).
     The sleep: torch.cuda._sleep(c), c chosen from one timed sleep so that it lasts about 20 ms, measured again and required to
     last at least 5 ms.  Measured on the MI355X: 1 000 000 cycles took 0.419 ms, so c = 47 718 574, and that sleep measured 19.8 ms.
 (c) two threads, two streams, disjoint buffers: each runs the cases of THREAD_SEQUENCE (every entry that calls
     hipFuncSetAttribute, every entry behind a `static const ... getenv` initialiser), the second thread in the opposite order; both
     must produce the single-thread bytes.  Run once: a failure is to be read out of the host code (shared mutable state).

ewn_step's scratch is the one buffer called scratch that is state by contract ("zero-initialised once and then left alone between
calls": the MT19937 refill queue, the split-phase hand-off), so it is an in-place buffer here, zero in A and in B; every other scratch
is filled with 0xFF before a call and 0x5A between replays.

Site -> case.  Every `<<<` of csrc (LAUNCH_SITES has the per-file counts, tests/test_stream_contract_cpu.py compares them with the
sources), by file and function, with the cases that reach it.  There were two hipMemsetAsync as well, in ewn_playout_wins and in
ewn_endgame_build; property (a) found that a captured memset node of value 0 is not replayed faithfully by the ROCm 7.0 runtime (from
the second replay on it writes an 8-byte pattern that is not zero), so both are kernels now (k_zero_wins, k_endgame_clear),
MEMSET_SITES is empty and the CPU module keeps it so:

  ewn_kernels.hip (28)
    launch_minimax                 k_predict_minimax                  ewn_predict_minimax[no-tables]
    launch_minimax_sim             k_predict_minimax_sim              ewn_predict_minimax_sim[d1], ewn_step[split-sim_winrate]
    ewn_init_aux / ewn_reset / ewn_roll_dice                          ewn_init_aux[shaped], ewn_reset[mt19937], ewn_reset[philox-masked],
                                                                      ewn_roll_dice[mt19937], ewn_roll_dice[philox-masked]
    mcts_launch                    k_mcts_init, k_mcts_pick           ewn_predict_mcts[lean], ewn_predict_mcts[generic]
                                   k_mcts_rollout_lean                ewn_predict_mcts[lean], ewn_step[split-mcts-lean]
                                   k_mcts_rollout                     ewn_predict_mcts[generic], ewn_step[split-mcts-generic]
    ewn_step                       k_step<1, 0, S> (STEP_TABLES)      ewn_step[tables-one-thread-per-game]: step_plan takes it only under
                                                                      EWN_D3_T=0, latched per process, so the case runs (a) and (b) in a
                                                                      child process with that environment (CHILD_ENV)
                                   k_step<NW, 0, 0> (STEP_GENERIC)    ewn_step[generic-7x7-L4], ewn_step[generic-9x9]
                                   k_step<NW, 1, 0>, k_step<NW, 2, 0> ewn_step[split-mcts-lean], [split-mcts-generic], [split-sim_winrate]
                                   k_mt_refill                        ewn_step[mt19937-autoreset-null-scratch]
    ewn_step_k                     k_rollout_mcts                     ewn_step_k[mcts]
                                   k_rollout_generic                  ewn_step_k[generic-7x7-L4], ewn_step_k[generic-9x9]
    ewn_step_k_agent               k_rollout_mcts_agent<2, 2, 0>      ewn_step_k_agent[mcts-vs-mcts]
                                   k_rollout_mcts_agent<2, 0, 0>      ewn_step_k_agent[mcts-vs-random]
                                   AGL (table instances)              ewn_step_k_agent[minimax-vs-mcts-5x5], [mcts-vs-minimax-7x7]
    ewn_legal_actions / ewn_apply_action / ewn_evaluate               the cases of those names
    ewn_playout_wins               k_zero_wins                        ewn_playout_wins[lean], ewn_playout_wins[generic]
                                   k_playout_wins_lean                ewn_playout_wins[lean]
                                   k_playout_wins                     ewn_playout_wins[generic]
    ewn_predict_minimax            k_predict_minimax_fast<S, true>    ewn_predict_minimax[tables-two_min_dist]
                                   k_predict_minimax_fast<S, false>   ewn_predict_minimax[tables]
    ewn_predict_random             k_predict_random                   ewn_predict_random[step], ewn_predict_random[step_dev]
  ewn_step_d3_tu.inc (2)
    d3_launch_one                  k_step_d3                          ewn_step[lean-tables], [lean-two_min_dist], [lean-random],
                                                                      [lean-tables-d5], [mt19937-autoreset-scratch], [..-null-scratch]
    D3_LAUNCHER                    k_mtq_flip                         ewn_step[mt19937-autoreset-scratch]
  ewn_rollout_tu.inc (4)
    roll_launch                    k_rollout_d3                       ewn_step_k[lockstep-columns], [lockstep-record], [d5],
                                                                      [two_min_dist], [minimax-agent], [mt19937]
    slots_launch                   k_rollout_slots<.., 1> (records)   ewn_step_k[slots-record]
                                   k_rollout_slots<.., 2> (totals)    ewn_step_k[slots-totals]
                                   k_rollout_slots<.., 0>             ewn_step_k[slots-columns]
  ewn_policy.hip (11)
    a2c_reduce_launch              k_a2c_reduce2                      ewn_a2c_grad[5x5], [7x7], ewn_ppo_grad, ewn_sup_grad[5x5]
                                   k_a2c_reduce                       ewn_a2c_grad[5x5-scratch+4], ewn_sup_grad[7x7-scratch+4]
    grad3_launch                   the value pass, the policy pass    ewn_a2c_grad, ewn_ppo_grad, ewn_sup_grad (every case)
    ewn_a2c_apply                  k_a2c_apply<true> / <false>        ewn_a2c_apply[aligned] / ewn_a2c_apply[scalar]
    ewn_ppo_shuffle                k_ppo_shuffle                      ewn_ppo_shuffle[counter]
    ewn_ppo_apply                  k_ppo_apply<true> / <false>        ewn_ppo_apply[aligned] / ewn_ppo_apply[scalar]
    sup_grad_launch                k_sup_rows                         ewn_sup_grad[5x5], ewn_sup_grad[7x7-scratch+4]
    ewn_lookahead_targets          k_lookahead_targets                ewn_lookahead_targets[t0], ewn_lookahead_targets[t0.5]
  ewn_policy_host.hpp (1)
    pol_launch_kernel              every policy, search and tree kernel: ewn_step_k_policy, ewn_step_k_selfplay, ewn_step_vs,
                                   ewn_step_k_vs, ewn_policy_eval, ewn_policy_eval_mcts, ewn_policy_eval_vs, ewn_ppo_prepare,
                                   ewn_predict_policy, ewn_predict_lookahead, ewn_predict_lookahead_eg, ewn_lookahead_expand,
                                   ewn_lookahead_reduce, ewn_puct_begin, ewn_puct_advance, ewn_puct_advance_noise, ewn_puct_result,
                                   ewn_puct_play, ewn_puct_search, ewn_puct_selfplay (the cases of those names, 5x5 and 7x7)
  ewn_endgame.hip (3)
    eg_build                       k_endgame_clear, k_endgame_level   ewn_endgame_build[3x3-2-4] (a clear and one launch per level)
    ewn_endgame_lookup             k_endgame_lookup                   ewn_endgame_lookup[3x3-2-4]
"""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                        # the case table below is plain data and imports without torch (tests/test_stream_contract_cpu.py reads
    import torch            # it); torch and the suite's helpers are needed only where a builder or a property runs, on a GPU
except ImportError:
    torch = None


def _suite(module, name):
    """`name` of another module of the suite, imported when a builder first asks for it (those modules need torch at import)"""
    import importlib
    return getattr(importlib.import_module("tests." + module), name)


def pool(ea, S):
    return _suite("test_gpu_predict_policy", "pool")(ea, S)


def _random_positions(*a, **kw):
    return _suite("test_gpu_parity", "_random_positions")(*a, **kw)


def reset_positions(ea, S, n):
    return _suite("test_gpu_puct_selfplay", "reset_positions")(ea, S, n)


def soft_targets(m, seed):
    return _suite("test_gpu_sup_grad", "soft_targets")(m, seed)

# the `<<<` of every file under ewn_gym_amd/csrc that has one: a new launch site forces an edit here, next to the table above
LAUNCH_SITES = {"ewn_kernels.hip": 28, "ewn_policy.hip": 11, "ewn_rollout_tu.inc": 4, "ewn_step_d3_tu.inc": 2, "ewn_endgame.hip": 3,
                "ewn_policy_host.hpp": 1}
MEMSET_SITES = {}           # hipMemset* calls per file: none (a captured memset node of value 0 is not replayed faithfully)

# entries whose call updates a buffer in place or reads a device counter: three replays against three eager calls
STATEFUL = ("ewn_reset", "ewn_init_aux", "ewn_roll_dice", "ewn_step", "ewn_step_k", "ewn_step_k_agent", "ewn_step_k_policy",
            "ewn_step_k_selfplay", "ewn_step_vs", "ewn_step_k_vs", "ewn_policy_eval", "ewn_policy_eval_mcts", "ewn_policy_eval_vs",
            "ewn_a2c_apply", "ewn_ppo_apply", "ewn_ppo_shuffle", "ewn_predict_random", "ewn_puct_advance", "ewn_puct_advance_noise",
            "ewn_puct_play", "ewn_puct_selfplay")

M = 300          # lanes, positions
DEV = "cuda"


@pytest.fixture(scope="module")
def ea():
    if torch is None or not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


# ---------------------------------------------------------------- a case's buffers and their roles

FILL_OUT, FILL_SCRATCH = 0xA5, 0xFF


def _bytes(t):
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def same_bytes(x, y):
    """x and y (dicts name -> tensor) hold the same bytes; same_bytes.last names the first buffer that differs"""
    assert x.keys() == y.keys()
    for k in x:
        if not torch.equal(_bytes(x[k]), _bytes(y[k])):
            same_bytes.last = "%s (%d of %d bytes)" % (k, int((_bytes(x[k]) != _bytes(y[k])).sum()), _bytes(x[k]).numel())
            return False
    return True


same_bytes.last = None


class Live:
    """One case, built: the argument list of its entry (without the stream) over preallocated device buffers, and what each buffer is.
    inp: an input, with its two valid sets A and B.  io: updated in place -- an input (A, B) whose bytes after the call are compared
    too.  out: written only; filled with 0xA5 before a call.  scr: scratch; filled with 0xFF (or what the test asks for).  const: read
    only and the same in A and B (parameters, table images)."""

    def __init__(self, entry):
        self.entry, self.args, self.fn = entry, None, None
        self.bufs, self.A, self.B = {}, {}, {}
        self.outs, self.scratch, self.inplace, self.keep = [], [], [], []

    def inp(self, name, a, b, buf=None):
        assert name not in self.bufs and a.shape == b.shape and a.dtype == b.dtype
        self.bufs[name] = a.clone() if buf is None else buf
        assert self.bufs[name].shape == a.shape and self.bufs[name].dtype == a.dtype and self.bufs[name].is_contiguous()
        self.A[name], self.B[name] = a.clone(), b.clone()
        self.bufs[name].copy_(a)
        return self.bufs[name]

    def io(self, name, a, b, buf=None):
        self.inplace.append(name)
        return self.inp(name, a, b, buf)

    def out(self, name, shape=None, dtype=None, buf=None):
        assert name not in self.bufs
        self.bufs[name] = torch.zeros(shape, dtype=dtype, device=DEV) if buf is None else buf
        assert self.bufs[name].is_contiguous()
        self.outs.append(name)
        return self.bufs[name]

    def scr(self, name, shape=None, buf=None):
        assert name not in self.bufs
        self.bufs[name] = torch.zeros(shape, dtype=torch.uint8, device=DEV) if buf is None else buf
        self.scratch.append(name)
        return self.bufs[name]

    def const(self, name, t):
        assert name not in self.bufs and t.is_contiguous()
        self.bufs[name] = t
        return t

    def bind(self, lib):
        self.fn = getattr(lib, self.entry)
        assert len(self.args) + 1 == len(self.fn.argtypes), self.entry      # the stream is the last parameter

    def call(self, stream):
        return self.fn(*self.args, C.c_void_p(stream))

    def restore(self, which):
        for k, t in (self.A if which == "A" else self.B).items():
            self.bufs[k].copy_(t)

    def fill(self, out=FILL_OUT, scratch=FILL_SCRATCH):
        for k in self.outs:
            _bytes(self.bufs[k]).fill_(out)
        for k in self.scratch:
            _bytes(self.bufs[k]).fill_(scratch)

    def observe(self):
        return {k: self.bufs[k].clone() for k in self.outs + self.inplace}

    def eager(self, which, n):
        """n calls in a row on the current stream from the input set `which`: what the outputs and the in-place buffers hold after each"""
        self.restore(which)
        seen = []
        for _ in range(n):
            self.fill()
            rc = self.call(torch.cuda.current_stream().cuda_stream)
            assert rc == 0, (self.entry, rc)
            torch.cuda.synchronize()
            seen.append(self.observe())
        return seen


# ---------------------------------------------------------------- what the builders share

def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seeds(n, off):
    return torch.from_numpy((np.arange(n, dtype=np.uint64) * 7 + off).astype(np.uint32).view(np.int32).copy()).to(DEV)


def _actions(n, seed):
    """any [flag, dir] is a valid input of a step: a move that leaves the board is the env's business"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, 2, (n,), generator=g), torch.randint(0, 3, (n,), generator=g)], 1).to(torch.int8).to(DEV)


def _positions(ea, S, L=3, m=M):
    """((boards A, dice A), (boards B, dice B)): real play.  cube_layer 3 on 5x5 / 7x7: disjoint slices of test_gpu_predict_policy's pool"""
    if L == 3 and S in (5, 7):
        p = pool(ea, S)
        return tuple((p["boards"][lo:lo + m].clone(), p["dice"][lo:lo + m].clone()) for lo in (0, 4000))
    b, d = _random_positions(S, L, 2 * m, 40 + S)
    b, d = torch.as_tensor(b).to(torch.int8).to(DEV), torch.as_tensor(d).to(torch.int8).to(DEV)
    return (b[:m].contiguous(), d[:m].contiguous()), (b[m:].contiguous(), d[m:].contiguous())


def _params(ea, S):
    return pool(ea, S)["params"]


def _obs(live, ea, S, L=3, m=M):
    """the two position sets as the inputs `boards` and `dice`"""
    (ba, da), (bb, db) = _positions(ea, S, L, m)
    return live.inp("boards", ba, bb), live.inp("dice", da, db)


STATE = ("board", "dice", "done", "rng_state", "prev_score", "tolerance")


def _env(live, ea, n=M, seeds=(3, 100003), warm=None, **kw):
    """a VecEWN whose state buffers are the case's in-place buffers: A and B are the states after reset(seeds[0]) / reset(seeds[1])
    (and `warm`, which may play a few steps)"""
    kw.setdefault("rng", "philox")
    kw.setdefault("autoreset", True)
    env = ea.VecEWN(n, seed_stride=n, philox_key=77, **kw)
    snaps = []
    for s in seeds:
        env.reset(seeds=_seeds(n, s))
        if warm is not None:
            warm(env)
        torch.cuda.synchronize()
        snaps.append({k: getattr(env, k).clone() for k in STATE if getattr(env, k) is not None})
    for k in snaps[0]:
        live.io(k, snaps[0][k], snaps[1][k], buf=getattr(env, k))
    live.keep.append(env)
    return env


def _rollout_out(live, env, K, layout, totals=True, initial_obs=False):
    """ewn_rollout_out over fresh buffers: layout "columns", "record" (the record and its reward column) or None (no trajectory)"""
    traj = {}
    if layout == "record":
        t = env.alloc_rollout(K, layout="record", initial_obs=initial_obs)
        traj = {"record": t["record"], "reward": t["reward"]}
    elif layout == "columns":
        traj = env.alloc_rollout(K)
    for k, t in traj.items():
        live.out("traj_" + k, buf=t)
    tot = env.alloc_totals() if totals else {}
    for k, t in tot.items():
        live.io("total_" + k, t.clone(), t.clone(), buf=t)       # ADDED to: in place, zero in A and in B
    out = env._rollout_out(traj, tot)
    live.keep.append((traj, tot, out))
    return out


def _records(ea, S, n, K, seed):
    """(record [K + 1][n][stride], reward [K][n]) of a policy rollout on the shaped env, as the trainers collect them"""
    env = ea.VecEWN(n, board_size=S, opponent_policy="minimax", max_depth=2, rng="philox", shaped=True, reward=10.0,
                    illegal_move_tolerance=4, shaped_refresh_on_reset=True, autoreset=True, seed_stride=n, philox_key=31)
    env.reset(seeds=_seeds(n, seed))
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, _params(ea, S), traj=traj, noise_key=seed)
    torch.cuda.synchronize()
    return env, traj["record"].clone(), traj["reward"].clone()


def _a2c_hyper(ea):
    return ea._lib.EwnA2cHyper(0.97, 0.5, 0.01, 0.5, 7e-4, 0.99, 1e-5, 1)


def _ppo_hyper(ea):
    return ea._lib.EwnPpoHyper(0.99, 0.95, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-5, 1, 1)


def _f32(seed, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _off(n, dtype, offset):
    """a buffer of n elements `offset` elements past an allocation's (16-byte aligned) start"""
    return torch.zeros(n + offset, dtype=dtype, device=DEV)[offset:]


# ---------------------------------------------------------------- the builders: each returns a Live

def b_reset(ea, rng, masked):
    L = Live("ewn_reset")
    env = _env(L, ea, rng=rng, opponent_policy="random")
    seeds = L.inp("seeds", _seeds(M, 11), _seeds(M, 500011))
    mask = L.const("mask", (torch.arange(M, device=DEV) % 3 != 1).to(torch.uint8)) if masked else None
    L.args = [C.byref(env.cfg), C.byref(env._st), _ptr(seeds), _ptr(mask)]
    return L


def b_init_aux(ea):
    L = Live("ewn_init_aux")
    env = _env(L, ea, opponent_policy="minimax", max_depth=2, shaped=True, reward=10.0, illegal_move_tolerance=4,
               warm=lambda e: e.step(_actions(M, 1)))
    L.args = [C.byref(env.cfg), C.byref(env._st)]
    return L


def b_roll_dice(ea, rng, masked):
    L = Live("ewn_roll_dice")
    env = _env(L, ea, rng=rng, opponent_policy="random")
    mask = L.const("mask", (torch.arange(M, device=DEV) % 3 != 1).to(torch.uint8)) if masked else None
    L.args = [C.byref(env.cfg), C.byref(env._st), _ptr(mask)]
    return L


def b_step(ea, null_scratch=False, lanes_per_game=None, extras=True, need_env=None, **kw):
    L = Live("ewn_step")
    for k, v in (need_env or {}).items():      # a latched override that selects this case's path: set before the library first read it
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    env = _env(L, ea, want_terminal_obs=extras, want_random_action=extras, **kw)
    if lanes_per_game is not None:          # the kernel family this case is meant to run
        assert env.lib.ewn_lanes_per_game(C.byref(env.cfg), 0) == lanes_per_game
    nscr = int(env.lib.ewn_step_scratch_bytes(C.byref(env.cfg)))
    if nscr > 0 and not null_scratch:       # state by contract: zeroed once, then the library's
        L.io("scratch", torch.zeros_like(env.scratch), torch.zeros_like(env.scratch), buf=env.scratch)
    acts = L.inp("actions", _actions(M, 5), _actions(M, 6))
    for k in ("reward", "terminated", "truncated", "info", "terminal_board", "terminal_dice", "random_action"):
        if getattr(env, k) is not None:
            L.out(k, buf=getattr(env, k))
    L.args = [C.byref(env.cfg), C.byref(env._st), _ptr(acts), C.byref(env._out), None if null_scratch or nscr == 0 else _ptr(env.scratch)]
    return L


def b_step_k(ea, n=M, K=4, agent="random", depth=3, layout="columns", totals=True, lanes_per_game=None, **kw):
    L = Live("ewn_step_k")
    env = _env(L, ea, n=n, **kw)
    assert env.supports_rollout(agent, depth)
    if lanes_per_game is not None:
        assert env.lib.ewn_lanes_per_game(C.byref(env.cfg), 1) == lanes_per_game
    out = _rollout_out(L, env, K, layout, totals)
    L.args = [C.byref(env.cfg), C.byref(env._st), K, ea._lib.AGENT[agent], depth, C.byref(out)]
    return L


def b_step_k_agent(ea, S, agent, **kw):
    L = Live("ewn_step_k_agent")
    env = _env(L, ea, board_size=S, num_simulations=2, num_env_copies=2, **kw)
    assert env.supports_agent_rollout(agent)
    a = env._agent_struct(agent, step_base=3, key=9)
    out = _rollout_out(L, env, 3, "columns")
    L.keep.append(a)
    L.args = [C.byref(env.cfg), C.byref(env._st), 3, C.byref(a), C.byref(out)]
    return L


def _policy_struct(L, ea, env, S, K, value=True):
    P = ea._lib.EwnPolicy
    lg = L.out("logits", (K, M, 5), torch.float32)
    v = L.out("value", (K, M), torch.float32) if value else None
    nz = L.out("noise", (K, M, 5), torch.float32)
    pol = P(_ptr(L.const("params", _params(ea, S))), 0, 1, 99, _ptr(lg), _ptr(v), _ptr(nz))
    L.keep.append(pol)
    return pol


def _opponent_struct(L, ea, S, rows, deterministic=0):
    act = L.out("opponent_action", rows + (M, 3), torch.int8)
    opp = ea._lib.EwnOpponentPolicy(_ptr(L.const("opponent_params", pool(ea, S)["params"].flip(0).contiguous())), deterministic, 5, _ptr(act))
    L.keep.append(opp)
    return opp


def b_step_k_policy(ea, S):
    L = Live("ewn_step_k_policy")
    env = _env(L, ea, board_size=S, opponent_policy="minimax", max_depth=3, shaped=True, reward=10.0, illegal_move_tolerance=4,
               shaped_refresh_on_reset=True)
    assert env.supports_policy_rollout()
    pol = _policy_struct(L, ea, env, S, 4)
    out = _rollout_out(L, env, 4, "record", initial_obs=True)
    L.args = [C.byref(env.cfg), C.byref(env._st), 4, C.byref(pol), C.byref(out)]
    return L


def b_step_k_selfplay(ea, S):
    L = Live("ewn_step_k_selfplay")
    env = _env(L, ea, board_size=S, opponent_policy="random")
    assert env.supports_selfplay_rollout(value=S == 5)
    pol = _policy_struct(L, ea, env, S, 4, value=S == 5)        # 7x7 with the value output is not served (three weight images)
    opp = _opponent_struct(L, ea, S, (4,))
    out = _rollout_out(L, env, 4, "record", initial_obs=True)
    L.args = [C.byref(env.cfg), C.byref(env._st), 4, C.byref(pol), C.byref(opp), C.byref(out)]
    return L


def b_step_vs(ea, S):
    L = Live("ewn_step_vs")
    env = _env(L, ea, board_size=S, opponent_policy="random", shaped=True, reward=10.0, illegal_move_tolerance=4, want_terminal_obs=True)
    assert env.supports_step_vs()
    opp = _opponent_struct(L, ea, S, (), deterministic=1)
    acts = L.inp("actions", _actions(M, 5), _actions(M, 6))
    for k in ("reward", "terminated", "truncated", "info", "terminal_board", "terminal_dice"):
        L.out(k, buf=getattr(env, k))
    L.args = [C.byref(env.cfg), C.byref(env._st), _ptr(acts), C.byref(opp), C.byref(env._out)]
    return L


def b_step_k_vs(ea, S, agent, depth):
    L = Live("ewn_step_k_vs")
    env = _env(L, ea, board_size=S, opponent_policy="random")
    assert env.tables is not None and env.lib.ewn_step_k_vs_supported(C.byref(env.cfg), ea._lib.AGENT[agent], depth) == 1
    opp = _opponent_struct(L, ea, S, (4,))
    out = _rollout_out(L, env, 4, "columns")
    L.args = [C.byref(env.cfg), C.byref(env._st), 4, ea._lib.AGENT[agent], depth, C.byref(opp), C.byref(out)]
    return L


def b_policy_eval(ea, S, kind, **kw):
    L = Live({"plain": "ewn_policy_eval", "mcts": "ewn_policy_eval_mcts", "vs": "ewn_policy_eval_vs"}[kind])
    env = _env(L, ea, board_size=S, autoreset=False, num_simulations=2, num_env_copies=2, **kw)
    assert {"plain": env.supports_policy_eval, "mcts": env.supports_policy_eval_mcts, "vs": env.supports_policy_eval_vs}[kind]()
    act = L.out("action", (4, M, 2), torch.int8)
    tot = env.alloc_totals()
    for k, t in tot.items():
        L.io("total_" + k, t.clone(), t.clone(), buf=t)
    out = env._rollout_out({"action": act}, tot)
    L.keep.append((tot, out))
    params = _ptr(L.const("params", _params(ea, S)))
    opp = [C.byref(_opponent_struct(L, ea, S, (4,), deterministic=1))] if kind == "vs" else []
    L.args = [C.byref(env.cfg), C.byref(env._st), 4, params] + opp + [C.byref(out)]
    return L


def b_a2c_grad(ea, S, offset):
    L = Live("ewn_a2c_grad")
    K = 3
    env, ra, wa = _records(ea, S, M, K, 11)
    _, rb, wb = _records(ea, S, M, K, 12)
    rec, rew = L.inp("record", ra, rb), L.inp("reward", wa, wb)
    params = L.const("params", _params(ea, S))
    grad = L.out("grad", (params.numel() + 8,), torch.float32)
    nscr = int(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), K))
    scratch = L.scr("scratch", buf=_off(nscr, torch.uint8, offset))
    # `partial` = scratch + 4 K N bytes: 8-byte aligned it takes k_a2c_reduce2, else k_a2c_reduce (test_gpu_a2c_fused.py)
    assert (scratch.data_ptr() + 4 * K * M) % 8 == offset % 8
    hp = _a2c_hyper(ea)
    L.keep += [env, hp]
    L.args = [C.byref(env.cfg), K, _ptr(rec), _ptr(rew), _ptr(params), C.byref(hp), _ptr(grad), _ptr(scratch)]
    return L


def b_a2c_apply(ea, S, offset):
    L = Live("ewn_a2c_apply")
    env = ea.VecEWN(64, board_size=S, opponent_policy="random", rng="philox")
    P = env.policy_param_count()
    params = L.io("params", _params(ea, S).clone(), _f32(1, P), buf=_off(P, torch.float32, offset))
    sq = L.io("sq_avg", _f32(2, P).abs(), _f32(3, P).abs(), buf=_off(P, torch.float32, offset))
    grad = L.inp("grad", _f32(4, P + 8), _f32(5, P + 8), buf=_off(P + 8, torch.float32, offset))
    norm = L.out("grad_norm", (1,), torch.float32)
    assert (params.data_ptr() % 16 == 0) == (offset == 0)
    hp = _a2c_hyper(ea)
    L.keep += [env, hp]
    L.args = [C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm)]
    return L


def _ppo_samples(ea, env, K, rec, rew, S):
    samples = torch.zeros((K * M, 4), dtype=torch.float32, device=DEV)
    hp = _ppo_hyper(ea)
    assert env.lib.ewn_ppo_prepare(C.byref(env.cfg), K, _ptr(rec), _ptr(rew), _ptr(_params(ea, S)), C.byref(hp), _ptr(samples),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return samples


def b_ppo_prepare(ea, S):
    L = Live("ewn_ppo_prepare")
    K = 3
    env, ra, wa = _records(ea, S, M, K, 11)
    _, rb, wb = _records(ea, S, M, K, 12)
    rec, rew = L.inp("record", ra, rb), L.inp("reward", wa, wb)
    samples = L.out("samples", (K * M, 4), torch.float32)
    hp = _ppo_hyper(ea)
    L.keep += [env, hp]
    L.args = [C.byref(env.cfg), K, _ptr(rec), _ptr(rew), _ptr(L.const("params", _params(ea, S))), C.byref(hp), _ptr(samples)]
    return L


def b_ppo_shuffle(ea):
    L = Live("ewn_ppo_shuffle")
    n = 3 * M
    ctr = L.inp("counter", torch.tensor([3], dtype=torch.int32, device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV))
    perm = L.out("perm", (2, n), torch.int32)
    L.args = [C.c_int64(n), 2, C.c_uint64(7), _ptr(ctr), _ptr(perm)]
    return L


def b_ppo_grad(ea, S):
    L = Live("ewn_ppo_grad")
    K, B = 3, 128
    env, ra, wa = _records(ea, S, M, K, 11)
    _, rb, wb = _records(ea, S, M, K, 12)
    rec = L.inp("record", ra, rb)
    samples = L.inp("samples", _ppo_samples(ea, env, K, ra, wa, S), _ppo_samples(ea, env, K, rb, wb, S))
    g = torch.Generator().manual_seed(S)
    idx = L.inp("idx", *[torch.randperm(K * M, generator=g)[:B].to(torch.int32).to(DEV) for _ in range(2)])
    params = L.const("params", _params(ea, S))
    grad = L.out("grad", (params.numel() + 8,), torch.float32)
    scratch = L.scr("scratch", (int(env.lib.ewn_ppo_scratch_bytes(C.byref(env.cfg), K, B)),))
    hp = _ppo_hyper(ea)
    L.keep += [env, hp]
    L.args = [C.byref(env.cfg), K, _ptr(rec), _ptr(samples), _ptr(params), C.byref(hp), _ptr(idx), B, _ptr(grad), _ptr(scratch)]
    return L


def b_ppo_apply(ea, S, offset):
    L = Live("ewn_ppo_apply")
    env = ea.VecEWN(64, board_size=S, opponent_policy="random", rng="philox")
    P = env.policy_param_count()
    params = L.io("params", _params(ea, S).clone(), _f32(1, P), buf=_off(P, torch.float32, offset))
    m = L.io("exp_avg", _f32(2, P, scale=0.1), _f32(3, P, scale=0.1), buf=_off(P, torch.float32, offset))
    v = L.io("exp_avg_sq", _f32(4, P).abs(), _f32(5, P).abs(), buf=_off(P, torch.float32, offset))
    step = L.io("step", torch.tensor([2], dtype=torch.int32, device=DEV), torch.tensor([7], dtype=torch.int32, device=DEV))
    grad = L.inp("grad", _f32(6, P + 8), _f32(7, P + 8), buf=_off(P + 8, torch.float32, offset))
    norm = L.out("grad_norm", (1,), torch.float32)
    assert (params.data_ptr() % 16 == 0) == (offset == 0)
    hp = _ppo_hyper(ea)
    L.keep += [env, hp]
    L.args = [C.byref(env.cfg), _ptr(params), _ptr(m), _ptr(v), _ptr(step), _ptr(grad), C.byref(hp), _ptr(norm)]
    return L


def b_sup_grad(ea, S, offset):
    L = Live("ewn_sup_grad")
    b, d = _obs(L, ea, S)
    ta, tb = soft_targets(M, 1), soft_targets(M, 2)
    pi, tv, w = L.inp("target_pi", ta[0], tb[0]), L.inp("target_value", ta[1], tb[1]), L.inp("weight", ta[2], tb[2])
    params = L.const("params", _params(ea, S))
    grad = L.out("grad", (params.numel() + 8,), torch.float32)
    lib = ea._lib.load()
    scratch = L.scr("scratch", buf=_off(int(lib.ewn_sup_scratch_bytes(S, 3, M)), torch.uint8, offset))
    assert scratch.data_ptr() % 8 == offset % 8         # 8-byte aligned: the faster reduce kernel serves
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(pi), _ptr(tv), _ptr(w), _ptr(params), C.c_float(1.0), C.c_float(0.5), _ptr(grad), _ptr(scratch)]
    return L


def b_lookahead_targets(ea, temperature):
    L = Live("ewn_lookahead_targets")
    (ba, da), (bb, db) = _positions(ea, 5)
    qa, qb = [ea.predict_lookahead(b, d, _params(ea, 5), return_q=True)[1].reshape(M, 6).contiguous() for b, d in ((ba, da), (bb, db))]
    q = L.inp("q", qa, qb)
    pi, tv, w = L.out("target_pi", (M, 5), torch.float32), L.out("target_value", (M,), torch.float32), L.out("weight", (M,), torch.float32)
    L.args = [M, _ptr(q), C.c_float(temperature), _ptr(pi), _ptr(tv), _ptr(w)]
    return L


def b_legal_actions(ea, S, L3, player):
    L = Live("ewn_legal_actions")
    b, d = _obs(L, ea, S, L3)
    outs = [L.out("acts", (M, 6, 2), torch.int8)] + [L.out(k, (M,), torch.int8) for k in ("n_acts", "cube_small", "cube_large")]
    win = L.out("win", (M,), torch.uint8)
    L.args = [S, L3, M, _ptr(b), _ptr(d), player] + [_ptr(t) for t in outs] + [_ptr(win)]
    return L


def b_apply_action(ea, S, L3):
    L = Live("ewn_apply_action")
    b, d = _obs(L, ea, S, L3)
    a = L.inp("actions", _actions(M, 1), _actions(M, 2))
    nb, valid = L.out("new_boards", (M, S, S), torch.int8), L.out("valid", (M,), torch.uint8)
    L.args = [S, L3, M, _ptr(b), _ptr(d), 1, _ptr(a), _ptr(nb), _ptr(valid)]
    return L


def b_evaluate(ea, S, L3, heur):
    L = Live("ewn_evaluate")
    b, _ = _obs(L, ea, S, L3)
    out = L.out("out", (M,), torch.float64)
    L.args = [S, L3, M, _ptr(b), ea._lib.HEUR[heur], _ptr(out)]
    return L


def b_playout_wins(ea, S, L3):
    L = Live("ewn_playout_wins")
    b, _ = _obs(L, ea, S, L3)
    wins = L.out("wins", (M,), torch.int32)
    L.args = [S, L3, M, _ptr(b), 1, 8, C.c_uint64(5), _ptr(wins)]
    return L


def b_predict_minimax(ea, S, depth, heur, tables):
    L = Live("ewn_predict_minimax")
    b, d = _obs(L, ea, S)
    acts, vals = L.out("actions", (M, 2), torch.int8), L.out("values", (M,), torch.float64)
    from ewn_gym_amd.vec_env import search_tables
    t = L.const("tables", search_tables(S, 3, torch.device(DEV))) if tables else None
    L.args = [S, 3, M, _ptr(b), _ptr(d), depth, ea._lib.HEUR[heur], _ptr(acts), _ptr(vals), _ptr(t)]
    return L


def b_predict_minimax_sim(ea):
    L = Live("ewn_predict_minimax_sim")
    b, d = _obs(L, ea, 5)
    ids = L.inp("obs_id", torch.arange(M, dtype=torch.int32, device=DEV) + 5, torch.arange(M, dtype=torch.int32, device=DEV) + 900)
    acts, vals = L.out("actions", (M, 2), torch.int8), L.out("values", (M,), torch.float64)
    L.args = [5, 3, M, _ptr(b), _ptr(d), 1, C.c_uint64(3), _ptr(ids), _ptr(acts), _ptr(vals)]
    return L


def b_predict_random(ea, step_dev):
    L = Live("ewn_predict_random")
    b, d = _obs(L, ea, 5)
    sd = L.inp("step_dev", torch.tensor([4], dtype=torch.int32, device=DEV), torch.tensor([9], dtype=torch.int32, device=DEV)) if step_dev else None
    acts = L.out("actions", (M, 2), torch.int8)
    L.args = [5, 3, M, _ptr(b), _ptr(d), C.c_uint64(3), C.c_uint32(2), _ptr(sd), 40, _ptr(acts)]
    return L


def b_predict_mcts(ea, S, L3):
    L = Live("ewn_predict_mcts")
    b, d = _obs(L, ea, S, L3)
    acts, wins = L.out("actions", (M, 2), torch.int8), L.out("wins", (M, 6), torch.int32)    # wins: written by k_mcts_init first
    L.args = [S, L3, M, _ptr(b), _ptr(d), 2, 3, C.c_uint64(3), None, _ptr(acts), _ptr(wins)]
    return L


def b_predict_policy(ea, S, deterministic):
    L = Live("ewn_predict_policy")
    b, d = _obs(L, ea, S)
    u = None if deterministic else L.inp("uniforms", _f32(1, M, 5).sigmoid(), _f32(2, M, 5).sigmoid())
    acts, lg, v = L.out("actions", (M, 2), torch.int8), L.out("logits", (M, 5), torch.float32), L.out("value", (M,), torch.float32)
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(L.const("params", _params(ea, S))), deterministic, C.c_uint64(3), None, _ptr(u),
              _ptr(acts), _ptr(lg), _ptr(v)]
    return L


def b_predict_lookahead(ea, S):
    L = Live("ewn_predict_lookahead")
    b, d = _obs(L, ea, S)
    acts, q = L.out("actions", (M, 2), torch.int8), L.out("q", (M, 6), torch.float32)
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(L.const("params", _params(ea, S))), C.c_float(1.0), _ptr(acts), _ptr(q)]
    return L


def _few_cubes(S, K, T, seed, m=M):
    """m positions of the (S, K, T) endgame table and their dice: test_gpu_endgame's sampling"""
    import random
    rng = random.Random(seed)
    board_of, sample = _suite("test_gpu_endgame", "board_of"), _suite("test_gpu_endgame", "sample")
    b = torch.as_tensor(np.stack([board_of(sample(rng, S, K, T), S) for _ in range(m)])).to(DEV)
    d = torch.tensor([rng.randint(1, 6) for _ in range(m)], dtype=torch.int8, device=DEV)
    return b, d


def b_predict_lookahead_eg(ea, S):
    L = Live("ewn_predict_lookahead_eg")
    (ba, da), (bb, db) = _positions(ea, S)
    for (b, d), seed in (((ba, da), 1), ((bb, db), 2)):      # every third row three plies from the table: its leaves are exact
        fb, fd = _few_cubes(S, 2, 4, seed, m=M // 3)
        b[::3], d[::3] = fb, fd
    b, d = L.inp("boards", ba, bb), L.inp("dice", da, db)
    t = L.const("table", ea.EndgameTable.build(S, 1, 2).table)
    acts, q, cnt = L.out("actions", (M, 2), torch.int8), L.out("q", (M, 6), torch.float32), L.out("leaf_counts", (M, 2), torch.int16)
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(L.const("params", _params(ea, S))), C.c_float(1.0), 1, 2, _ptr(t), _ptr(acts), _ptr(q), _ptr(cnt)]
    return L


def b_lookahead_expand(ea, S):
    L = Live("ewn_lookahead_expand")
    b, d = _obs(L, ea, S)
    lb, ld, kind = L.out("leaf_boards", (648 * M, S, S), torch.int8), L.out("leaf_dice", (648 * M,), torch.int8), L.out("kind", (M, 108), torch.int8)
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(lb), _ptr(ld), _ptr(kind)]
    return L


def b_lookahead_reduce(ea, S, width):
    L = Live("ewn_lookahead_reduce")
    (ba, da), (bb, db) = _positions(ea, S)
    b, d = L.inp("boards", ba, bb), L.inp("dice", da, db)
    kind = L.inp("kind", ea.lookahead_expand(ba, da)[2], ea.lookahead_expand(bb, db)[2])
    leaf = L.inp("leaf", _f32(1, 648 * M, width).tanh(), _f32(2, 648 * M, width).tanh())
    acts, q = L.out("actions", (M, 2), torch.int8), L.out("q", (M, 6), torch.float32)
    L.args = [S, 3, M, _ptr(b), _ptr(d), _ptr(kind), _ptr(leaf), width, C.c_float(1.0), _ptr(acts), _ptr(q)]
    return L


SIMS = 8


def b_puct_begin(ea, S):
    L = Live("ewn_puct_begin")
    b, d = _obs(L, ea, S)
    nb = int(ea._lib.load().ewn_puct_tree_bytes(S, 3, SIMS))
    tree, lb, ld = L.out("tree", (M, nb), torch.uint8), L.out("leaf_boards", (M, S, S), torch.int8), L.out("leaf_dice", (M,), torch.int8)
    L.args = [S, 3, M, SIMS, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld)]
    return L


def _rounds(ea, S, b, d, rounds):
    """the tree after puct_begin and `rounds` rounds, with the network's answer to its pending leaves"""
    params = _params(ea, S)
    tree, lb, ld = ea.puct_begin(b, d, SIMS)
    for _ in range(rounds):
        _, lg, v = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
        ea.puct_advance(tree, lg, v, lb, ld, SIMS)
    _, lg, v = ea.predict_policy(lb, ld, params, return_logits=True, return_value=True)
    torch.cuda.synchronize()
    return tree, lg, v


def b_puct_advance(ea, S, noise, rounds):
    L = Live("ewn_puct_advance_noise" if noise else "ewn_puct_advance")
    (ba, da), (bb, db) = _positions(ea, S)
    (ta, la, va), (tb, lb_, vb) = _rounds(ea, S, ba, da, rounds), _rounds(ea, S, bb, db, rounds)
    tree, lg, v = L.io("tree", ta, tb), L.inp("logits", la, lb_), L.inp("value", va, vb)
    rn = [_ptr(L.inp("root_noise", ea.selfplay_noise(M, 1.0, 3, 0, 0), ea.selfplay_noise(M, 1.0, 4, 0, 0))), C.c_float(0.25)] if noise else []
    lb, ld = L.out("leaf_boards", (M, S, S), torch.int8), L.out("leaf_dice", (M,), torch.int8)
    L.args = [S, 3, M, SIMS, C.c_float(1.5), C.c_float(1.0), _ptr(tree), _ptr(lg), _ptr(v)] + rn + [_ptr(lb), _ptr(ld)]
    return L


def _searched(ea, S):
    return [ea.puct_search(b, d, _params(ea, S), SIMS) for b, d in _positions(ea, S)]


def b_puct_result(ea, S):
    L = Live("ewn_puct_result")
    tree = L.inp("tree", *_searched(ea, S))
    outs = [L.out("actions", (M, 2), torch.int8), L.out("visits", (M, 6), torch.int32), L.out("q", (M, 6), torch.float32),
            L.out("value", (M,), torch.float32)]
    L.args = [S, 3, M, _ptr(tree)] + [_ptr(t) for t in outs]
    return L


def _play_rows(L, S, lead):
    """the six rec_* arguments of ewn_puct_play / ewn_puct_selfplay over fresh outputs of `lead` + the row's shape"""
    shapes = _suite("test_gpu_puct_selfplay", "row_shapes")(S)
    return [_ptr(L.out("rec_" + k, lead + shapes[k][0], shapes[k][1])) for k in _suite("test_gpu_puct_selfplay", "ROWS")]


def b_puct_play(ea, S):
    L = Live("ewn_puct_play")
    (ba, da), (bb, db) = _positions(ea, S)
    tree = L.inp("tree", *_searched(ea, S))
    b, d = L.io("boards", ba, bb), L.io("dice", da, db)
    game = L.io("game", torch.zeros((M, 4), dtype=torch.int32, device=DEV), torch.zeros((M, 4), dtype=torch.int32, device=DEV))
    L.args = [S, 3, M, _ptr(tree), _ptr(b), _ptr(d), _ptr(game), 8, C.c_uint64(11), C.c_int64(2 ** 32 + 5)] + _play_rows(L, S, (M,))
    return L


def b_puct_search(ea, S, noise):
    L = Live("ewn_puct_search")
    b, d = _obs(L, ea, S)
    rn = L.inp("root_noise", ea.selfplay_noise(M, 1.0, 3, 0, 0), ea.selfplay_noise(M, 1.0, 4, 0, 0)) if noise else None
    tree = L.out("tree", (M, int(ea._lib.load().ewn_puct_tree_bytes(S, 3, SIMS))), torch.uint8)
    L.args = [S, 3, M, SIMS, -1, C.c_float(1.5), C.c_float(1.0), _ptr(b), _ptr(d), _ptr(L.const("params", _params(ea, S))), _ptr(rn),
              C.c_float(0.25), _ptr(tree)]
    return L


def b_puct_selfplay(ea, S):
    """33 games on 2 blocks of 4 columns: every column is refilled; cut at 6 plies"""
    L = Live("ewn_puct_selfplay")
    n, T, tile, blocks = 33, 6, 4, 2
    lib = ea._lib.load()
    ba, da = reset_positions(ea, S, n)
    p = pool(ea, S)
    bb, db = p["boards"][8000:8000 + n].clone(), p["dice"][8000:8000 + n].clone()
    b, d = L.io("boards", ba, bb), L.io("dice", da, db)
    game = L.io("game", torch.zeros((n, 4), dtype=torch.int32, device=DEV), torch.zeros((n, 4), dtype=torch.int32, device=DEV))
    noise = L.inp("noise", *[torch.stack([ea.selfplay_noise(n, 1.0, key, 5, t) for t in range(T)]) for key in (11, 12)])
    nscr = int(lib.ewn_puct_selfplay_scratch_bytes(S, 3, n, SIMS, tile, blocks))
    assert nscr == lib.ewn_puct_tree_bytes(S, 3, SIMS) * blocks * tile
    scratch = L.scr("scratch", (nscr,))
    rows = _play_rows(L, S, (T, n))
    L.args = [S, 3, n, SIMS, T, C.c_float(1.5), C.c_float(1.0), _ptr(L.const("params", _params(ea, S))), _ptr(noise), C.c_float(0.25), 4,
              C.c_uint64(11), C.c_int64(5), tile, blocks, _ptr(b), _ptr(d), _ptr(game)] + rows + [_ptr(scratch)]
    return L


EG = (3, 2, 4)       # the smallest table test_gpu_endgame.py builds


def b_endgame_build(ea):
    L = Live("ewn_endgame_build")
    n = int(ea._lib.load().ewn_endgame_table_bytes(*EG))
    table = L.out("table", (n // 4,), torch.float32)
    L.args = [EG[0], EG[1], EG[2], _ptr(table), C.c_int64(n)]
    return L


def b_endgame_lookup(ea):
    L = Live("ewn_endgame_lookup")
    S = EG[0]
    (ba, da), (bb, db) = _few_cubes(*EG, seed=1), _few_cubes(*EG, seed=2)
    b, d = L.inp("boards", ba, bb), L.inp("dice", da, db)
    t = L.const("table", ea.EndgameTable.build(*EG).table)
    outs = [L.out("actions", (M, 2), torch.int8), L.out("q", (M, 6), torch.float32), L.out("value", (M,), torch.float32),
            L.out("covered", (M,), torch.uint8)]
    L.args = [S, EG[1], EG[2], _ptr(t), M, _ptr(b), _ptr(d)] + [_ptr(x) for x in outs]
    return L


# ---------------------------------------------------------------- the table

def _c(entry, config, build, *a, **kw):
    return (entry, config, lambda ea: build(ea, *a, **kw))


MM3 = dict(opponent_policy="minimax", max_depth=3)
MCTS = dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2)

CASES = [
    _c("ewn_reset", "mt19937", b_reset, "mt19937", False),
    _c("ewn_reset", "philox-masked", b_reset, "philox", True),
    _c("ewn_init_aux", "shaped", b_init_aux),
    _c("ewn_roll_dice", "mt19937", b_roll_dice, "mt19937", False),
    _c("ewn_roll_dice", "philox-masked", b_roll_dice, "philox", True),
    # ewn_step: one case per path of step_plan (ewn_host.hpp) and per refill form
    _c("ewn_step", "lean-tables", b_step, lanes_per_game=2, **MM3),
    _c("ewn_step", "lean-two_min_dist", b_step, lanes_per_game=2, heuristic="two_min_dist", **MM3),
    _c("ewn_step", "lean-tables-d5", b_step, lanes_per_game=2, opponent_policy="minimax", max_depth=5),
    _c("ewn_step", "lean-tables-7x7-shaped", b_step, lanes_per_game=2, board_size=7, shaped=True, reward=10.0, illegal_move_tolerance=4, **MM3),
    _c("ewn_step", "lean-random", b_step, lanes_per_game=1, opponent_policy="random"),
    # STEP_TABLES: step_plan takes it only with the lean kernel switched off (EWN_D3_T=0, latched): this case runs in a child process
    _c("ewn_step", "tables-one-thread-per-game", b_step, lanes_per_game=0, need_env={"EWN_D3_T": "0"}, **MM3),
    _c("ewn_step", "generic-7x7-L4", b_step, lanes_per_game=0, board_size=7, cube_layer=4, opponent_policy="minimax", max_depth=2, heuristic="attk"),
    _c("ewn_step", "generic-9x9", b_step, lanes_per_game=0, board_size=9, opponent_policy="random"),
    _c("ewn_step", "split-mcts-lean", b_step, **MCTS),
    _c("ewn_step", "split-mcts-generic", b_step, board_size=7, cube_layer=4, **MCTS),
    _c("ewn_step", "split-sim_winrate", b_step, opponent_policy="minimax", max_depth=1, heuristic="sim_winrate"),
    _c("ewn_step", "mt19937-autoreset-scratch", b_step, rng="mt19937", **MM3),
    _c("ewn_step", "mt19937-autoreset-null-scratch", b_step, null_scratch=True, rng="mt19937", **MM3),
    # ewn_step_k: one case per K-step plan (rollout_plan, generic_rollout_plan, mcts_rollout_plan; ewn_rollout_tu.inc)
    _c("ewn_step_k", "lockstep-columns", b_step_k, lanes_per_game=2, **MM3),
    _c("ewn_step_k", "lockstep-record", b_step_k, layout="record", lanes_per_game=2, **MM3),
    _c("ewn_step_k", "slots-record", b_step_k, n=65537, layout="record", totals=False, lanes_per_game=2, **MM3),
    _c("ewn_step_k", "slots-totals", b_step_k, n=65537, layout=None, lanes_per_game=2, **MM3),
    _c("ewn_step_k", "slots-columns", b_step_k, n=65537, layout="columns", lanes_per_game=2, **MM3),
    _c("ewn_step_k", "d5", b_step_k, K=3, lanes_per_game=2, opponent_policy="minimax", max_depth=5),
    _c("ewn_step_k", "two_min_dist", b_step_k, heuristic="two_min_dist", **MM3),
    _c("ewn_step_k", "minimax-agent", b_step_k, agent="minimax", depth=4, opponent_policy="random"),   # two table images: above 64 KB of LDS
    _c("ewn_step_k", "mt19937", b_step_k, rng="mt19937", autoreset=False, **MM3),
    _c("ewn_step_k", "generic-7x7-L4", b_step_k, lanes_per_game=0, board_size=7, cube_layer=4, opponent_policy="minimax", max_depth=2, heuristic="attk"),
    _c("ewn_step_k", "generic-9x9", b_step_k, lanes_per_game=0, layout="record", board_size=9, opponent_policy="random"),
    _c("ewn_step_k", "mcts", b_step_k, **MCTS),
    _c("ewn_step_k_agent", "mcts-vs-mcts", b_step_k_agent, 5, {"kind": "mcts", "num_simulations": 2, "num_env_copies": 2}, opponent_policy="mcts"),
    _c("ewn_step_k_agent", "mcts-vs-random", b_step_k_agent, 5, {"kind": "mcts", "num_simulations": 2, "num_env_copies": 2}, opponent_policy="random"),
    _c("ewn_step_k_agent", "minimax-vs-mcts-5x5", b_step_k_agent, 5, {"kind": "minimax", "max_depth": 2}, opponent_policy="mcts"),
    _c("ewn_step_k_agent", "mcts-vs-minimax-7x7", b_step_k_agent, 7, {"kind": "mcts", "num_simulations": 2, "num_env_copies": 2}, opponent_policy="minimax", max_depth=2),
    _c("ewn_step_k_policy", "5x5", b_step_k_policy, 5),
    _c("ewn_step_k_policy", "7x7", b_step_k_policy, 7),
    _c("ewn_step_k_selfplay", "5x5", b_step_k_selfplay, 5),
    _c("ewn_step_k_selfplay", "7x7", b_step_k_selfplay, 7),
    _c("ewn_step_vs", "5x5", b_step_vs, 5),
    _c("ewn_step_vs", "7x7", b_step_vs, 7),
    _c("ewn_step_k_vs", "5x5-random", b_step_k_vs, 5, "random", 3),
    _c("ewn_step_k_vs", "7x7-minimax", b_step_k_vs, 7, "minimax", 2),
    _c("ewn_policy_eval", "5x5", b_policy_eval, 5, "plain", **MM3),
    _c("ewn_policy_eval", "7x7-mt19937", b_policy_eval, 7, "plain", rng="mt19937", opponent_policy="random"),
    _c("ewn_policy_eval_mcts", "5x5", b_policy_eval, 5, "mcts", opponent_policy="mcts"),
    _c("ewn_policy_eval_mcts", "7x7", b_policy_eval, 7, "mcts", opponent_policy="mcts"),
    _c("ewn_policy_eval_vs", "5x5", b_policy_eval, 5, "vs", opponent_policy="random"),
    _c("ewn_policy_eval_vs", "7x7", b_policy_eval, 7, "vs", opponent_policy="random"),
    # the trainers' kernels
    _c("ewn_a2c_grad", "5x5", b_a2c_grad, 5, 0),
    _c("ewn_a2c_grad", "5x5-scratch+4", b_a2c_grad, 5, 4),
    _c("ewn_a2c_grad", "7x7", b_a2c_grad, 7, 0),
    _c("ewn_a2c_apply", "aligned", b_a2c_apply, 5, 0),
    _c("ewn_a2c_apply", "scalar", b_a2c_apply, 7, 1),
    _c("ewn_ppo_prepare", "5x5", b_ppo_prepare, 5),
    _c("ewn_ppo_prepare", "7x7", b_ppo_prepare, 7),
    _c("ewn_ppo_shuffle", "counter", b_ppo_shuffle),
    _c("ewn_ppo_grad", "5x5", b_ppo_grad, 5),
    _c("ewn_ppo_grad", "7x7", b_ppo_grad, 7),
    _c("ewn_ppo_apply", "aligned", b_ppo_apply, 7, 0),
    _c("ewn_ppo_apply", "scalar", b_ppo_apply, 5, 1),
    _c("ewn_sup_grad", "5x5", b_sup_grad, 5, 0),
    _c("ewn_sup_grad", "7x7-scratch+4", b_sup_grad, 7, 4),
    _c("ewn_lookahead_targets", "t0", b_lookahead_targets, 0.0),
    _c("ewn_lookahead_targets", "t0.5", b_lookahead_targets, 0.5),
    # the stateless queries
    _c("ewn_legal_actions", "5x5-player1", b_legal_actions, 5, 3, 1),
    _c("ewn_legal_actions", "7x7-L4-player2", b_legal_actions, 7, 4, 2),
    _c("ewn_apply_action", "5x5", b_apply_action, 5, 3),
    _c("ewn_apply_action", "7x7-L4", b_apply_action, 7, 4),
    _c("ewn_evaluate", "5x5-hybrid", b_evaluate, 5, 3, "hybrid"),
    _c("ewn_evaluate", "7x7-L4-attk", b_evaluate, 7, 4, "attk"),
    _c("ewn_playout_wins", "lean", b_playout_wins, 5, 3),
    _c("ewn_playout_wins", "generic", b_playout_wins, 7, 4),
    _c("ewn_predict_minimax", "tables", b_predict_minimax, 5, 3, "hybrid", True),
    _c("ewn_predict_minimax", "tables-two_min_dist", b_predict_minimax, 7, 3, "two_min_dist", True),
    _c("ewn_predict_minimax", "no-tables", b_predict_minimax, 5, 2, "hybrid", False),
    _c("ewn_predict_minimax_sim", "d1", b_predict_minimax_sim),
    _c("ewn_predict_random", "step", b_predict_random, False),
    _c("ewn_predict_random", "step_dev", b_predict_random, True),
    _c("ewn_predict_mcts", "lean", b_predict_mcts, 5, 3),
    _c("ewn_predict_mcts", "generic", b_predict_mcts, 7, 4),
    # the network: policy, lookahead, PUCT, endgame tables
    _c("ewn_predict_policy", "5x5-argmax", b_predict_policy, 5, 1),
    _c("ewn_predict_policy", "7x7-sampled", b_predict_policy, 7, 0),
    _c("ewn_predict_lookahead", "5x5", b_predict_lookahead, 5),
    _c("ewn_predict_lookahead", "7x7", b_predict_lookahead, 7),
    _c("ewn_predict_lookahead_eg", "5x5", b_predict_lookahead_eg, 5),
    _c("ewn_lookahead_expand", "5x5", b_lookahead_expand, 5),
    _c("ewn_lookahead_expand", "7x7", b_lookahead_expand, 7),
    _c("ewn_lookahead_reduce", "5x5-values", b_lookahead_reduce, 5, 1),
    _c("ewn_lookahead_reduce", "7x7-q-rows", b_lookahead_reduce, 7, 6),
    _c("ewn_puct_begin", "5x5", b_puct_begin, 5),
    _c("ewn_puct_begin", "7x7", b_puct_begin, 7),
    _c("ewn_puct_advance", "5x5-round3", b_puct_advance, 5, False, 3),
    _c("ewn_puct_advance", "7x7-round0", b_puct_advance, 7, False, 0),
    _c("ewn_puct_advance_noise", "5x5-round0", b_puct_advance, 5, True, 0),
    _c("ewn_puct_advance_noise", "7x7-round0", b_puct_advance, 7, True, 0),
    _c("ewn_puct_result", "5x5", b_puct_result, 5),
    _c("ewn_puct_result", "7x7", b_puct_result, 7),
    _c("ewn_puct_play", "5x5", b_puct_play, 5),
    _c("ewn_puct_play", "7x7", b_puct_play, 7),
    _c("ewn_puct_search", "5x5", b_puct_search, 5, False),
    _c("ewn_puct_search", "5x5-noise", b_puct_search, 5, True),
    _c("ewn_puct_search", "7x7-noise", b_puct_search, 7, True),
    _c("ewn_puct_selfplay", "5x5", b_puct_selfplay, 5),
    _c("ewn_puct_selfplay", "7x7", b_puct_selfplay, 7),
    _c("ewn_endgame_build", "3x3-2-4", b_endgame_build),
    _c("ewn_endgame_lookup", "3x3-2-4", b_endgame_lookup),
]
IDS = ["%s[%s]" % (e, c) for e, c, _ in CASES]
assert len(set(IDS)) == len(IDS)
# the cases whose path a latched override selects, with the environment of the fresh process they run in (one child each, both
# properties in it); every other case runs in the pytest process, whose environment sets none of the overrides (test_cabi_cpu.py)
CHILD_ENV = {"ewn_step[tables-one-thread-per-game]": {"EWN_D3_T": "0"}}
IN_PROCESS = [cid for cid in IDS if cid not in CHILD_ENV]
assert set(CHILD_ENV) <= set(IDS)

# property (c): every entry that calls hipFuncSetAttribute (ewn_step's lean kernel, ewn_step_k's two-image instances, ewn_step_k_agent's
# table instances, the gradient kernels, every policy kernel) and every entry behind a latched getenv (EWN_D3_T: ewn_step;
# EWN_ROLLOUT_T and EWN_ROLLOUT_SLOTS: ewn_step_k; EWN_MCTS_GPB: ewn_step_k[mcts]; EWN_EVAL_NT: ewn_policy_eval*, ewn_step_vs), and
# EWN_PUCT_TILE's reader
THREAD_SEQUENCE = ["ewn_step[lean-tables]", "ewn_step[lean-tables-7x7-shaped]", "ewn_step[mt19937-autoreset-scratch]", "ewn_step[split-mcts-lean]",
                   "ewn_step_k[lockstep-columns]", "ewn_step_k[minimax-agent]", "ewn_step_k[mcts]", "ewn_step_k_agent[mcts-vs-minimax-7x7]",
                   "ewn_step_k_policy[7x7]", "ewn_step_k_selfplay[5x5]", "ewn_step_vs[7x7]", "ewn_step_k_vs[5x5-random]",
                   "ewn_policy_eval[5x5]", "ewn_policy_eval_mcts[7x7]", "ewn_policy_eval_vs[5x5]", "ewn_a2c_grad[5x5]", "ewn_ppo_prepare[7x7]",
                   "ewn_ppo_grad[5x5]", "ewn_sup_grad[7x7-scratch+4]", "ewn_predict_policy[7x7-sampled]", "ewn_predict_lookahead[5x5]",
                   "ewn_puct_search[7x7-noise]", "ewn_puct_selfplay[5x5]", "ewn_playout_wins[lean]", "ewn_endgame_build[3x3-2-4]"]
assert set(THREAD_SEQUENCE) <= set(IN_PROCESS)


# ---------------------------------------------------------------- the properties

_LIVE = {}


def live(ea, cid):
    """the case's buffers and its eager bytes, built once per module: E_A (three calls in a row from A for a stateful entry) and E_B"""
    if cid not in _LIVE:
        entry, _, build = CASES[IDS.index(cid)]
        L = build(ea)
        assert L.entry == entry
        L.bind(ea._lib.load())
        torch.cuda.synchronize()
        n = 3 if entry in STATEFUL else 1
        L.EA = L.eager("A", n)
        again = L.eager("A", 1)
        L.EB = L.eager("B", 1)[0]
        # the precondition: two eager calls on the same inputs agree byte for byte
        assert same_bytes(again[0], L.EA[0]), "%s: two eager calls on the same inputs differ in %s" % (cid, same_bytes.last)
        if L.A:
            assert not same_bytes(L.EA[0], L.EB), "%s: E_A == E_B, the case cannot tell a late launch from a correct one" % cid
        _LIVE[cid] = L
    return _LIVE[cid]


def measure_sleep():
    """torch.cuda._sleep's argument for about 20 ms, from one timed sleep; the sleep of that length measured again: at least 5 ms"""
    def timed(c):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        torch.cuda._sleep(c)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)
    timed(1000)                                  # the kernel's first launch is not timed
    probe = 1_000_000
    ms = timed(probe)
    assert ms > 0
    c = max(probe // 100, int(probe * 20.0 / ms))
    got = timed(c)
    print("torch.cuda._sleep: %d cycles took %.3f ms; %d cycles took %.3f ms" % (probe, ms, c, got))
    assert got >= 5.0, (c, got)
    return c


@pytest.fixture(scope="module")
def sleep_cycles(ea):
    return measure_sleep()


def check_capture(ea, cid):
    """property (a)"""
    L = live(ea, cid)
    L.restore("A")
    L.fill()
    torch.cuda.synchronize()
    before = L.observe()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        rc = L.call(torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert same_bytes(L.observe(), before), "%s: the captured call ran (or wrote) during the capture: %s" % (cid, same_bytes.last)
    g.replay()
    torch.cuda.synchronize()
    assert same_bytes(L.observe(), L.EA[0]), "%s: first replay differs from the eager call in %s" % (cid, same_bytes.last)
    for k in range(1, len(L.EA)):               # a stateful entry: the second and third replay against the second and third eager call
        L.fill()
        g.replay()
        torch.cuda.synchronize()
        assert same_bytes(L.observe(), L.EA[k]), "%s: replay %d differs from eager call %d in %s" % (cid, k + 1, k + 1, same_bytes.last)
    if not L.A:                                  # no device input: again into refilled outputs, a device-to-device copy in between
        for k in (2, 3):
            L.fill(scratch=0x5A)
            before[L.outs[0]].copy_(L.bufs[L.outs[0]])
            g.replay()
            torch.cuda.synchronize()
            assert same_bytes(L.observe(), L.EA[0]), "%s: replay %d differs from the eager call in %s" % (cid, k, same_bytes.last)
    else:                                        # the graph holds pointers, not values; no scratch or counter carries over
        for which, want in (("B", L.EB), ("A", L.EA[0])):
            L.restore(which)
            L.fill(scratch=0x5A)
            g.replay()
            torch.cuda.synchronize()
            assert same_bytes(L.observe(), want), "%s: replay on %s differs from the eager call in %s" % (cid, which, same_bytes.last)


def check_side_stream(ea, cid, sleep_cycles):
    """property (b)"""
    L = live(ea, cid)
    L.restore("A")
    L.fill(out=0x3C)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(sleep_cycles)
        L.restore("B")
        L.fill()
        rc = L.call(s.cuda_stream)
        got = L.observe()
    s.synchronize()
    assert rc == 0, rc
    assert same_bytes(got, L.EB), "%s: the call did not wait for the work queued on its stream before it: %s" % (cid, same_bytes.last)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cid", IN_PROCESS)
def test_captured_nothing_runs_replayed_the_eager_bytes(ea, cid):
    check_capture(ea, cid)


@pytest.mark.parametrize("cid", IN_PROCESS)
def test_a_side_stream_is_honoured(ea, cid, sleep_cycles):
    check_side_stream(ea, cid, sleep_cycles)


def child_main(cid):
    """what a child process of test_latched_paths_in_a_fresh_process runs: properties (a) and (b) of one case"""
    import ewn_gym_amd
    check_capture(ewn_gym_amd, cid)
    check_side_stream(ewn_gym_amd, cid, measure_sleep())
    print("child ok: %s" % cid)


@pytest.mark.parametrize("cid", sorted(CHILD_ENV))
def test_latched_paths_in_a_fresh_process(ea, cid):
    """A path that only a latched override selects cannot be reached in this process, whose library has read its environment: the case
    runs in a child whose environment sets the override, properties (a) and (b), under a time limit of its own."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), **CHILD_ENV[cid])
    r = subprocess.run([sys.executable, "-c", "import sys; from tests import test_gpu_stream_contract as m; m.child_main(sys.argv[1])", cid],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert ("child ok: %s" % cid) in r.stdout


def test_two_threads_two_streams_disjoint_buffers(ea):
    lib = ea._lib.load()
    want = [live(ea, cid).EA[0] for cid in THREAD_SEQUENCE]
    sets = []
    for _ in range(2):                           # each thread its own buffers
        built = []
        for cid in THREAD_SEQUENCE:
            L = CASES[IDS.index(cid)][2](ea)
            L.bind(lib)
            L.restore("A")
            L.fill()
            built.append(L)
        sets.append(built)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    results, errors = [None, None], [None, None]
    go = threading.Barrier(2)

    def work(t):
        try:
            order = list(range(len(THREAD_SEQUENCE)))
            if t == 1:
                order.reverse()
            got = {}
            go.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for i in order:
                    rc = sets[t][i].call(streams[t].cuda_stream)
                    assert rc == 0, (THREAD_SEQUENCE[i], rc)
                    got[i] = sets[t][i].observe()
            streams[t].synchronize()
            results[t] = got
        except BaseException as exc:             # reported by the main thread
            errors[t] = exc

    threads = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    t0 = time.time()
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    print("two threads x %d calls: %.2f s" % (len(THREAD_SEQUENCE), time.time() - t0))
    assert errors == [None, None], errors
    for t in (0, 1):
        for i, cid in enumerate(THREAD_SEQUENCE):
            assert same_bytes(results[t][i], want[i]), "thread %d, %s: differs from the single-thread bytes in %s" % (t, cid, same_bytes.last)
