"""The host side of the seven policy entry points without a GPU: the code each gives for a malformed call, and which check answers
when a call has two faults at once.  Every case carries at least one fault, so nothing is launched; every pointer is a small host
address no kernel may ever see.

One table: per entry point the faults it refuses, in the order its checks run, each with its code.  A call with several faults gets
the code of the first of them in that order (faults that share one `if` share a code, so their order inside it does not show)."""
import ctypes as C
import itertools

import pytest

torch = pytest.importorskip("torch")

from ewn_gym_amd import _lib  # noqa: E402
from ewn_gym_amd._lib import (AGENT, OPP, RNG, EwnConfig, EwnOpponentPolicy, EwnPolicy, EwnRolloutOut, EwnState,  # noqa: E402
                              EwnStepOut)

EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
TOTALS = ("return_sum", "n_steps", "n_episodes", "n_wins")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def well_formed(opponent="random", tables=8, out="rollout"):
    """the arguments of a call that would be served, as plain values the faults below edit"""
    ctx = {
        "cfg": dict(board_size=5, cube_layer=3, n_lanes=64, opponent_kind=OPP[opponent], max_depth=3, heuristic=0, num_simulations=10,
                    num_env_copies=5, rng_kind=RNG["philox"], shaped=0, illegal_move_tolerance=10, autoreset=0, seed_stride=64,
                    reward=1.0, illegal_move_reward=-1.0),
        "st": dict(board=8, dice=8, done=8, rng=8, prev_score=None, tolerance=None, tables=tables),
        "K": 4,
        "params": 8,                                   # ewn_policy.params, or the evaluation calls' `params`
        "opp": dict(params=8, deterministic=1),
        "actions": 8,
        "agent": (AGENT["random"], 0),
    }
    if out == "rollout":
        ctx["out"] = {}                                # every column of ewn_rollout_out is optional
    elif out == "totals":
        ctx["out"] = {f: 8 for f in TOTALS + ("action",)}
    else:
        ctx["out"] = dict(reward=8, terminated=8, truncated=8, info=8)
    return ctx


# fault -> edits (argument, member or None for the argument itself, value)
FAULTS = {
    "cfg null": [("cfg", None, None)],
    "n_lanes 0": [("cfg", "n_lanes", 0)],
    "K 0": [("K", None, 0)],
    "state null": [("st", None, None)],
    "tables missing": [("st", "tables", None)],
    "shaped without prev_score / tolerance": [("cfg", "shaped", 1)],          # the state's prev_score / tolerance stay NULL
    "params missing": [("params", None, None)],
    "opponent null": [("opp", None, None)],
    "opponent empty": [("opp", None, {})],
    "actions null": [("actions", None, None)],
    "out null": [("out", None, None)],
    "totals missing": [("out", "n_episodes", None)],
    "step column missing": [("out", "truncated", None)],
    "trajectory column in an evaluation": [("out", "reward", 8)],
    "random_action asked": [("out", "random_action", 8)],
    "minimax agent of depth 0": [("agent", None, (AGENT["minimax"], 0))],
    "board size 6": [("cfg", "board_size", 6)],
    "MT19937 dice": [("cfg", "rng_kind", RNG["mt19937"])],
    "MT19937 dice with auto-reset": [("cfg", "rng_kind", RNG["mt19937"]), ("cfg", "autoreset", 1)],
}


def apply_faults(ctx, case):
    for f in case:
        for key, member, value in FAULTS[f]:
            if member is None:
                ctx[key] = value
            elif ctx[key] is not None:                 # else: a member of a struct that another fault of the case took away
                ctx[key][member] = value


def _ref(cls, fields):
    return None if fields is None else C.byref(cls(**fields))


def _common(ctx):
    return _ref(EwnConfig, ctx["cfg"]), _ref(EwnState, ctx["st"])


def _policy(ctx):
    return C.byref(EwnPolicy(params=ctx["params"]))    # a present struct: `params missing` is its NULL member


def call_step_k_policy(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_step_k_policy(cfg, st, ctx["K"], _policy(ctx), _ref(EwnRolloutOut, ctx["out"]), None)


def call_step_k_selfplay(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_step_k_selfplay(cfg, st, ctx["K"], _policy(ctx), _ref(EwnOpponentPolicy, ctx["opp"]), _ref(EwnRolloutOut, ctx["out"]), None)


def call_policy_eval(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_policy_eval(cfg, st, ctx["K"], ctx["params"], _ref(EwnRolloutOut, ctx["out"]), None)


def call_policy_eval_vs(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_policy_eval_vs(cfg, st, ctx["K"], ctx["params"], _ref(EwnOpponentPolicy, ctx["opp"]), _ref(EwnRolloutOut, ctx["out"]), None)


def call_policy_eval_mcts(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_policy_eval_mcts(cfg, st, ctx["K"], ctx["params"], _ref(EwnRolloutOut, ctx["out"]), None)


def call_step_vs(lib, ctx):
    cfg, st = _common(ctx)
    return lib.ewn_step_vs(cfg, st, ctx["actions"], _ref(EwnOpponentPolicy, ctx["opp"]), _ref(EwnStepOut, ctx["out"]), None)


def call_step_k_vs(lib, ctx):
    cfg, st = _common(ctx)
    kind, depth = ctx["agent"]
    return lib.ewn_step_k_vs(cfg, st, ctx["K"], kind, depth, _ref(EwnOpponentPolicy, ctx["opp"]), _ref(EwnRolloutOut, ctx["out"]), None)


# entry point -> (the call, its well-formed arguments, [(fault, code)] in the order of the entry point's checks)
ENTRY_POINTS = {
    "ewn_step_k_policy": (call_step_k_policy, dict(opponent="minimax"), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("params missing", ENULL),
        ("shaped without prev_score / tolerance", ENULL),
        ("board size 6", EUNSUPPORTED), ("MT19937 dice", EUNSUPPORTED)]),
    "ewn_step_k_selfplay": (call_step_k_selfplay, dict(), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("params missing", ENULL), ("opponent null", ENULL), ("opponent empty", ENULL),
        ("shaped without prev_score / tolerance", ENULL),
        ("board size 6", EUNSUPPORTED), ("MT19937 dice", EUNSUPPORTED)]),
    "ewn_policy_eval": (call_policy_eval, dict(opponent="minimax", out="totals"), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("params missing", ENULL), ("out null", ENULL),
        ("totals missing", ENULL), ("trajectory column in an evaluation", EINVAL),
        ("board size 6", EUNSUPPORTED), ("shaped without prev_score / tolerance", EUNSUPPORTED)]),    # no shaped evaluation at all
    "ewn_policy_eval_vs": (call_policy_eval_vs, dict(out="totals"), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("params missing", ENULL), ("opponent null", ENULL), ("opponent empty", ENULL),
        ("out null", ENULL),
        ("totals missing", ENULL), ("trajectory column in an evaluation", EINVAL),
        ("board size 6", EUNSUPPORTED), ("shaped without prev_score / tolerance", EUNSUPPORTED)]),
    # this one reads no table image: its well-formed call has tables NULL, so every case below shows that it is not asked for
    "ewn_policy_eval_mcts": (call_policy_eval_mcts, dict(opponent="mcts", tables=None, out="totals"), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL),
        ("state null", ENULL), ("params missing", ENULL), ("out null", ENULL),
        ("totals missing", ENULL), ("trajectory column in an evaluation", EINVAL),
        ("board size 6", EUNSUPPORTED), ("shaped without prev_score / tolerance", EUNSUPPORTED)]),
    "ewn_step_vs": (call_step_vs, dict(out="step"), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("actions null", ENULL), ("opponent null", ENULL), ("opponent empty", ENULL),
        ("out null", ENULL),
        ("step column missing", ENULL), ("shaped without prev_score / tolerance", ENULL), ("random_action asked", EINVAL),
        ("board size 6", EUNSUPPORTED), ("MT19937 dice with auto-reset", EUNSUPPORTED)]),
    "ewn_step_k_vs": (call_step_k_vs, dict(), [
        ("cfg null", ENULL), ("n_lanes 0", EINVAL), ("K 0", EINVAL), ("minimax agent of depth 0", EINVAL),
        ("state null", ENULL), ("tables missing", ENULL), ("opponent null", ENULL), ("opponent empty", ENULL),
        ("shaped without prev_score / tolerance", ENULL),
        ("board size 6", EUNSUPPORTED), ("MT19937 dice with auto-reset", EUNSUPPORTED)]),
}


def test_the_table_covers_every_fault():
    assert set(ENTRY_POINTS) == {"ewn_step_k_policy", "ewn_step_k_selfplay", "ewn_policy_eval", "ewn_policy_eval_vs", "ewn_policy_eval_mcts",
                                 "ewn_step_vs", "ewn_step_k_vs"}
    assert {f for _, _, order in ENTRY_POINTS.values() for f, _ in order} == set(FAULTS)


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_refusals_and_their_order(lib, entry):
    call, base, order = ENTRY_POINTS[entry]
    names = [f for f, _ in order]
    cases = [(f,) for f in names] + list(itertools.combinations(names, 2))
    for case in cases:
        ctx = well_formed(**base)
        apply_faults(ctx, case)
        want = next(code for f, code in order if f in case)
        assert call(lib, ctx) == want, (entry, case)
