"""Batched agent-vs-opponent evaluation: the counterpart of the reference's
eval_{random,minimax,mcts}.py loops (eval_minimax.py:16-50) and of eval_pairs.py:10-35.

Every evaluation episode is one lane: episode k is `reset(seed=k)` exactly as upstream
(`for seed in range(num): env.reset(seed=seed)`), all lanes are stepped together until
each has terminated, the agent's `predict` is the same batched policy kernel the env
uses for opponents, and the score of an episode is its final reward (win <=> > 0).
With the MT19937-compat dice stream and a deterministic agent (minimax) the per-episode
results are bit-identical to the reference's; for random / MCTS agents they agree
statistically (different host RNG interleaving upstream).

The confidence interval is a Wilson interval on the win COUNT; the reference passes the
win *rate* as the count to proportion_confint (eval_minimax.py:102).
"""
import argparse
import json
import math

import torch

from .vec_env import VecEWN, predict_mcts, predict_minimax, predict_random


def wilson(wins, n, z=1.959963984540054):
    if n == 0:
        return (0.0, 1.0)
    p = wins / n
    den = 1 + z * z / n
    c = (p + z * z / (2 * n)) / den
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / den
    return (max(0.0, c - h), min(1.0, c + h))


def _model_size(spec):
    return getattr(spec["model"], "S", spec.get("board_size", 5))


def _torch_policy(model):
    """the model's argmax in torch (model.act), the per-step policy of a bare "mlp" agent"""
    return lambda b, d, t: model.act(b, d, deterministic=True)[0]


def _policy(spec, cube_layer, key):
    if callable(spec):          # e.g. A2CTrainer.policy_fn(): (board, dice, t) -> int8 [N, 2]
        return spec
    kind = spec["kind"]
    if kind == "random":
        return lambda b, d, t: predict_random(b, d, key=key, step=t, cube_layer=cube_layer)
    if kind == "minimax":
        return lambda b, d, t: predict_minimax(b, d, spec.get("max_depth", 3), spec.get("heuristic", "hybrid"),
                                               cube_layer=cube_layer)[0]
    if kind == "mcts":
        return lambda b, d, t: predict_mcts(b, d, spec.get("num_simulations", 10), spec.get("num_env_copies", 5),
                                            key=(key + 0x9E3779B97F4A7C15 * (t + 1)) & 0xFFFFFFFFFFFFFFFF,
                                            cube_layer=cube_layer)[0]
    if kind == "playout_search":   # the PUCT tree with uniform priors and random playouts at the leaves (predict_playout_search),
        # ply by ply through ewn_step; keyed like the mcts kind: episode m is observation id m, step t its own key
        from .playout_search import KEY_PLY, _numbers, predict_playout_search
        _numbers("playout_search", spec.get("sims", 64), spec.get("playouts", 64), spec.get("c_puct", 1.5), key, 0)   # refused here, not at the first ply
        if spec.get("endgame_table") is not None:   # a table or its path (loaded once): exact values at the leaves it covers
            from .endgame import EndgameTable, _accept_table
            from .playout_exact import predict_playout_search_exact
            table = _accept_table("playout_search", spec["endgame_table"], None, None, load=EndgameTable.load)
            return lambda b, d, t: predict_playout_search_exact(b, d, table, sims=spec.get("sims", 64), playouts=spec.get("playouts", 64),
                                                                c_puct=spec.get("c_puct", 1.5), key=(key + KEY_PLY * (t + 1)) & 0xFFFFFFFFFFFFFFFF,
                                                                cube_layer=cube_layer)
        return lambda b, d, t: predict_playout_search(b, d, sims=spec.get("sims", 64), playouts=spec.get("playouts", 64),
                                                      c_puct=spec.get("c_puct", 1.5), key=(key + KEY_PLY * (t + 1)) & 0xFFFFFFFFFFFFFFFF,
                                                      cube_layer=cube_layer)
    if kind == "mlp":           # the model's policy through ewn_predict_policy; evaluate() itself plays this kind on its own paths
        from classical_policies.model import ModelAgent
        return ModelAgent(spec["model"], board_size=_model_size(spec), cube_layer=cube_layer,
                          deterministic=spec.get("deterministic", True), key=key).policy_fn()
    if kind == "mlp_lookahead":   # the model's lookahead on its own value net (ewn_predict_lookahead; "plies": 2 the two-move one), ply by ply through ewn_step
        from classical_policies.model import ValueSearchAgent
        return ValueSearchAgent(spec["model"], board_size=_model_size(spec), cube_layer=cube_layer,
                                terminal_value=spec.get("terminal_value", 1.0), plies=spec.get("plies", 1),
                                endgame_table=spec.get("endgame_table")).policy_fn()   # a table or its path: exact leaves
    if kind == "mlp_puct":      # the model's PUCT search on both of its heads (predict_puct), ply by ply through ewn_step
        from classical_policies.model import PuctAgent
        return PuctAgent(spec["model"], board_size=_model_size(spec), cube_layer=cube_layer, sims=spec.get("sims", 64),
                         c_puct=spec.get("c_puct", 1.5), terminal_value=spec.get("terminal_value", 1.0),
                         endgame_table=spec.get("endgame_table"), fused=spec.get("fused", False),   # fused: one launch (4r)
                         leaves=spec.get("leaves", 1),                                              # leaves > 1: the wide launch (4u)
                         leaf_table=spec.get("leaf_table")).policy_fn()                             # exact leaves in one launch (4w)
    if kind == "endgame":       # the exact move where the endgame table covers the position, the "fallback" spec's policy elsewhere
        from classical_policies.model import EndgameAgent
        if "table" not in spec or "fallback" not in spec:
            raise ValueError("the endgame kind takes {'kind': 'endgame', 'table': an EndgameTable or its path, 'fallback': an agent spec}")
        return EndgameAgent(spec["table"], _SpecPolicy(spec["fallback"], cube_layer, key)).policy_fn()
    raise ValueError("unknown agent kind %r" % kind)


class _SpecPolicy:
    """an agent spec behind predict_batch, for EndgameAgent's fallback; step t of the evaluation reaches the spec's policy through
    EndgameAgent.policy_fn's single call per step"""

    def __init__(self, spec, cube_layer, key):
        if isinstance(spec, dict) and spec.get("kind") == "mlp":   # evaluate() plays a bare "mlp" agent itself; inside a wrapper it is the per-step policy
            self.fn = _torch_policy(spec["model"])
        else:
            self.fn = _policy(spec, cube_layer, key)
        self.t = 0

    def predict_batch(self, boards, dice):
        a = self.fn(boards, dice, self.t)
        self.t += 1
        return a


def flat_policy_params(model):
    """The actor-critic's parameters as ONE fp32 device vector in parameters() order (the layout ewn_policy_eval reads): a copy, the
    module is left as it is."""
    return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in model.parameters()]).contiguous()


def _model_on_board(who, model, board_size):
    """raise unless the model plays board_size; who: how the message starts ("evaluate: the model")"""
    if getattr(model, "S", board_size) != board_size:
        raise ValueError("%s plays %dx%d boards, the evaluation is on %dx%d" % (who, model.S, model.S, board_size, board_size))


def _totals_result(totals, num, engine):
    score, length = totals["return_sum"], totals["n_steps"]   # un-shaped env: the only non-zero reward of an episode is its last
    wins = int((score > 0).sum().item())
    lo, hi = wilson(wins, num)
    return {"scores": score, "lengths": length, "wins": wins, "episodes": num, "win_rate": wins / num, "engine": engine,
            "ci95": [lo, hi], "avg_score": float(score.mean().item()), "avg_length": float(length.float().mean().item())}


# ---------------------------------------------------------------- the evaluation env and the two loops every evaluation ends in

def _eval_env(opponent, num, board_size, cube_layer, rng, seed_offset, key, before_reset=None):
    """The evaluation env, reset to the seeds seed_offset .. seed_offset + num - 1.  opponent: a classical spec, or None for the env the
    model-opponent paths build (opponent_policy="random"; the model is not the env's to know).  before_reset(env): what has to come
    between the two, a refusal or set_opponent_model."""
    own = {"opponent_policy": "random"} if opponent is None else {
        "opponent_policy": opponent["kind"], "max_depth": opponent.get("max_depth", 3), "heuristic": opponent.get("heuristic", "hybrid"),
        "num_simulations": opponent.get("num_simulations", 10), "num_env_copies": opponent.get("num_env_copies", 5)}
    env = VecEWN(num, board_size=board_size, cube_layer=cube_layer, rng=rng, autoreset=False, philox_key=key ^ 0x5DEECE66D, **own)
    if before_reset is not None:
        before_reset(env)
    env.reset(seeds=torch.arange(seed_offset, seed_offset + num, dtype=torch.int64).to(torch.int32))
    return env


def _play_chunks(env, launch, max_steps, chunk, num, engine):
    """The engine's loop: launch(t0, totals) enqueues `chunk` steps of every lane from step t0 on and adds to the totals; one host read
    per chunk stops it once every lane is done."""
    totals = env.alloc_totals()
    for t0 in range(0, max_steps, chunk):
        launch(t0, totals)
        if bool((env.done != 0).all()):
            break
    env.check_rng()
    return _totals_result(totals, num, engine)


def _play_plies(env, policy, max_steps, num, engine):
    """The per-step loop: one policy evaluation and one step() per ply, one host read per ply."""
    score = torch.zeros(num, dtype=torch.float64, device=env.device)
    length = torch.zeros(num, dtype=torch.int32, device=env.device)
    for t in range(max_steps):
        alive = env.done == 0
        if not bool(alive.any()):
            break
        _, _, reward, terminated, _, _ = env.step(policy(env.board, env.dice, t))
        just = alive & (terminated != 0)
        score = torch.where(just, reward, score)
        length += alive.to(torch.int32)
    env.check_rng()
    return _totals_result({"return_sum": score, "n_steps": length}, num, engine)


def _rollout_launch(env, agent, chunk):
    """env.rollout (ewn_step_k; with a model set ewn_step_k_vs) as _play_chunks' launch where it serves the agent -- RandomAgent or
    'hybrid' minimax -- else None"""
    if not (isinstance(agent, dict) and agent["kind"] in ("random", "minimax") and agent.get("heuristic", "hybrid") == "hybrid"
            and env.supports_rollout(agent["kind"], agent.get("max_depth", 3))):
        return None
    return lambda t0, totals: env.rollout(chunk, agent=agent["kind"], agent_max_depth=agent.get("max_depth", 3), totals=totals)


def evaluate(agent, opponent, num=1024, board_size=5, cube_layer=3, rng="mt19937", seed_offset=0, key=12345, max_steps=400,
             use_rollout=True, chunk=16):
    """agent: a dict like the opponent's, {"kind": "mlp", "model": a2c.ActorCritic} (its deterministic policy),
    {"kind": "mlp_lookahead", "model": ..., terminal_value=, plies=} (its lookahead on its own value net, ply by ply),
    {"kind": "mlp_puct", "model": ..., sims=, c_puct=, terminal_value=, leaf_table=} (its PUCT search on both of its heads, ply by ply),
    {"kind": "endgame", "table": an EndgameTable or its path, "fallback": any of these dicts} (the exact move where the table covers
    the position, the fallback's elsewhere, ply by ply),
    {"kind": "playout_search", sims=, playouts=, c_puct=, endgame_table=} (the same tree without a network: uniform priors, random playouts at the
    leaves, ply by ply), or a callable policy (board, dice, t) -> actions.
    agent / opponent: dicts {"kind": "random"|"minimax"|"mcts", max_depth=, heuristic=, num_simulations=, num_env_copies=}.
    Returns per-episode scores (float64 tensor), episode lengths and summary statistics.
    When both sides are engine policies the table-driven kernels cover (RandomAgent, 'hybrid' minimax; cube_layer 3) the whole
    predict/step loop runs on the device, `chunk` steps per launch (ewn_step_k); an MCTS agent, or a minimax agent against MCTS, likewise
    through ewn_step_k_agent (cube_layer 3, boards 5..8); an "mlp" agent wherever ewn_policy_eval (RandomAgent, minimax) or
    ewn_policy_eval_mcts (the MCTS opponent) serves the opponent and geometry;
    an "mlp" agent against an "mlp" opponent ({"kind": "mlp", "model": ...}: the opponent model's argmax on its canonical view)
    through ewn_policy_eval_vs, the only model opponent evaluate() itself plays (every other agent kind against a model:
    evaluate_vs_model below);
    otherwise one policy evaluation + one ewn_step per step (use_rollout=False forces that loop).  The engines give the per-step loop's
    per-episode results, the MCTS agent's included: its playouts at step t use key + 0x9E3779B97F4A7C15 * (t + 1) either way
    ("engine" in the result says which one ran)."""
    if opponent["kind"] == "mlp":
        return _evaluate_vs_model(agent, opponent, num, board_size, cube_layer, rng, seed_offset, key, max_steps, chunk)
    env = _eval_env(opponent, num, board_size, cube_layer, rng, seed_offset, key)
    launch = _rollout_launch(env, agent, chunk) if use_rollout else None
    if launch is not None:
        return _play_chunks(env, launch, max_steps, chunk, num, "ewn_step_k")
    if use_rollout and isinstance(agent, dict) and agent["kind"] in ("minimax", "mcts") and env.supports_agent_rollout(agent):
        # the MCTS agent, or the minimax agent against MCTS: ewn_step_k_agent, whose MCTS agent draws the playouts the per-step loop's
        # predict_mcts draws at the same step t (step_base + k)
        return _play_chunks(env, lambda t0, totals: env.agent_rollout(chunk, agent, step_base=t0, key=key, totals=totals),
                            max_steps, chunk, num, "ewn_step_k_agent")
    if isinstance(agent, dict) and agent["kind"] == "mlp":
        model = agent["model"]
        _model_on_board("evaluate: the model", model, board_size)
        params = flat_policy_params(model).to(env.device)
        # the engine's call for this opponent (the MCTS opponent's playout stream is keyed by the lane's RNG header, so the chunking
        # changes nothing there either), or None: the per-step loop below
        engine = ("ewn_policy_eval" if env.supports_policy_eval() else
                  "ewn_policy_eval_mcts" if env.supports_policy_eval_mcts() else None)
        if use_rollout and engine is not None and params.numel() == env.policy_param_count():
            return _play_chunks(env, lambda t0, totals: env.eval_policy(chunk, params, totals), max_steps, chunk, num, engine)
        policy = _torch_policy(model)      # not _policy's ModelAgent (ewn_predict_policy)
    else:
        policy = _policy(agent, cube_layer, key)
    return _play_plies(env, policy, max_steps, num, "ewn_step")


def _evaluate_vs_model(agent, opponent, num, board_size, cube_layer, rng, seed_offset, key, max_steps, chunk):
    """model against model: ewn_policy_eval_vs, both sides deterministic.  There is no per-step path for a model opponent (ewn_step has
    none), so anything the engine does not serve raises."""
    if not (isinstance(agent, dict) and agent.get("kind") == "mlp"):
        raise ValueError("evaluate: a model opponent ({'kind': 'mlp'}) is played by a model agent only (ewn_policy_eval_vs); every other "
                         "agent kind meets it in evaluate_vs_model (ewn_step_k_vs / ewn_step_vs)")
    for side in (agent, opponent):
        _model_on_board("evaluate: a model", side["model"], board_size)

    def served(env):
        if not env.supports_policy_eval_vs():
            raise ValueError("evaluate: ewn_policy_eval_vs does not serve %dx%d boards with cube_layer %d" % (board_size, board_size, cube_layer))
    env = _eval_env(None, num, board_size, cube_layer, rng, seed_offset, key, before_reset=served)
    params, opp = flat_policy_params(agent["model"]).to(env.device), flat_policy_params(opponent["model"]).to(env.device)
    return _play_chunks(env, lambda t0, totals: env.eval_policy(chunk, params, totals, opponent_params=opp),
                        max_steps, chunk, num, "ewn_policy_eval_vs")


def _stand_in_random(env):
    """RandomAgent on the hash stream ewn_step_k / ewn_step_k_vs draw the agent's action from (ewn_step_out.random_action's: one word
    per (episode seed, draws so far, global lane, philox_key), read off the lane's RNG header), as a per-step policy: the ply-by-ply
    loop then plays what the K-step launch plays.  Plumbing around ewn_legal_actions; the hash is a dozen integer ops per lane."""
    from .vec_env import legal_actions
    M = 0xFFFFFFFF

    def fmix(h):            # on a tensor of lanes and on a Python int alike
        h = h ^ (h >> 16)
        h = (h * 0x85EBCA6B) & M
        h = h ^ (h >> 13)
        h = (h * 0xC2B2AE35) & M
        return h ^ (h >> 16)

    key = int(env.cfg.philox_key)
    kterm = fmix((key & M) ^ 0x41474E54) ^ (((key >> 32) * 0x85EBCA6B) & M)
    lane = torch.arange(env.N, dtype=torch.int64, device=env.device) + int(env.cfg.lane_offset)
    philox = int(env.cfg.rng_kind) == 1

    def policy(board, dice, t):
        hdr = env.rng_state.view(-1)[:4 * env.N].view(env.N, 4).to(torch.int64) & M   # the headers lead the buffer (ewn_state.rng)
        seed = hdr[:, 0] ^ ((hdr[:, 3] * 0x9E3779B9) & M) if philox else hdr[:, 0]
        w = fmix(seed ^ fmix((hdr[:, 1] * 0x9E3779B1 + lane) & M) ^ kterm)
        acts, n = legal_actions(board, dice, player=1, cube_layer=env.L)[:2]
        n = n.to(torch.int64)
        idx = ((w * n) >> 32).clamp(max=5)
        a = acts.gather(1, idx[:, None, None].expand(-1, 1, 2))[:, 0]
        return torch.where((n > 0)[:, None], a, torch.zeros_like(a)).contiguous()
    return policy


def evaluate_vs_model(agent, opponent, num=1024, board_size=5, cube_layer=3, rng="mt19937", seed_offset=0, key=12345, max_steps=400,
                      use_rollout=True, chunk=16, deterministic=True):
    """Any agent against a trained policy as the env's opponent (the reference's eval_random.py / eval_minimax.py / eval_mcts.py run on an
    env built with opponent_policy=<path>).  opponent: {"kind": "mlp", "model": a2c.ActorCritic}; it plays its argmax on its canonical
    view (deterministic=False: samples).  agent: as in evaluate().  RandomAgent and 'hybrid' minimax run K steps per launch
    (ewn_step_k_vs, engine "ewn_step_k_vs"); the MCTS agent, callables, the other heuristics and use_rollout=False go ply by ply through
    step() (ewn_step_vs, engine "ewn_step_vs") -- both give the same per-episode results for the random and minimax agents; an "mlp"
    agent is evaluate()'s model-against-model path (ewn_policy_eval_vs)."""
    if not (isinstance(opponent, dict) and opponent.get("kind") == "mlp"):
        raise ValueError("evaluate_vs_model: the opponent is {'kind': 'mlp', 'model': ...}; evaluate() plays the classical opponents")
    if isinstance(agent, dict) and agent.get("kind") == "mlp":
        return _evaluate_vs_model(agent, opponent, num, board_size, cube_layer, rng, seed_offset, key, max_steps, chunk)
    model = opponent["model"]
    _model_on_board("evaluate_vs_model: the model", model, board_size)

    def seat(env):          # the refusal, then the model takes the opponent's seat: both before the reset
        if not env.supports_step_vs():
            raise ValueError("evaluate_vs_model: ewn_step_vs does not serve %dx%d boards with cube_layer %d" % (board_size, board_size, cube_layer))
        env.set_opponent_model(flat_policy_params(model).to(env.device), deterministic=deterministic, noise_key=key)
    env = _eval_env(None, num, board_size, cube_layer, rng, seed_offset, key, before_reset=seat)
    launch = _rollout_launch(env, agent, chunk) if use_rollout else None
    if launch is not None:
        return _play_chunks(env, launch, max_steps, chunk, num, "ewn_step_k_vs")
    policy = _stand_in_random(env) if isinstance(agent, dict) and agent.get("kind") == "random" else _policy(agent, cube_layer, key)
    return _play_plies(env, policy, max_steps, num, "ewn_step_vs")


def _row(r):
    return {k: r[k] for k in ("wins", "episodes", "win_rate", "ci95", "avg_length", "engine")}


def _classical_spec(kind, max_depth, heuristic, num_simulations, num_env_copies):
    return {"kind": kind, "max_depth": max_depth, "heuristic": heuristic, "num_simulations": num_simulations, "num_env_copies": num_env_copies}


def evaluate_agents_vs_model(model, names=("random", "minimax", "mcts"), num=1024, max_depth=5, num_simulations=10, num_env_copies=5,
                             board_size=5, cube_layer=3, heuristic="hybrid", rng="mt19937"):
    """every listed classical agent against the model as the opponent"""
    table = {}
    for a in names:
        agent = _classical_spec(a, max_depth, heuristic, num_simulations, num_env_copies)
        r = evaluate_vs_model(agent, {"kind": "mlp", "model": model}, num=num, board_size=board_size, cube_layer=cube_layer, rng=rng)
        table["%s vs opponent_model" % a] = _row(r)
    return table


def tournament(names=("random", "minimax", "mcts"), num=1024, max_depth=5, num_simulations=10, num_env_copies=5,
               board_size=5, cube_layer=3, heuristic="hybrid", rng="mt19937", sims=64, playouts=64, c_puct=1.5, playout_table=None):
    """eval_pairs.py:10-35: every (agent, opponent) pair, 1024 episodes, depth 5, 10 simulations by default.
    "playout_search" among the names (sims, playouts and c_puct are its own): the tree search on random playouts, an agent only --
    the env has no such opponent -- so it adds the rows "playout_search vs <every other name>".  playout_table: an EndgameTable or
    the path of a saved one (loaded once) whose exact values that search takes at the leaves it covers."""
    if playout_table is not None:
        from .endgame import EndgameTable, _accept_table
        playout_table = _accept_table("tournament", playout_table, board_size, "playout_table is for %%dx%%d boards, the tournament plays %dx%d" % (
            board_size, board_size), name="playout_table", load=EndgameTable.load)

    def spec(n):
        if n == "playout_search":
            return {"kind": n, "sims": sims, "playouts": playouts, "c_puct": c_puct, "endgame_table": playout_table}
        return _classical_spec(n, max_depth, heuristic, num_simulations, num_env_copies)
    table = {}
    for a in names:
        for o in (o for o in names if o != "playout_search"):
            r = evaluate(spec(a), spec(o), num=num, board_size=board_size, cube_layer=cube_layer, rng=rng)
            table["%s vs %s" % (a, o)] = _row(r)
    return table


def load_policy(path, board_size=5, cube_layer=3, device="cuda"):
    """The actor-critic of a checkpoint written by any of the trainers (A2CTrainer / PPOTrainer: a "model" state dict;
    FusedA2CTrainer / FusedPPOTrainer: the flat "params" vector), on `device`, in eval mode."""
    from .a2c import ActorCritic
    sd = torch.load(path, map_location=device, weights_only=True)
    model = ActorCritic(board_size, cube_layer * (cube_layer + 1) // 2).to(device)
    if "params" in sd:
        flat = sd["params"].to(device=device, dtype=torch.float32).reshape(-1)
        n = sum(p.numel() for p in model.parameters())
        if flat.numel() != n:
            raise ValueError("%s: %d parameters, a %dx%d actor-critic has %d (wrong --board_size / --cube_layer?)" % (
                path, flat.numel(), board_size, board_size, n))
        model.load_flat_parameters(flat)
    elif "model" in sd:
        model.load_state_dict(sd["model"])
    else:
        raise ValueError("%s holds neither a \"model\" state dict nor flat \"params\": not a checkpoint of these trainers" % path)
    return model.eval()


def evaluate_model(model, names=("random", "minimax"), num=1024, max_depth=5, num_simulations=10, num_env_copies=5, board_size=5,
                   cube_layer=3, heuristic="hybrid", rng="mt19937", lookahead=False, endgame_table=None, puct=None,
                   endgame_leaves=False, fused=False, leaves=1, puct_table=None):
    """eval_A2C.py's loop: the model's deterministic policy against every listed opponent; lookahead (1 / True, or 2): and, beside
    each, its lookahead policy of that many moves ({"kind": "mlp_lookahead", "plies": ...}) on the same episodes.  endgame_table (an
    EndgameTable or its path): every agent plays the exact move where the table covers the position ({"kind": "endgame"}, ply by ply).
    puct (a number of simulations): and its PUCT search of that budget ({"kind": "mlp_puct", "sims": ...}), rows "puct(SIMS) vs ..."
    fused (with puct): that search as one launch per move (ewn_puct_search): the same moves, so the same rows.
    leaves (with puct; 2..32): that search with up to so many leaves per tree and round (ewn_puct_search_wide): fewer
    rounds per move, other trees, so other rows.
    puct_table (with puct, leaves 1 and no endgame_table; an EndgameTable or its path): beside each puct row, the same search with the
    table's exact values at the leaves it covers, one launch per move (ewn_puct_search_eg), "puct(SIMS) + exact leaves vs ..."
    endgame_leaves (with lookahead and endgame_table): the table is not laid over the agents' moves; beside the lookahead's row
    stands the same lookahead with the table's exact values at the leaves it covers, "lookahead + exact leaves vs ..." """
    if endgame_leaves and (endgame_table is None or not lookahead):
        raise ValueError("evaluate_model: endgame_leaves goes with lookahead and an endgame_table")
    if puct_table is not None:
        if puct is None or endgame_table is not None:
            raise ValueError("evaluate_model: puct_table goes with puct and without endgame_table")
        from .endgame import EndgameTable, _accept_table
        from .search import _leaf_table_alone
        from .wide import _leaves
        _leaf_table_alone("evaluate_model", puct_table, None, _leaves("evaluate_model", leaves))
        puct_table = _accept_table("evaluate_model", puct_table, board_size, "the table is for %%dx%%d boards, the evaluation is on %dx%d" % (
            board_size, board_size), name="puct_table", load=EndgameTable.load)       # loaded once
    if endgame_table is not None:       # loaded once
        from .endgame import EndgameTable
        endgame_table = endgame_table if isinstance(endgame_table, EndgameTable) else EndgameTable.load(endgame_table)
    agents = [("model", {"kind": "mlp", "model": model})]       # (the row's label, the agent's spec), in the order of the rows
    if lookahead:
        plies = 2 if int(lookahead) == 2 else 1
        label = "lookahead(2)" if plies == 2 else "lookahead"
        agents.append((label, {"kind": "mlp_lookahead", "model": model, "plies": plies}))
        if endgame_leaves:
            agents.append((label + " + exact leaves", {"kind": "mlp_lookahead", "model": model, "plies": plies, "endgame_table": endgame_table}))
    if endgame_table is not None and not endgame_leaves:     # the table laid over every agent's moves; these tables have no PUCT row
        agents = [("endgame+" + label, {"kind": "endgame", "table": endgame_table, "fallback": spec}) for label, spec in agents]
    elif puct is not None:
        agents.append(("puct(%d)" % int(puct), {"kind": "mlp_puct", "model": model, "sims": int(puct), "fused": bool(fused), "leaves": leaves}))
        if puct_table is not None:
            agents.append(("puct(%d) + exact leaves" % int(puct), {"kind": "mlp_puct", "model": model, "sims": int(puct), "leaf_table": puct_table}))
    table = {}
    for o in names:
        opp = _classical_spec(o, max_depth, heuristic, num_simulations, num_env_copies)
        for label, spec in agents:
            r = evaluate(spec, opp, num=num, board_size=board_size, cube_layer=cube_layer, rng=rng)
            table["%s vs %s" % (label, o)] = _row(r)
    return table


def arena(model_a, model_b, num=1024, sims=64, board_size=5, cube_layer=3, seed_offset=0, key=12345, max_plies=None, c_puct=1.5,
          terminal_value=1.0, whole_games=True):
    """Two networks' PUCT searches of `sims` simulations against each other, whole games in one launch (arena_puct_games,
    ewn_puct_arena): what tells whether checkpoint A is stronger than checkpoint B at the strength both are used at.
    Game m starts from the reset position and dice of seed seed_offset + m // 2, and first[m] = m & 1: every start position is
    played twice, once with each network moving first.  No root noise, the most visited move; the dice of game m are those of the
    global game 2 * seed_offset + m under `key`.  whole_games=False plays the same games through arena_puct, ply by ply
    (ewn_puct_search): the same results.  Returns wins_a, wins_b, undecided (cut at max_plies), episodes, A's win_rate with the
    Wilson ci95, avg_length (plies), the two halves a_first and b_first, each {wins_a, episodes}, and the engine."""
    from .arena import arena_puct, arena_puct_games
    for model in (model_a, model_b):
        _model_on_board("arena: a model", model, board_size)
    env = _eval_env(None, (num + 1) // 2, board_size, cube_layer, "mt19937", seed_offset, key)
    boards = env.board.repeat_interleave(2, 0)[:num].contiguous()
    dice = env.dice.repeat_interleave(2, 0)[:num].contiguous()
    first = (torch.arange(num, device=env.device) & 1).to(torch.int8)
    pa, pb = flat_policy_params(model_a).to(env.device), flat_policy_params(model_b).to(env.device)
    play = arena_puct_games if whole_games else arena_puct
    rec = play(boards, dice, pa, pb, first, sims=sims, max_plies=max_plies, c_puct=c_puct, terminal_value=terminal_value, key=key,
               game_offset=2 * seed_offset, cube_layer=cube_layer)
    res, a_moves_first = rec["result_a"], rec["first"] == 0
    wins_a, wins_b = int((res > 0).sum().item()), int((res < 0).sum().item())
    lo, hi = wilson(wins_a, num)
    half = lambda sel: {"wins_a": int(((res > 0) & sel).sum().item()), "episodes": int(sel.sum().item())}   # noqa: E731
    return {"wins_a": wins_a, "wins_b": wins_b, "undecided": num - wins_a - wins_b, "episodes": num, "win_rate": wins_a / num if num else 0.0,
            "ci95": [lo, hi], "avg_length": float(rec["plies"].float().mean().item()) if num else 0.0, "a_first": half(a_moves_first),
            "b_first": half(~a_moves_first), "engine": "ewn_puct_arena" if whole_games else "ewn_puct_search"}


def _parser():
    ap = argparse.ArgumentParser(description="agent-vs-opponent win-rate matrix (counterpart of eval_pairs.py); with --model, a "
                                             "trained policy against each listed opponent (counterpart of eval_A2C.py)")
    ap.add_argument("--agents", nargs="+", default=["random", "minimax", "mcts"],
                    help="random, minimax, mcts; without --model also playout_search (the tree search on random playouts, an agent only)")
    ap.add_argument("--sims", type=int, default=64, help="playout_search: simulations per move")
    ap.add_argument("--playouts", type=int, default=64, help="playout_search: random playouts per leaf")
    ap.add_argument("--c_puct", type=float, default=1.5, help="playout_search and --arena: the exploration constant")
    ap.add_argument("--playout_table", default=None, metavar="PATH",
                    help="playout_search: a saved EndgameTable; the leaves it covers are worth their exact value and run no playouts")
    ap.add_argument("--model", default=None, help="checkpoint (best.pt) of any of the trainers: evaluate its deterministic policy")
    ap.add_argument("--opponent_model", default=None, help="a checkpoint that plays the opponent (its argmax): against --model, or "
                                                           "without --model against every agent of --agents")
    ap.add_argument("--lookahead", nargs="?", const=1, default=None, type=int, choices=(1, 2),
                    help="with --model: beside the raw policy, its lookahead on its own value net (ewn_predict_lookahead) against the "
                         "same opponents; the bare flag or 1: one move ahead, 2: two moves")
    ap.add_argument("--puct", default=None, type=int, metavar="SIMS",
                    help="with --model: beside the raw policy, its PUCT search of SIMS simulations (predict_puct) against the same "
                         "opponents, rows \"puct(SIMS) vs ...\"")
    ap.add_argument("--arena", default=None, type=int, metavar="SIMS",
                    help="with --model and --opponent_model: the two checkpoints' PUCT searches of SIMS simulations against each other, "
                         "whole games in one kernel launch (ewn_puct_arena), every start position once with each moving first, row "
                         "\"arena(SIMS): model vs opponent_model\"; it reads --num, --c_puct, --board_size and --cube_layer, and no "
                         "other flag (no --agents, no classical opponent's settings, no --rng: the dice are the search's own)")
    ap.add_argument("--fused", action="store_true",
                    help="with --puct: the search of a move in one kernel launch (ewn_puct_search) instead of the staged launches; the "
                         "same moves")
    ap.add_argument("--leaves", type=int, default=1, metavar="N",
                    help="with --puct: up to N leaves per tree and round in one kernel launch per move (ewn_puct_search_wide): about "
                         "SIMS / N rounds instead of SIMS + 1; another tree than N = 1, so not always the same moves")
    ap.add_argument("--puct_table", default=None, metavar="PATH",
                    help="with --puct (and --leaves 1): a saved EndgameTable; beside each puct row, the same search with the table's "
                         "exact values at the leaves it covers, one launch per move (ewn_puct_search_eg), rows \"puct(SIMS) + exact "
                         "leaves vs ...\"")
    ap.add_argument("--endgame_table", default=None,
                    help="with --model: a saved EndgameTable; the model (and its --lookahead) plays the exact move wherever the table "
                         "covers the position")
    ap.add_argument("--endgame_leaves", action="store_true",
                    help="with --lookahead and --endgame_table: the table is not laid over the moves; beside the lookahead's row, the "
                         "same lookahead with the table's exact values at the leaves it covers (\"lookahead + exact leaves vs ...\")")
    ap.add_argument("--num", type=int, default=1024)
    ap.add_argument("--max_depth", type=int, default=5)
    ap.add_argument("--heuristic", default="hybrid")
    ap.add_argument("--num_simulations", type=int, default=10)
    ap.add_argument("--num_env_copies", type=int, default=5)
    ap.add_argument("--board_size", type=int, default=5)
    ap.add_argument("--cube_layer", type=int, default=3)
    ap.add_argument("--rng", default="mt19937")
    return ap


def main():
    ap = _parser()
    a = ap.parse_args()
    if a.arena is not None:
        if a.model is None or a.opponent_model is None:
            ap.error("--arena goes with --model and --opponent_model: it plays the two checkpoints' searches against each other")
        if (a.puct is not None or a.lookahead or a.fused or a.leaves != 1 or a.puct_table or a.endgame_table or a.endgame_leaves
                or a.playout_table):
            ap.error("--arena does not go with --puct, --lookahead, --fused, --leaves or the table flags")
        if not 0 <= a.arena <= 4096:
            ap.error("--arena takes 0..4096 simulations")
    if a.lookahead and (a.model is None or a.opponent_model is not None):
        ap.error("--lookahead goes with --model and the classical opponents of --agents")
    if a.puct is not None and (a.model is None or a.opponent_model is not None or a.endgame_table):
        ap.error("--puct goes with --model and the classical opponents of --agents, without --endgame_table")
    if a.puct is not None and not 0 <= a.puct <= 4096:
        ap.error("--puct takes 0..4096 simulations")
    if a.fused and a.puct is None:
        ap.error("--fused goes with --puct")
    if a.leaves != 1 and (a.puct is None or not 1 <= a.leaves <= 32):
        ap.error("--leaves goes with --puct and takes 1..32")
    if a.puct_table and (a.puct is None or a.leaves != 1):
        ap.error("--puct_table goes with --puct and --leaves 1")
    if a.endgame_table and (a.model is None or a.opponent_model is not None):
        ap.error("--endgame_table goes with --model and the classical opponents of --agents")
    if a.endgame_leaves and not (a.endgame_table and a.lookahead):
        ap.error("--endgame_leaves goes with --lookahead and --endgame_table")
    if "playout_search" in a.agents and (a.model is not None or a.opponent_model is not None):
        ap.error("playout_search among --agents goes without --model and --opponent_model")
    if a.playout_table and "playout_search" not in a.agents:
        ap.error("--playout_table goes with playout_search among --agents")
    if a.arena is not None:
        r = arena(load_policy(a.model, a.board_size, a.cube_layer), load_policy(a.opponent_model, a.board_size, a.cube_layer), num=a.num,
                  sims=a.arena, board_size=a.board_size, cube_layer=a.cube_layer, c_puct=a.c_puct)
        t = {"arena(%d): model vs opponent_model" % a.arena: dict(r, wins=r["wins_a"])}
    elif a.opponent_model is not None and a.model is None:
        t = evaluate_agents_vs_model(load_policy(a.opponent_model, a.board_size, a.cube_layer), a.agents, a.num, a.max_depth,
                                     a.num_simulations, a.num_env_copies, a.board_size, a.cube_layer, a.heuristic, a.rng)
    elif a.opponent_model is not None:
        r = evaluate({"kind": "mlp", "model": load_policy(a.model, a.board_size, a.cube_layer)},
                     {"kind": "mlp", "model": load_policy(a.opponent_model, a.board_size, a.cube_layer)},
                     num=a.num, board_size=a.board_size, cube_layer=a.cube_layer, rng=a.rng)
        t = {"model vs opponent_model": _row(r)}
    elif a.model is not None:
        model = load_policy(a.model, a.board_size, a.cube_layer)
        t = evaluate_model(model, a.agents, a.num, a.max_depth, a.num_simulations, a.num_env_copies, a.board_size, a.cube_layer,
                           a.heuristic, a.rng, lookahead=a.lookahead or False, endgame_table=a.endgame_table, puct=a.puct,
                           endgame_leaves=a.endgame_leaves, fused=a.fused, leaves=a.leaves, puct_table=a.puct_table)
    else:
        t = tournament(a.agents, a.num, a.max_depth, a.num_simulations, a.num_env_copies, a.board_size, a.cube_layer,
                       a.heuristic, a.rng, sims=a.sims, playouts=a.playouts, c_puct=a.c_puct, playout_table=a.playout_table)
    for k, v in t.items():
        print("%-22s win rate %.3f  (95%% CI %.3f-%.3f, %d/%d, %.1f steps/episode)  %s"
              % (k, v["win_rate"], v["ci95"][0], v["ci95"][1], v["wins"], v["episodes"], v["avg_length"], v["engine"]))
    print(json.dumps(t))


if __name__ == "__main__":
    main()
