"""tournament.evaluate / evaluate_vs_model, cell by cell: which engine plays a cell ("engine" of the result), that its chunked loop
gives the same episodes whatever the chunk and -- where the per-step loop plays the same moves -- the per-step loop's, that the
MT19937-compat cells end through check_rng(), the keys of the result, and the refusals.  Small on purpose: 32 episodes a cell; the
table layers above these two functions have their own tests."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_policy_eval import f64_bits, trained  # noqa: E402

KEYS = {"scores", "lengths", "wins", "episodes", "win_rate", "engine", "ci95", "avg_score", "avg_length"}
NUM = 32
RANDOM = {"kind": "random"}
MINIMAX = {"kind": "minimax", "max_depth": 3}
MCTS = {"kind": "mcts", "num_simulations": 3, "num_env_copies": 2}

# a chunked cell's per-step loop (use_rollout=False):
SAME = "same"        # plays the engine's moves: the same episodes, bit for bit
OTHER = "other"      # plays other moves by design, so only its engine name is checked: the random agent of evaluate() draws from
#                      predict_random's stream per step and from ewn_step_k's hash stream in the engine
NONE = None          # there is none: a model against a model is ewn_policy_eval_vs or an error


def cells(model, policy):
    """(name, function, agent, opponent, keywords, engine, per-step loop) of every 5x5 cell; model: the trained actor-critic, policy: a
    callable (board, dice, t) -> actions"""
    mlp = {"kind": "mlp", "model": model}
    return [
        ("random vs minimax", "evaluate", RANDOM, MINIMAX, {}, "ewn_step_k", OTHER),
        ("minimax vs random mt19937", "evaluate", MINIMAX, RANDOM, {"rng": "mt19937"}, "ewn_step_k", SAME),
        ("minimax(2, attk) vs random", "evaluate", {"kind": "minimax", "max_depth": 2, "heuristic": "attk"}, RANDOM, {}, "ewn_step", NONE),
        ("mcts vs random", "evaluate", MCTS, RANDOM, {}, "ewn_step_k_agent", SAME),
        ("minimax vs mcts", "evaluate", MINIMAX, MCTS, {}, "ewn_step_k_agent", SAME),
        ("mlp vs minimax", "evaluate", mlp, MINIMAX, {}, "ewn_policy_eval", SAME),
        ("mlp vs mcts", "evaluate", mlp, MCTS, {}, "ewn_policy_eval_mcts", SAME),
        ("mlp vs mlp", "evaluate", mlp, mlp, {}, "ewn_policy_eval_vs", NONE),
        ("mlp_lookahead vs random", "evaluate", {"kind": "mlp_lookahead", "model": model}, RANDOM, {}, "ewn_step", NONE),
        ("mlp_puct(8) vs random", "evaluate", {"kind": "mlp_puct", "model": model, "sims": 8, "fused": False}, RANDOM, {}, "ewn_step", NONE),
        ("mlp_puct(8) fused vs random", "evaluate", {"kind": "mlp_puct", "model": model, "sims": 8, "fused": True}, RANDOM, {}, "ewn_step", NONE),
        ("callable vs random", "evaluate", policy, RANDOM, {}, "ewn_step", NONE),
        ("random vs model", "evaluate_vs_model", RANDOM, mlp, {}, "ewn_step_k_vs", SAME),
        ("minimax vs model", "evaluate_vs_model", MINIMAX, mlp, {}, "ewn_step_k_vs", SAME),
        ("mcts vs model", "evaluate_vs_model", MCTS, mlp, {}, "ewn_step_vs", NONE),
        ("mlp vs model", "evaluate_vs_model", mlp, mlp, {}, "ewn_policy_eval_vs", NONE),
    ]


CHUNKED = ("ewn_step_k", "ewn_step_k_agent", "ewn_policy_eval", "ewn_policy_eval_mcts", "ewn_policy_eval_vs", "ewn_step_k_vs")
PER_STEP = {"evaluate": "ewn_step", "evaluate_vs_model": "ewn_step_vs"}


def play(cell, **kw):
    from ewn_gym_amd import tournament
    _, fn, agent, opponent, own, _, _ = cell
    return getattr(tournament, fn)(agent, opponent, num=NUM, **dict(own, **kw))


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.fixture(scope="module")
def table(ea):
    tr = trained(ea, 5)
    return cells(tr.model, tr.policy_fn())


def test_the_model_plays_games_of_several_plies(ea):
    """the recipe's own stop rule: an untrained model forfeits on move one and would hide a loop that stops early"""
    from ewn_gym_amd.tournament import evaluate
    r = evaluate({"kind": "mlp", "model": trained(ea, 5).model}, RANDOM, num=256, board_size=5, rng="philox")
    assert r["avg_length"] >= 5, r["avg_length"]


@pytest.mark.parametrize("i", range(16), ids=[c[0] for c in cells(None, None)])
def test_cell(table, i):
    cell = table[i]
    name, fn, _, _, _, engine, per_step = cell
    r = play(cell)                                  # the default chunk, 16; the mt19937 cells (the default rng) end through check_rng()
    assert r["engine"] == engine, (name, r["engine"])
    assert set(r) == KEYS, (name, sorted(r))
    assert r["episodes"] == NUM and r["scores"].dtype == torch.float64 and r["lengths"].dtype == torch.int32
    assert int(r["lengths"].min()) >= 1 and r["wins"] == int((r["scores"] > 0).sum())
    if engine not in CHUNKED:
        assert per_step is NONE
        return
    others = [("chunk=3", play(cell, use_rollout=True, chunk=3), engine)]   # below the shortest game: several boundaries, lanes done and not
    if per_step is not NONE:
        others.append(("use_rollout=False", play(cell, use_rollout=False), PER_STEP[fn]))
    for what, q, e in others:
        assert q["engine"] == e and set(q) == KEYS, (name, what, q["engine"])
        if what == "chunk=3" or per_step == SAME:
            assert torch.equal(f64_bits(q["scores"]), f64_bits(r["scores"])), (name, what)
            assert torch.equal(q["lengths"], r["lengths"]) and q["wins"] == r["wins"], (name, what)


@pytest.mark.parametrize("agent,engine", [("random", "ewn_step_k"), ("mlp", "ewn_policy_eval")])
def test_a_7x7_cell(ea, agent, engine):
    """engine name and keys only: the actor-critic is untrained"""
    from ewn_gym_amd.a2c import ActorCritic
    from ewn_gym_amd.tournament import evaluate
    torch.manual_seed(7)
    spec = RANDOM if agent == "random" else {"kind": "mlp", "model": ActorCritic(7, 6).cuda()}
    r = evaluate(spec, MINIMAX, num=NUM, board_size=7)
    assert r["engine"] == engine and set(r) == KEYS and r["episodes"] == NUM


def test_refusals(table):
    from ewn_gym_amd.tournament import evaluate, evaluate_vs_model
    mlp = table[7][2]
    with pytest.raises(ValueError):
        evaluate(RANDOM, mlp, num=NUM)
    with pytest.raises(ValueError):
        evaluate_vs_model(RANDOM, MINIMAX, num=NUM)
