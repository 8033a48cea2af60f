"""ewn_policy_eval: a trained policy's argmax against RandomAgent / minimax max_depth 1-6 in the engine, K steps per launch.  The core
check is bit-exactness against the per-step path it replaces (model.act(deterministic=True) + ewn_step per ply, pinned to the oracle):
end states, RNG headers, per-episode returns and lengths.  Then tournament.evaluate's "mlp" agent, the CLI and the trainer's
evaluation, and exact guard zones around every buffer the kernel touches."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


_TRAINED = {}


def trained(ea, S):
    """a FusedA2CTrainer trained briefly against RandomAgent (shaped env, as train_a2c.py trains) until its deterministic policy plays
    games of several plies: evaluated against untrained weights the comparison would be mostly first-move forfeits"""
    if S not in _TRAINED:
        from ewn_gym_amd.a2c import FusedA2CTrainer
        from ewn_gym_amd.tournament import evaluate
        N = 4096
        env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_reward=-1.0,
                        illegal_move_tolerance=10, autoreset=True, shaped_refresh_on_reset=True, philox_key=11 + S)
        env.reset(seeds=torch.arange(N, dtype=torch.int32))
        tr = FusedA2CTrainer(env, n_steps=5, learning_rate=1e-3, seed=S)
        for _ in range(8):
            for _ in range(300):
                tr.collect_and_update()
            if evaluate({"kind": "mlp", "model": tr.model}, {"kind": "random"}, num=256, board_size=S, rng="philox")["avg_length"] >= 5:
                break
        torch.cuda.synchronize()
        _TRAINED[S] = tr
    return _TRAINED[S]


def f64_bits(t):
    return t.contiguous().view(torch.int64)


def _per_step(env, model, max_steps=400):
    """today's path: the model's argmax + one ewn_step per ply; per-episode final reward, plies played, finished / won, the actions"""
    N = env.N
    score = torch.zeros(N, dtype=torch.float64, device="cuda")
    length = torch.zeros(N, dtype=torch.int32, device="cuda")
    eps = torch.zeros(N, dtype=torch.int32, device="cuda")
    acts = []
    for _ in range(max_steps):
        alive = env.done == 0
        if not bool(alive.any()):
            break
        a = model.act(env.board, env.dice, deterministic=True)[0]
        acts.append((a.clone(), alive.clone()))
        _, _, r, term, _, _ = env.step(a)
        just = alive & (term != 0)
        score = torch.where(just, r, score)
        length += alive.to(torch.int32)
        eps += just.to(torch.int32)
    return score, length, eps, acts


def _engine(env, params, K, max_steps=400):
    totals = env.alloc_totals()
    action = torch.full((K, env.N, 2), -7, dtype=torch.int8, device="cuda")
    rows = []
    for _ in range(0, max_steps, K):
        action.fill_(-7)
        env.eval_policy(K, params, totals, action=action)
        rows.append(action.clone())
        if bool((env.done != 0).all()):
            break
    env.check_rng()
    return totals, torch.cat(rows, 0)


def _compare(ea, S, N, opp, rng, K=8, seed_offset=0, pre_done=False):
    from ewn_gym_amd.tournament import flat_policy_params
    model = trained(ea, S).model
    kw = dict(board_size=S, rng=rng, autoreset=False, philox_key=77, **opp)
    a, b = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    assert a.supports_policy_eval()
    seeds = torch.arange(seed_offset, seed_offset + N, dtype=torch.int32)
    a.reset(seeds=seeds)
    b.reset(seeds=seeds)
    if pre_done:
        # lanes finished before the first launch: two plies played by both paths (some episodes end there), and every 7th lane frozen
        for _ in range(2):
            for env in (a, b):
                env.step(model.act(env.board, env.dice, deterministic=True)[0])
        for env in (a, b):
            env.done[::7] = 1
        assert bool((a.done != 0).any()) and not bool((a.done != 0).all())
    params = flat_policy_params(model)
    totals, rows = _engine(a, params, K)
    score, length, eps, acts = _per_step(b, model)
    torch.cuda.synchronize()
    ctx = (S, N, opp, rng, seed_offset, pre_done)
    assert torch.equal(a.board, b.board), ctx
    assert torch.equal(a.dice, b.dice), ctx
    assert torch.equal(a.done, b.done) and bool((a.done != 0).all()), ctx
    hdr = slice(0, 4 * N)                                                               # the N RNG headers (seed, draws, next seed, flags) lead the buffer
    assert torch.equal(a.rng_state.view(-1)[hdr], b.rng_state.view(-1)[hdr]), ctx
    assert torch.equal(f64_bits(totals["return_sum"]), f64_bits(score)), ctx
    assert torch.equal(totals["n_steps"], length), ctx
    assert torch.equal(totals["n_episodes"], eps), ctx
    assert torch.equal(totals["n_wins"], ((score > 0) & (eps > 0)).to(torch.int32)), ctx
    # the action column: the argmax the per-step path played wherever the lane was in play, untouched elsewhere
    for t, (act, alive) in enumerate(acts):
        assert torch.equal(rows[t][alive], act[alive]), (ctx, t)
        assert bool((rows[t][~alive] == -7).all()), (ctx, t)
    live = length > 0
    assert float(length[live].float().mean()) >= 3.0, (ctx, float(length[live].float().mean()))   # the policy plays, it does not just forfeit
    return totals


@pytest.mark.parametrize("S,N,opp,rng,seed_offset,pre_done", [
    (5, 257, dict(opponent_policy="minimax", max_depth=5), "mt19937", 0, False),
    (5, 37, dict(opponent_policy="minimax", max_depth=6), "mt19937", 0, True),
    (5, 1000, dict(opponent_policy="minimax", max_depth=3, heuristic="attk"), "mt19937", 0, False),
    (5, 257, dict(opponent_policy="random"), "mt19937", 3, True),
    (5, 1000, dict(opponent_policy="minimax", max_depth=5), "philox", 500, False),
    (5, 257, dict(opponent_policy="minimax", max_depth=5, heuristic="min_dist"), "mt19937", 0, False),
    (7, 257, dict(opponent_policy="minimax", max_depth=5), "mt19937", 0, False),
    (7, 1000, dict(opponent_policy="minimax", max_depth=2), "philox", 0, True),
], ids=lambda v: str(v) if not isinstance(v, dict) else "-".join("%s=%s" % kv for kv in sorted(v.items())))
def test_eval_matches_the_per_step_path(ea, S, N, opp, rng, seed_offset, pre_done):
    _compare(ea, S, N, opp, rng, seed_offset=seed_offset, pre_done=pre_done)


def test_eval_matches_the_per_step_path_on_the_wide_blocks(ea):
    """more than 8 192 games: the 256-thread instance (the smaller evaluations run 64-thread blocks)"""
    _compare(ea, 5, 9000, dict(opponent_policy="minimax", max_depth=3), "philox", K=16)


def test_eval_policy_rejects_malformed_buffers(ea):
    """params: contiguous float32 [P]; totals: the four [N] tensors of alloc_totals; action: contiguous int8 [>= K, N, 2] -- each
    violation raises ValueError before anything is launched; unsupported configurations raise the engine's error"""
    from ewn_gym_amd._lib import EwnError
    N, K = 300, 4
    env = ea.VecEWN(N, opponent_policy="minimax", max_depth=5, rng="mt19937")
    env.reset(seeds=np.arange(N))
    P = env.policy_param_count()
    good = torch.zeros(P, dtype=torch.float32, device="cuda")
    before = env.state_dict()
    for params in (torch.zeros(P - 1, device="cuda"), torch.zeros(P, dtype=torch.float64, device="cuda"), torch.zeros(P),
                   torch.zeros((P, 2), device="cuda")[:, 0]):
        with pytest.raises(ValueError, match="params"):
            env.eval_policy(K, params, env.alloc_totals())
    for name in ("return_sum", "n_steps", "n_episodes", "n_wins"):
        for bad in (None, torch.zeros(N + 1, dtype=env.alloc_totals()[name].dtype, device="cuda"), torch.zeros(N, dtype=torch.float32, device="cuda")):
            t = env.alloc_totals()
            if bad is None:
                del t[name]
            else:
                t[name] = bad
            with pytest.raises(ValueError, match=name):
                env.eval_policy(K, good, t)
    for action in (torch.zeros((K - 1, N, 2), dtype=torch.int8, device="cuda"), torch.zeros((K, N, 2), dtype=torch.int16, device="cuda"),
                   torch.zeros((K, N + 1, 2), dtype=torch.int8, device="cuda"), torch.zeros((K, 2, N), dtype=torch.int8, device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="action"):
            env.eval_policy(K, good, env.alloc_totals(), action=action)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in env.state_dict().items())
    shaped = ea.VecEWN(N, opponent_policy="minimax", max_depth=3, rng="philox", shaped=True)
    assert not shaped.supports_policy_eval()
    with pytest.raises(EwnError):
        shaped.eval_policy(K, good, shaped.alloc_totals())


# ---------------------------------------------------------------- tournament.evaluate, the CLI, the trainer's evaluation

@pytest.mark.parametrize("opp", [dict(kind="minimax", max_depth=5), dict(kind="random")], ids=["minimax5", "random"])
def test_evaluate_mlp_agent_runs_in_the_engine(ea, opp):
    from ewn_gym_amd.tournament import evaluate
    tr = trained(ea, 5)
    r = evaluate({"kind": "mlp", "model": tr.model}, opp, num=300, rng="mt19937", seed_offset=11)
    q = evaluate(tr.policy_fn(True), opp, num=300, rng="mt19937", seed_offset=11)
    assert r["engine"] == "ewn_policy_eval" and q["engine"] == "ewn_step"
    assert torch.equal(f64_bits(r["scores"]), f64_bits(q["scores"])) and torch.equal(r["lengths"], q["lengths"])
    assert r["wins"] == q["wins"] and r["ci95"] == q["ci95"]


def test_evaluate_mlp_agent_falls_back_where_the_engine_has_no_instance(ea):
    from ewn_gym_amd.a2c import ActorCritic
    from ewn_gym_amd.tournament import evaluate
    tr = trained(ea, 5)
    opp = dict(kind="minimax", max_depth=5, heuristic="two_min_dist")
    r = evaluate({"kind": "mlp", "model": tr.model}, opp, num=64)
    q = evaluate(tr.policy_fn(True), opp, num=64)
    assert r["engine"] == "ewn_step" and torch.equal(r["scores"], q["scores"]) and torch.equal(r["lengths"], q["lengths"])
    torch.manual_seed(0)
    m6 = ActorCritic(6, 6).cuda()
    r = evaluate({"kind": "mlp", "model": m6}, {"kind": "random"}, num=64, board_size=6)
    assert r["engine"] == "ewn_step" and r["episodes"] == 64 and int(r["lengths"].min()) >= 1


def test_tournament_cli_loads_trainer_checkpoints(ea, tmp_path, monkeypatch, capsys):
    from ewn_gym_amd import tournament
    from ewn_gym_amd.ppo import PPOTrainer
    fused = trained(ea, 5)
    p_fused = str(tmp_path / "fused_a2c.pt")
    fused.save(p_fused)
    env = ea.VecEWN(256, opponent_policy="random", rng="philox", shaped=True, reward=10.0, autoreset=True, philox_key=3)
    env.reset(seeds=torch.arange(256, dtype=torch.int32))
    ppo = PPOTrainer(env, n_steps=4, n_epochs=1, seed=4)
    p_ppo = str(tmp_path / "torch_ppo.pt")
    ppo.save(p_ppo)
    for path, model in ((p_fused, fused.model), (p_ppo, ppo.model)):
        loaded = tournament.load_policy(path)
        for p, q in zip(loaded.parameters(), model.parameters()):
            assert torch.equal(p, q)
        monkeypatch.setattr(sys, "argv", ["tournament", "--model", path, "--agents", "minimax", "random", "--num", "64"])
        tournament.main()
        out = capsys.readouterr().out
        assert "model vs minimax" in out and "model vs random" in out
        table = json.loads(out.strip().splitlines()[-1])
        assert table["model vs minimax"]["engine"] == table["model vs random"]["engine"] == "ewn_policy_eval"
        assert table["model vs minimax"]["episodes"] == 64
    with pytest.raises(ValueError, match="board_size"):
        tournament.load_policy(p_fused, board_size=7)


def test_train_a2c_evaluates_in_the_engine(ea, tmp_path, monkeypatch, capsys):
    from ewn_gym_amd import train_a2c
    argv = ["train_a2c", "--num_envs", "256", "--n_steps", "4", "--epoch_num", "1", "--timesteps_per_epoch", "2048",
            "--eval_episode_num", "32", "--save_dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_a2c.main()
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 1 and ep[0]["eval_engine"] == "ewn_policy_eval" and ep[0]["eval_s"] > 0
    assert os.path.exists(os.path.join(str(tmp_path), "best.pt"))


# ---------------------------------------------------------------- guard zones

@pytest.mark.parametrize("S,N", [(5, 257), (5, 3000), (7, 257), (7, 3000)])
def test_guard_zones(ea, S, N):
    """exact guard zones (tests/guarded_alloc.py) around the env state, the tables, the parameters, the totals and the action column"""
    from ewn_gym_amd import vec_env
    from ewn_gym_amd.tournament import flat_policy_params
    model = trained(ea, S).model
    saved = dict(vec_env._TABLES)
    vec_env._TABLES.clear()
    tables, alloc = GuardedAllocator(), GuardedAllocator()
    try:
        with tables.patch(tag="tables"):
            assert vec_env.search_tables(S, 3, torch.device("cuda")) is not None
        K = 6
        for opp, rng in ((dict(opponent_policy="minimax", max_depth=5), "mt19937"), (dict(opponent_policy="random"), "philox")):
            with alloc.patch(tag="env"):
                env = ea.VecEWN(N, board_size=S, rng=rng, autoreset=False, philox_key=5, **opp)
                totals = env.alloc_totals()
            env.reset(seeds=torch.arange(N, dtype=torch.int32))
            params = alloc.zeros(env.policy_param_count(), tag="params")
            params.copy_(flat_policy_params(model))
            action = alloc.zeros((K, N, 2), dtype=torch.int8, tag="action")
            for t in totals.values():
                assert alloc.owns(t)
            for _ in range(3):
                env.eval_policy(K, params, totals, action=action)
            torch.cuda.synchronize()
            alloc.check("S=%d N=%d %s" % (S, N, opp))
            tables.check("tables")
            assert int(totals["n_steps"].sum()) > 0
    finally:
        alloc.clear()
        tables.clear()
        vec_env._TABLES.clear()
        vec_env._TABLES.update(saved)
