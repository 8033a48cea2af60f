"""ewn_policy_eval_mcts: a trained policy's argmax against the flat Monte-Carlo opponent in the engine, K steps per launch.

One helper (_replay) carries every comparison, in two parts, because an argmax over bf16 x 3 logits and one over torch fp32 logits may
differ where two logits nearly tie, and such a step must not be able to fail or hide anything else:
  1. transitions, exact: a second env is stepped with ewn_step (pinned to the oracle by the rest of the suite) on the actions the
     kernel recorded; states, RNG headers and totals are equal bit for bit after every chunk;
  2. the recorded actions are the model's argmax wherever a head's top-two gap exceeds 2e-5 (twice the 1e-5 to which
     tests/test_gpu_policy.py holds the engine's logits to torch); at most 1 % of a case's played lane-steps may be excused.
Then tournament.evaluate, the CLI, the trainer's evaluation, argument validation, exact guard zones and determinism."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402

GAP = 2e-5          # a head whose two best logits are closer than this may be decided either way
EXCUSED_CAP = 0.01  # share of the played lane-steps of a case that may be excused by GAP


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


def _envs(ea, S, N, rng, sims, lane_offset=0, seed_stride=None, n=2, philox_key=77):
    kw = dict(board_size=S, opponent_policy="mcts", num_simulations=sims[0], num_env_copies=sims[1], rng=rng, autoreset=False,
              philox_key=philox_key, lane_offset=lane_offset, seed_stride=seed_stride)
    return [ea.VecEWN(N, **kw) for _ in range(n)]


def _replay(ea, S, N, rng, sims=(10, 5), K=8, seed_offset=0, pre_done=False, lane_offset=0, seed_stride=None, max_steps=400,
            philox_key=77):
    """env `a` plays eval_policy in chunks of K with the action column recorded; env `b`, same seeds, is stepped with ewn_step on
    a's recorded actions.  Returns a's totals, the recorded rows and b's per-episode results."""
    from ewn_gym_amd.tournament import flat_policy_params
    model = trained(ea, S).model
    a, b = _envs(ea, S, N, rng, sims, lane_offset, seed_stride, philox_key=philox_key)
    assert a.supports_policy_eval_mcts() and not a.supports_policy_eval()
    seeds = torch.arange(seed_offset + lane_offset, seed_offset + lane_offset + N, dtype=torch.int32)
    a.reset(seeds=seeds)
    b.reset(seeds=seeds)
    if pre_done:
        # lanes finished before the first launch: two plies played by both envs (some episodes end there), and every 7th lane frozen
        for _ in range(2):
            for env in (a, b):
                env.step(model.act(env.board, env.dice, deterministic=True)[0])
        for env in (a, b):
            env.done[::7] = 1
        assert bool((a.done != 0).any()) and not bool((a.done != 0).all())
    params = flat_policy_params(model)
    ctx = (S, N, rng, sims, K, seed_offset, pre_done, lane_offset)
    totals = a.alloc_totals()
    action = torch.full((K, N, 2), -7, dtype=torch.int8, device="cuda")
    score = torch.zeros(N, dtype=torch.float64, device="cuda")
    length = torch.zeros(N, dtype=torch.int32, device="cuda")
    eps = torch.zeros(N, dtype=torch.int32, device="cuda")
    hdr = slice(0, 4 * N)                                   # the N RNG headers (seed, draws, next seed, flags) lead the buffer
    rows, played, excused, wrong = [], 0, 0, 0
    for _ in range(0, max_steps, K):
        action.fill_(-7)
        a.eval_policy(K, params, totals, action=action)
        rows.append(action.clone())
        for k in range(K):
            alive = b.done == 0
            rec = action[k]
            assert bool((rec[~alive] == -7).all()), (ctx, "a row of a lane not in play was written", k)
            if not bool(alive.any()):
                continue
            # part 2: the recorded action against torch's fp32 argmax, head by head, wherever the head's top-two gap exceeds GAP
            with torch.no_grad():
                l0, l1, _ = model(b.board, b.dice)
            for head, lg in enumerate((l0, l1)):
                top = lg.topk(2, dim=1)
                tie = (top.values[:, 0] - top.values[:, 1]) <= GAP
                mine = rec[:, head].to(torch.int64)
                differs = alive & (mine != lg.argmax(1))
                ok = differs & tie & (mine == top.indices[:, 1])      # excused: the runner-up of a near-tie, nothing else
                excused += int(ok.sum())
                wrong += int((differs & ~ok).sum())
            played += int(alive.sum())
            # part 1: b plays a's recorded actions (a finished lane is not stepped: its action does not matter)
            act = torch.where(alive[:, None], rec, torch.zeros_like(rec)).contiguous()
            _, _, r, term, _, _ = b.step(act)
            just = alive & (term != 0)
            score = torch.where(just, r, score)
            length += alive.to(torch.int32)
            eps += just.to(torch.int32)
        torch.cuda.synchronize()
        assert torch.equal(a.board, b.board), ctx
        assert torch.equal(a.dice, b.dice), ctx
        assert torch.equal(a.done, b.done), ctx
        assert torch.equal(a.rng_state.view(-1)[hdr], b.rng_state.view(-1)[hdr]), ctx
        assert torch.equal(f64_bits(totals["return_sum"]), f64_bits(score)), ctx
        assert torch.equal(totals["n_steps"], length), ctx
        assert torch.equal(totals["n_episodes"], eps), ctx
        assert torch.equal(totals["n_wins"], ((score > 0) & (eps > 0)).to(torch.int32)), ctx
        if bool((a.done != 0).all()):
            break
    a.check_rng()
    assert bool((a.done != 0).all()), (ctx, "a lane did not finish")
    live = length > 0
    mean_len = float(length[live].float().mean())
    print("policy_eval_mcts %s: played %d lane-steps, mean length %.2f, excused %d, wrong %d" % (ctx, played, mean_len, excused, wrong))
    assert mean_len >= 3.0, (ctx, mean_len)                # the policy plays, it does not just forfeit
    assert wrong == 0, (ctx, "%d recorded actions differ from torch's argmax at a top-two gap above %g (%d excused below it, %d played)"
                        % (wrong, GAP, excused, played))
    assert excused <= EXCUSED_CAP * played, (ctx, "%d of %d played lane-steps excused by the near-tie rule" % (excused, played))
    return dict(totals=totals, rows=torch.cat(rows, 0), score=score, length=length, eps=eps, env=a)


@pytest.mark.parametrize("S,N,rng,sims,K,seed_offset,pre_done", [
    (5, 257, "mt19937", (10, 5), 8, 0, False),
    (5, 3000, "philox", (10, 5), 8, 0, False),
    (5, 257, "philox", (3, 2), 1, 0, False),
    (5, 3000, "mt19937", (3, 2), 8, 500, False),
    (5, 257, "mt19937", (10, 5), 8, 3, True),
    (7, 257, "mt19937", (10, 5), 8, 0, False),
    (7, 3000, "philox", (3, 2), 8, 0, False),
    (7, 257, "philox", (10, 5), 1, 11, False),
    (7, 3000, "mt19937", (10, 5), 8, 0, True),
], ids=str)
def test_eval_matches_ewn_step_and_the_models_argmax(ea, S, N, rng, sims, K, seed_offset, pre_done):
    _replay(ea, S, N, rng, sims=sims, K=K, seed_offset=seed_offset, pre_done=pre_done)


# The launcher takes 8 games per block and doubles that while N / (2 gpb) >= 2 048: every case above runs 8 games per block and one
# network wave.  The other block shapes need more lanes: 16 games per block from 32 768 lanes, 32 from 65 536, 64 (two network waves,
# tiles(gpb) = 2) from 131 072 and 128 (four: every wave of the block) from 262 144.  A partial last block each, MCTS(3 x 2) to keep
# the per-step replay short.
@pytest.mark.parametrize("S,N,rng,K,pre_done,gpb", [
    (5, 40001, "philox", 8, False, 16),
    (7, 65537, "mt19937", 8, False, 32),
    (5, 131073, "mt19937", 8, True, 64),
    (7, 131073, "philox", 5, False, 64),
    (5, 262145, "philox", 5, False, 128),
    (7, 262145, "mt19937", 8, True, 128),
], ids=str)
def test_eval_matches_ewn_step_at_every_block_shape(ea, S, N, rng, K, pre_done, gpb):
    g = 8
    while g < 128 and N // (2 * g) >= 2048:
        g *= 2
    assert g == gpb, "the case no longer runs the block shape it is here for: the launcher's rule (ewn_policy_eval_mcts) changed?"
    _replay(ea, S, N, rng, sims=(3, 2), K=K, pre_done=pre_done)


@pytest.mark.parametrize("S,rng", [(5, "mt19937"), (7, "philox")])
def test_shard_invariance(ea, S, rng):
    """one 512-lane env gives the results of two 256-lane envs built with lane_offset 0 / 256 and the matching seeds"""
    whole = _replay(ea, S, 512, rng, seed_stride=512)
    for lo in (0, 256):
        part = _replay(ea, S, 256, rng, lane_offset=lo, seed_stride=512)
        sl = slice(lo, lo + 256)
        assert torch.equal(f64_bits(part["score"]), f64_bits(whole["score"][sl])), (S, rng, lo)
        assert torch.equal(part["length"], whole["length"][sl]), (S, rng, lo)
        assert torch.equal(part["totals"]["n_wins"], whole["totals"]["n_wins"][sl]), (S, rng, lo)
        n = min(part["rows"].shape[0], whole["rows"].shape[0])
        assert torch.equal(part["rows"][:n], whole["rows"][:n, sl]), (S, rng, lo)
        assert bool((part["rows"][n:] == -7).all()) and bool((whole["rows"][n:, sl] == -7).all())
        assert torch.equal(part["env"].board, whole["env"].board[sl])


def test_graph_free_determinism(ea):
    """two runs from the same seeds give identical totals and action columns"""
    from ewn_gym_amd.tournament import flat_policy_params
    params = flat_policy_params(trained(ea, 5).model)
    runs = []
    for _ in range(2):
        env, = _envs(ea, 5, 1000, "mt19937", (10, 5), n=1)
        env.reset(seeds=torch.arange(1000, dtype=torch.int32))
        totals = env.alloc_totals()
        action = torch.full((40, 1000, 2), -7, dtype=torch.int8, device="cuda")
        for t0 in range(0, 40, 8):
            env.eval_policy(8, params, totals, action=action[t0:t0 + 8])
        torch.cuda.synchronize()
        runs.append((totals, action, env.board.clone(), env.done.clone()))
    (t0, a0, b0, d0), (t1, a1, b1, d1) = runs
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and torch.equal(d0, d1)
    assert torch.equal(f64_bits(t0["return_sum"]), f64_bits(t1["return_sum"]))
    for name in ("n_steps", "n_episodes", "n_wins"):
        assert torch.equal(t0[name], t1[name]), name
    assert int(t0["n_steps"].sum()) > 0


def test_eval_policy_rejects_malformed_buffers(ea):
    """params: contiguous float32 [P]; totals: the four [N] tensors of alloc_totals; action: contiguous int8 [>= K, N, 2] -- each
    violation raises ValueError before anything is launched; unsupported configurations raise the engine's error"""
    from ewn_gym_amd._lib import EwnError
    N, K = 300, 4
    env = ea.VecEWN(N, opponent_policy="mcts", rng="mt19937")
    env.reset(seeds=np.arange(N))
    assert env.supports_policy_eval_mcts()
    P = env.policy_param_count()
    good = torch.zeros(P, dtype=torch.float32, device="cuda")
    before = env.state_dict()
    for params in (torch.zeros(P - 1, device="cuda"), torch.zeros(P, dtype=torch.float64, device="cuda"), torch.zeros(P),
                   torch.zeros((P, 2), device="cuda")[:, 0]):
        with pytest.raises(ValueError, match="params"):
            env.eval_policy(K, params, env.alloc_totals())
    for name in ("return_sum", "n_steps", "n_episodes", "n_wins"):
        for bad in (None, torch.zeros(N + 1, dtype=env.alloc_totals()[name].dtype, device="cuda"), torch.zeros(N, dtype=torch.float32, device="cuda"),
                    torch.zeros(N, dtype=env.alloc_totals()[name].dtype)):
            t = env.alloc_totals()
            if bad is None:
                del t[name]
            else:
                t[name] = bad
            with pytest.raises(ValueError, match=name):
                env.eval_policy(K, good, t)
    for action in (torch.zeros((K - 1, N, 2), dtype=torch.int8, device="cuda"), torch.zeros((K, N, 2), dtype=torch.int16, device="cuda"),
                   torch.zeros((K, N + 1, 2), dtype=torch.int8, device="cuda"), torch.zeros((K, 2, N), dtype=torch.int8, device="cuda").transpose(1, 2),
                   torch.zeros((K, N, 2), dtype=torch.int8)):
        with pytest.raises(ValueError, match="action"):
            env.eval_policy(K, good, env.alloc_totals(), action=action)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in env.state_dict().items())
    shaped = ea.VecEWN(N, opponent_policy="mcts", rng="philox", shaped=True)
    assert not shaped.supports_policy_eval_mcts()
    with pytest.raises(EwnError):
        shaped.eval_policy(K, good, shaped.alloc_totals())
    six = ea.VecEWN(N, board_size=6, opponent_policy="mcts", rng="philox")
    assert not six.supports_policy_eval_mcts()


# ---------------------------------------------------------------- tournament.evaluate, the CLI, the trainer's evaluation

def test_evaluate_mlp_agent_against_mcts_runs_in_the_engine(ea):
    from ewn_gym_amd.a2c import ActorCritic
    from ewn_gym_amd.tournament import evaluate
    tr = trained(ea, 5)
    opp = dict(kind="mcts", num_simulations=10, num_env_copies=5)
    r = evaluate({"kind": "mlp", "model": tr.model}, opp, num=300, rng="mt19937", seed_offset=11, key=12345)
    assert r["engine"] == "ewn_policy_eval_mcts" and r["episodes"] == 300
    # the helper's replay on the same seeds and the same engine key (evaluate: philox_key = key ^ 0x5DEECE66D)
    h = _replay(ea, 5, 300, "mt19937", sims=(10, 5), K=16, seed_offset=11, philox_key=12345 ^ 0x5DEECE66D)
    assert torch.equal(f64_bits(r["scores"]), f64_bits(h["score"])) and torch.equal(r["lengths"], h["length"])
    assert r["wins"] == int((h["score"] > 0).sum()) == int(h["totals"]["n_wins"].sum())
    q = evaluate({"kind": "mlp", "model": tr.model}, opp, num=300, rng="mt19937", seed_offset=11, key=12345, use_rollout=False)
    assert q["engine"] == "ewn_step" and q["episodes"] == 300
    torch.manual_seed(0)
    m6 = ActorCritic(6, 6).cuda()
    r6 = evaluate({"kind": "mlp", "model": m6}, opp, num=64, board_size=6)
    assert r6["engine"] == "ewn_step" and r6["episodes"] == 64 and int(r6["lengths"].min()) >= 1


def test_tournament_cli_runs_model_vs_mcts_in_the_engine(ea, tmp_path, monkeypatch, capsys):
    from ewn_gym_amd import tournament
    path = str(tmp_path / "fused_a2c.pt")
    trained(ea, 5).save(path)
    monkeypatch.setattr(sys, "argv", ["tournament", "--model", path, "--agents", "mcts", "random", "--num", "64"])
    tournament.main()
    out = capsys.readouterr().out
    assert "model vs mcts" in out and "model vs random" in out
    table = json.loads(out.strip().splitlines()[-1])
    assert table["model vs mcts"]["engine"] == "ewn_policy_eval_mcts" and table["model vs mcts"]["episodes"] == 64
    assert table["model vs random"]["engine"] == "ewn_policy_eval"
    assert "ewn_policy_eval_mcts" in [ln for ln in out.splitlines() if ln.startswith("model vs mcts")][0]


def test_train_a2c_evaluates_against_mcts_in_the_engine(ea, tmp_path, monkeypatch, capsys):
    from ewn_gym_amd import train_a2c
    argv = ["train_a2c", "--num_envs", "256", "--n_steps", "4", "--epoch_num", "1", "--timesteps_per_epoch", "2048",
            "--eval_opponent", "mcts", "--eval_episode_num", "32", "--save_dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_a2c.main()
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 1 and ep[0]["eval_engine"] == "ewn_policy_eval_mcts" and ep[0]["eval_s"] > 0


# ---------------------------------------------------------------- guard zones

@pytest.mark.parametrize("S,N", [(5, 257), (5, 3000), (7, 257), (7, 3000), (5, 131073), (7, 131073), (5, 262145), (7, 262145)])
def test_guard_zones(ea, S, N):
    """exact guard zones (tests/guarded_alloc.py) around the env state, the parameters, the totals and the action column; the
    cases from 131 073 lanes on run 64 and 128 games per block (two and four network waves)"""
    from ewn_gym_amd.tournament import flat_policy_params
    model = trained(ea, S).model
    alloc = GuardedAllocator()
    try:
        K = 6
        for sims, rng in (((10, 5), "mt19937"), ((3, 2), "philox")):
            with alloc.patch(tag="env"):
                env = ea.VecEWN(N, board_size=S, opponent_policy="mcts", num_simulations=sims[0], num_env_copies=sims[1], rng=rng,
                                autoreset=False, philox_key=5)
                totals = env.alloc_totals()
            env.reset(seeds=torch.arange(N, dtype=torch.int32))
            params = alloc.zeros(env.policy_param_count(), tag="params")
            params.copy_(flat_policy_params(model))
            action = alloc.zeros((K, N, 2), dtype=torch.int8, tag="action")
            for t in totals.values():
                assert alloc.owns(t)
            assert alloc.owns(env.board) and alloc.owns(env.rng_state)
            for _ in range(3):
                env.eval_policy(K, params, totals, action=action)
            torch.cuda.synchronize()
            alloc.check("S=%d N=%d MCTS%s %s" % (S, N, sims, rng))
            assert int(totals["n_steps"].sum()) > 0
    finally:
        alloc.clear()
