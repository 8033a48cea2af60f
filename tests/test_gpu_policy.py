"""ewn_step_k_policy: K env steps per launch with the actor-critic of train.py:35-63 as the agent (the rollout collector of the
trainer as one kernel).  The network's outputs against a plain fp32 torch forward of the same parameters on the same
observations; the sampling against the recorded noise and statistically; every transition against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def cpu(t):
    return t.detach().cpu().numpy()


def make_model(S, seed, head_gain=3.0):
    from ewn_gym_amd.a2c import ActorCritic
    torch.manual_seed(seed)
    m = ActorCritic(S, 6).cuda()
    with torch.no_grad():          # SB3's 0.01-gain action head gives near-uniform policies: spread the logits so that sampling is tested
        m.action_net.weight.mul_(head_gain / 0.01)
        m.action_net.bias.uniform_(-0.5, 0.5)
        m.value_net.bias.fill_(0.25)
        for seq in (m.pi, m.vf):
            for lin in seq:
                if hasattr(lin, "bias"):
                    lin.bias.uniform_(-0.3, 0.3)
    return m


def gumbel_actions(logits, u):
    g = -torch.log(-torch.log(u))
    z = logits + g
    return torch.stack([z[..., :2].argmax(-1), z[..., 2:].argmax(-1)], -1).to(torch.int8)


def _policy_vs_torch_and_oracle(ea, N, lo, hi, K, launches, S=5, layout="record", want_value=True, deterministic=False, autoreset=True, **kw):
    okw = dict(kw)
    opp = okw.pop("opponent_policy")
    env = ea.VecEWN(N, board_size=S, opponent_policy=opp, autoreset=autoreset, seed_stride=N, rng="philox", **okw)
    assert env.supports_policy_rollout()
    seeds = (np.arange(N, dtype=np.uint64) * 5 + 77).astype(np.uint32)
    env.reset(seeds=seeds)
    orc = po.OracleVecEnv(hi - lo, board_size=S, opponent=opp, autoreset=autoreset, seed_stride=N, lane_offset=lo, rng="philox", **okw)
    ob, od = orc.reset(seeds=seeds[lo:hi])
    model = make_model(S, 5)
    params = model.flat_parameters()
    assert params.numel() == env.policy_param_count()
    rec = layout == "record"
    traj = env.alloc_rollout(K, layout=layout, initial_obs=rec)
    totals = env.alloc_totals()
    logits = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    value = torch.zeros((K, N), dtype=torch.float32, device="cuda") if want_value else None
    noise = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    frozen = np.zeros(hi - lo, bool)
    nep, flips, total = 0, 0, 0
    counts = np.zeros(5)
    probs = np.zeros(5)
    for launch in range(launches):
        b0, d0 = env.board.clone(), env.dice.clone()
        env.rollout_policy(K, params, traj=traj, totals=totals, deterministic=deterministic, noise_key=99, logits=logits, value=value, noise=noise)
        torch.cuda.synchronize()
        for k in range(K):
            # the observation the policy saw at step k: the state before the launch, then the previous step's row
            if rec:
                bo, di = traj["obs_board"][k], traj["obs_dice"][k]
                if k == 0:
                    assert torch.equal(bo, b0) and torch.equal(di, d0)
            else:
                bo, di = (b0, d0) if k == 0 else (traj["board"][k - 1], traj["dice"][k - 1])
            with torch.no_grad():
                l0, l1, v = model(bo, di)
            ref = torch.cat([l0, l1], 1)
            assert torch.allclose(logits[k], ref, atol=1e-5, rtol=0), (launch, k, float((logits[k] - ref).abs().max()))
            if want_value:
                assert torch.allclose(value[k], v, atol=1e-5, rtol=0), (launch, k, float((value[k] - v).abs().max()))
            # the noise is the engine's hash stream at that step, the action its Gumbel-max (argmax when deterministic)
            assert np.array_equal(cpu(noise[k, lo:hi]), orc.policy_noise(99)), (launch, k)
            act = traj["action"][k]
            if deterministic:
                exp = torch.stack([logits[k][:, :2].argmax(1), logits[k][:, 2:].argmax(1)], 1).to(torch.int8)
                assert torch.equal(act, exp)
            else:
                exp = gumbel_actions(logits[k], noise[k])
                bad = int((act != exp).any(1).sum())
                flips += bad
                total += N
                a = cpu(act.to(torch.int64))
                p = cpu(torch.cat([torch.softmax(logits[k][:, :2], 1), torch.softmax(logits[k][:, 2:], 1)], 1).double())
                counts += np.array([(a[:, 0] == 0).sum(), (a[:, 0] == 1).sum(), (a[:, 1] == 0).sum(), (a[:, 1] == 1).sum(), (a[:, 1] == 2).sum()])
                probs += p.sum(0)
            # every transition against the oracle, the recorded action fed in
            acts = cpu(act[lo:hi])
            live = ~frozen
            ob, od, r, te, tr, info = orc.step(np.where(live[:, None], acts, 0).astype(np.int8))
            ctx = (kw, launch, k)
            assert np.array_equal(cpu(traj["board"][k, lo:hi]), ob), ctx
            assert np.array_equal(cpu(traj["dice"][k, lo:hi]), od), ctx
            assert np.array_equal(bits(cpu(traj["reward"][k, lo:hi])), bits(r)), ctx
            assert np.array_equal(cpu(traj["terminated"][k, lo:hi]), te) and np.array_equal(cpu(traj["truncated"][k, lo:hi]), tr), ctx
            assert np.array_equal(cpu(traj["info"][k, lo:hi]), info), ctx
            nep += int((live & (te != 0)).sum())
            if not autoreset:
                frozen |= te != 0
        assert np.array_equal(cpu(env.board[lo:hi]), ob) and np.array_equal(cpu(env.dice[lo:hi]), od)
        assert np.array_equal(cpu(env.done[lo:hi]) != 0, frozen)
        if kw.get("shaped"):
            ps, tol, _ = orc.aux()
            assert np.array_equal(bits(cpu(env.prev_score[lo:hi])), bits(ps)) and np.array_equal(cpu(env.tolerance[lo:hi]), tol)
    if not deterministic:
        assert flips <= max(2, total // 20000), (flips, total)     # only near-ties of fp32 log rounding may differ
        chi2 = float((((counts - probs) ** 2) / np.maximum(probs, 1)).sum())
        assert chi2 < 40.0, (chi2, counts, probs)                   # 3 degrees of freedom; a policy that ignored its logits is off by thousands
    return nep


def test_policy_rollout_shaped_env_minimax_opponent(ea):
    """config 4's collector: MiniMaxHeuristicEnv semantics (shaped reward, tolerance), depth-3 minimax opponent, records with the
    initial observation, value requested; 3 000 games = 11 full blocks of 256 and a partial one"""
    kw = dict(opponent_policy="minimax", max_depth=3, shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=4,
              shaped_refresh_on_reset=True, philox_key=9487)
    assert _policy_vs_torch_and_oracle(ea, 3000, 2600, 3000, 6, 3, **kw) > 100


@pytest.mark.parametrize("kw", [
    dict(opponent_policy="random"), dict(opponent_policy="minimax", max_depth=1), dict(opponent_policy="minimax", max_depth=4, heuristic="attk"),
    dict(opponent_policy="minimax", max_depth=2, shaped=True, reward=10.0, illegal_move_tolerance=10, shaped_refresh_on_reset=False),
], ids=lambda kw: "-".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_policy_rollout_other_opponents(ea, kw):
    _policy_vs_torch_and_oracle(ea, 700, 100, 500, 5, 2, philox_key=3, **kw)


def test_policy_rollout_columns_no_value_deterministic_and_frozen_lanes(ea):
    _policy_vs_torch_and_oracle(ea, 600, 0, 300, 5, 2, layout="columns", want_value=False, opponent_policy="minimax", max_depth=3, philox_key=8)
    _policy_vs_torch_and_oracle(ea, 600, 200, 600, 6, 2, deterministic=True, opponent_policy="minimax", max_depth=3, philox_key=9)
    _policy_vs_torch_and_oracle(ea, 520, 0, 520, 9, 3, autoreset=False, opponent_policy="minimax", max_depth=3, philox_key=10)


def test_policy_rollout_7x7(ea):
    _policy_vs_torch_and_oracle(ea, 400, 100, 400, 5, 2, S=7, opponent_policy="minimax", max_depth=3, philox_key=12)
    _policy_vs_torch_and_oracle(ea, 400, 0, 200, 4, 2, S=7, opponent_policy="random", shaped=True, reward=10.0, philox_key=13)


def test_policy_rollout_at_config4_shape(ea):
    """65 536 lanes, shaped env, depth-3 opponent: a slice against torch and the oracle"""
    kw = dict(opponent_policy="minimax", max_depth=3, shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10,
              shaped_refresh_on_reset=True, philox_key=9487)
    _policy_vs_torch_and_oracle(ea, 65536, 65236, 65536, 5, 2, **kw)


def _f64_bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("N", [3000, 65536])
def test_trainer_instance_matches_the_generic_instance(ea, N):
    """FusedA2CTrainer's call (records from the initial observation on + the reward column, nothing else, sampled actions) runs its own
    kernel instance, k_rollout_mlp<S, 0, NT, 1>, which the tests above never reach (they ask for logits and noise).  From the same saved
    state and with the same noise key it must play exactly what the generic instance plays: records, rewards, end state, prev_score and
    tolerance bit-identical (no flip budget needed: both instances run the same arithmetic).  Its actions against the Gumbel-max of the
    generic run's logits and noise (torch's log against the device's: the near-tie budget of _policy_vs_torch_and_oracle), and a 96-lane
    slice of it replayed on the oracle, whose policy noise must equal the generic run's."""
    K, lo, hi, key = 5, N - 96, N, 99
    kw = dict(max_depth=3, shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10, shaped_refresh_on_reset=True,
              philox_key=9487)
    env = ea.VecEWN(N, opponent_policy="minimax", rng="philox", autoreset=True, seed_stride=N, **kw)
    seeds = (np.arange(N, dtype=np.uint64) * 3 + 41).astype(np.uint32)
    env.reset(seeds=seeds)
    orc = po.OracleVecEnv(hi - lo, opponent="minimax", rng="philox", autoreset=True, seed_stride=N, lane_offset=lo, **kw)
    orc.reset(seeds=seeds[lo:hi])
    params = make_model(5, 17).flat_parameters()
    # a few launches first (mid-game state: finished episodes, tolerance counters), their actions fed to the oracle slice
    pre = env.alloc_rollout(6, layout="record")
    for _ in range(3):
        env.rollout_policy(6, params, traj=pre, noise_key=3)
        for k in range(6):
            orc.step(cpu(pre["action"][k, lo:hi]))
    assert np.array_equal(cpu(env.board[lo:hi]), orc.obs()[0])
    sd = env.state_dict()
    gen = env.alloc_rollout(K, layout="record", initial_obs=True)
    logits = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    noise = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    env.rollout_policy(K, params, traj=gen, noise_key=key, logits=logits, noise=noise)        # the generic instance (TRJ = 0)
    end_gen = env.state_dict()
    env.load_state_dict(sd)
    trn = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, params, traj=trn, noise_key=key)                                     # the trainer's instance (TRJ = 1)
    end_trn = env.state_dict()
    torch.cuda.synchronize()
    assert torch.equal(gen["record"], trn["record"])
    assert _f64_bits_equal(gen["reward"], trn["reward"])
    for name in ("board", "dice", "done", "rng_state", "tolerance"):
        assert torch.equal(end_gen[name], end_trn[name]), name
    assert _f64_bits_equal(end_gen["prev_score"], end_trn["prev_score"])
    # the trainer's actions are the Gumbel-max of the generic run's logits and noise
    exp = gumbel_actions(logits, noise)
    flips = int((trn["action"] != exp).any(-1).sum())
    assert flips <= max(2, K * N // 20000), (flips, K * N)
    # the oracle slice: the same noise stream, the same transitions
    for k in range(K):
        assert np.array_equal(cpu(noise[k, lo:hi]), orc.policy_noise(key)), k
        ob, od, r, te, tr, info = orc.step(cpu(trn["action"][k, lo:hi]))
        assert np.array_equal(cpu(trn["board"][k, lo:hi]), ob) and np.array_equal(cpu(trn["dice"][k, lo:hi]), od), k
        assert np.array_equal(bits(cpu(trn["reward"][k, lo:hi])), bits(r)), k
        assert np.array_equal(cpu(trn["terminated"][k, lo:hi]), te) and np.array_equal(cpu(trn["truncated"][k, lo:hi]), tr), k
        assert np.array_equal(cpu(trn["info"][k, lo:hi]), info), k
    ps, tol, _ = orc.aux()
    assert np.array_equal(bits(cpu(env.prev_score[lo:hi])), bits(ps)) and np.array_equal(cpu(env.tolerance[lo:hi]), tol)


def test_rollout_policy_rejects_malformed_buffers(ea):
    """logits / noise must be contiguous float32 [>= K, N, 5], value [>= K, N], column trajectories [>= K, N, ...] and contiguous: each
    violation raises ValueError before anything is launched (the state is untouched)"""
    N, K = 300, 4
    env = ea.VecEWN(N, opponent_policy="minimax", max_depth=3, rng="philox", autoreset=True, philox_key=4)
    env.reset(seeds=np.arange(N) + 1)
    params = make_model(5, 3).flat_parameters()
    f32 = dict(dtype=torch.float32, device="cuda")
    good = dict(logits=torch.zeros((K, N, 5), **f32), value=torch.zeros((K, N), **f32), noise=torch.zeros((K, N, 5), **f32))
    bad = {
        "logits": [torch.zeros((K - 1, N, 5), **f32), torch.zeros((K, N - 1, 5), **f32), torch.zeros((K, N, 4), **f32),
                   torch.zeros((K, N * 5), **f32), torch.zeros((K, N, 5), dtype=torch.float64, device="cuda"),
                   torch.zeros((K, 5, N), **f32).transpose(1, 2), torch.zeros((K, N, 5))],
        "value": [torch.zeros((K - 1, N), **f32), torch.zeros((K, N + 1), **f32), torch.zeros((K, N, 1), **f32),
                  torch.zeros((K, N), dtype=torch.float16, device="cuda"), torch.zeros((N, K), **f32).t()],
        "noise": [torch.zeros((K - 1, N, 5), **f32), torch.zeros((K, N, 6), **f32), torch.zeros((K, N, 5), dtype=torch.int32, device="cuda")],
    }
    before = env.state_dict()
    for name, cases in bad.items():
        for t in cases:
            kw = dict(good)
            kw[name] = t
            with pytest.raises(ValueError, match=name):
                env.rollout_policy(K, params, **kw)
    cols = env.alloc_rollout(K)
    for name in ("board", "dice", "action", "reward", "terminated", "truncated", "info"):
        short = dict(cols)
        short[name] = cols[name][:K - 1]
        with pytest.raises(ValueError, match=name):
            env.rollout_policy(K, params, traj=short)
        narrow = dict(cols)
        narrow[name] = cols[name][:, :N - 1]
        with pytest.raises(ValueError, match=name):
            env.rollout_policy(K, params, traj=narrow)
    strided = dict(cols)
    strided["dice"] = torch.zeros((N, K), dtype=torch.int8, device="cuda").t()
    with pytest.raises(ValueError, match="dice"):
        env.rollout_policy(K, params, traj=strided)
    rec = env.alloc_rollout(K, layout="record", initial_obs=True)
    rec["reward"] = rec["reward"][:K - 1]
    with pytest.raises(ValueError, match="reward"):
        env.rollout_policy(K, params, traj=rec)
    torch.cuda.synchronize()
    after = env.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # the well-formed call still runs, and over-long buffers (first dimension > K) stay allowed
    env.rollout_policy(K, params, traj=env.alloc_rollout(K + 2), logits=torch.zeros((K + 1, N, 5), **f32), noise_key=1)
    torch.cuda.synchronize()


def test_rollout_refuses_a_trajectory_allocated_for_rollout_policy(ea):
    """ewn_step_k has no initial-observation row: a record trajectory allocated with initial_obs=True (K + 1 rows, the step views from
    row 1 on) would read back one step late through rollout() / bind_rollout(); both refuse it.  A plain record trajectory through
    rollout() still agrees with the columns layout."""
    N, K = 500, 6
    kw = dict(opponent_policy="minimax", max_depth=3, rng="philox", autoreset=True, philox_key=6, seed_stride=N)
    env = ea.VecEWN(N, **kw)
    env.reset(seeds=np.arange(N) + 8)
    bad = env.alloc_rollout(K, layout="record", initial_obs=True)
    before = env.state_dict()
    with pytest.raises(ValueError, match="initial_obs"):
        env.rollout(K, traj=bad)
    with pytest.raises(ValueError, match="initial_obs"):
        env.bind_rollout(K, traj=bad)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in env.state_dict().items())
    env2 = ea.VecEWN(N, **kw)
    env2.reset(seeds=np.arange(N) + 8)
    rec, cols = env.alloc_rollout(K, layout="record"), env2.alloc_rollout(K)
    for _ in range(2):
        env.rollout(K, traj=rec)
        env2.rollout(K, traj=cols)
        torch.cuda.synchronize()
        for name in ("board", "dice", "action", "terminated", "truncated", "info"):
            assert torch.equal(rec[name], cols[name]), name
        assert _f64_bits_equal(rec["reward"], cols["reward"])
    assert torch.equal(env.board, env2.board) and torch.equal(env.dice, env2.dice)


def test_policy_rollout_is_unsupported_where_documented(ea):
    env = ea.VecEWN(64, opponent_policy="minimax", max_depth=5, rng="philox")
    assert not env.supports_policy_rollout()
    env = ea.VecEWN(64, opponent_policy="minimax", max_depth=3, rng="mt19937")
    assert not env.supports_policy_rollout()
    env = ea.VecEWN(64, board_size=6, opponent_policy="random", rng="philox")
    assert not env.supports_policy_rollout()
