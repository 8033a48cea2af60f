"""ewn_predict_policy: the trained actor-critic as a stateless batched policy (predict_policy, classical_policies.ModelAgent).  Its
network against a plain fp32 torch forward; against the rollout kernel's recorded outputs bit for bit; the grid-stride tile loop against
chunked calls; the hashed sampling; exact guard zones around every output; and ModelAgent through the drop-in env and the tournament."""
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


def bits(t):
    return t.contiguous().view(torch.int32)


def first_argmax_actions(logits):
    return torch.stack([logits[:, :2].argmax(1), logits[:, 2:].argmax(1)], 1).to(torch.int8)


_POOL = {}


def pool(ea, S):
    """per board size, computed once and left unchanged: a model, its flat parameters, 45 056 observations of real play (the start
    position of 4 096 games and every observation of a 10-step random-agent rollout of them) and, for the first 300, the torch forward"""
    if S not in _POOL:
        N, K = 4096, 10
        env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=31 + S)
        b0, d0 = env.reset(seeds=(np.arange(N, dtype=np.uint64) * 3 + 11).astype(np.uint32))
        b0, d0 = b0.clone(), d0.clone()
        traj = env.alloc_rollout(K)
        env.rollout(K, agent="random", traj=traj)
        boards = torch.cat([b0[None], traj["board"]]).reshape(-1, S, S).contiguous()
        dice = torch.cat([d0[None], traj["dice"]]).reshape(-1).contiguous()
        perm = torch.randperm(boards.shape[0], generator=torch.Generator().manual_seed(S)).cuda()   # mix start, middle and end games
        boards, dice = boards[perm].contiguous(), dice[perm].contiguous()
        assert int(dice.min()) >= 1 and int(dice.max()) <= 6 and bool((boards[:300] != boards[0]).any())
        model = make_model(S, 5)
        with torch.no_grad():
            l0, l1, v = model(boards[:300], dice[:300])
        _POOL[S] = dict(model=model, params=model.flat_parameters(), boards=boards, dice=dice, ref_logits=torch.cat([l0, l1], 1), ref_value=v)
    return _POOL[S]


# ---------------------------------------------------------------- 1. against torch

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [1, 31, 33, 129, 300])   # a lone sample, a partial wave, one past a wave, one past a block, several blocks
def test_against_torch(ea, S, M):
    p = pool(ea, S)
    b, d = p["boards"][:M], p["dice"][:M]
    act, logits, value = ea.predict_policy(b, d, p["params"], return_logits=True, return_value=True)
    assert act.shape == (M, 2) and act.dtype == torch.int8 and logits.shape == (M, 5) and value.shape == (M,)
    el, ev = float((logits - p["ref_logits"][:M]).abs().max()), float((value - p["ref_value"][:M]).abs().max())
    print("S=%d M=%d: max |logits - torch| %.3g, max |value - torch| %.3g" % (S, M, el, ev))
    assert torch.allclose(logits, p["ref_logits"][:M], atol=1e-5, rtol=0), el
    assert torch.allclose(value, p["ref_value"][:M], atol=1e-5, rtol=0), ev
    assert torch.equal(act, first_argmax_actions(logits))           # the first-index argmax of the RETURNED logits, exactly
    # without the value (the other kernel instance: one weight image): the same bits
    act2, logits2 = ea.predict_policy(b, d, p["params"], return_logits=True)
    assert torch.equal(bits(logits2), bits(logits)) and torch.equal(act2, act)
    assert torch.equal(ea.predict_policy(b, d, p["params"]), act)
    if M == 1:                                                        # a single [S, S] board, as predict_minimax takes it
        assert torch.equal(ea.predict_policy(b[0], d, p["params"]), act)


# ---------------------------------------------------------------- 2. against the rollout kernel, bit for bit

@pytest.mark.parametrize("S", [5, 7])
def test_replays_a_recorded_rollout_bit_for_bit(ea, S):
    N, K = 300, 4
    p = pool(ea, S)
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=5)
    assert env.supports_policy_rollout()
    env.reset(seeds=(np.arange(N, dtype=np.uint64) * 5 + 77).astype(np.uint32))
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    logits = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    value = torch.zeros((K, N), dtype=torch.float32, device="cuda")
    noise = torch.zeros((K, N, 5), dtype=torch.float32, device="cuda")
    env.rollout_policy(K, p["params"], traj=traj, deterministic=False, noise_key=99, logits=logits, value=value, noise=noise)
    for k in range(K):
        # the record's observation columns are strided views of the 32 / 64-byte records: the kernel reads packed boards
        bo, di = traj["obs_board"][k].contiguous(), traj["obs_dice"][k].contiguous()
        act, lg, val = ea.predict_policy(bo, di, p["params"], deterministic=False, uniforms=noise[k], return_logits=True, return_value=True)
        nl, nv = int((bits(lg) != bits(logits[k])).sum()), int((bits(val) != bits(value[k])).sum())
        print("S=%d step %d: %d logits and %d values differ by bit pattern, max |d| %.3g" % (S, k, nl, nv, float((lg - logits[k]).abs().max())))
        assert nl == 0 and nv == 0, (k, nl, nv)
        assert torch.equal(act, traj["action"][k]), k
    assert int((traj["action"][:K] != first_argmax_actions(logits.reshape(-1, 5)).reshape(K, N, 2)).any(-1).sum()) > 0   # the noise mattered


# ---------------------------------------------------------------- 3. the grid-stride tile loop

def test_grid_stride_loop_equals_chunked_calls(ea):
    M, chunk = 40000, 4096                      # 1 250 tiles: more than 256 blocks x 4 waves, so blocks take a second trip, some waves without a tile
    p = pool(ea, 5)
    b, d = p["boards"][:M], p["dice"][:M]
    act, logits, value = ea.predict_policy(b, d, p["params"], return_logits=True, return_value=True)
    parts = [ea.predict_policy(b[i:i + chunk], d[i:i + chunk], p["params"], return_logits=True, return_value=True) for i in range(0, M, chunk)]
    assert torch.equal(bits(logits), bits(torch.cat([x[1] for x in parts])))
    assert torch.equal(bits(value), bits(torch.cat([x[2] for x in parts])))
    assert torch.equal(act, torch.cat([x[0] for x in parts]))
    assert torch.allclose(logits[:300], p["ref_logits"], atol=1e-5, rtol=0)
    M2 = 40000 - 7                              # ... and with a partial last tile
    l2 = ea.predict_policy(b[:M2], d[:M2], p["params"], return_logits=True)[1]
    assert torch.equal(bits(l2), bits(logits[:M2]))


# ---------------------------------------------------------------- 4. hashed sampling

def test_hashed_sampling(ea):
    M = 40000
    p = pool(ea, 5)
    b, d, params = p["boards"][:M], p["dice"][:M], p["params"]
    ids = torch.randperm(1 << 20, generator=torch.Generator().manual_seed(1))[:M].to(torch.int32).cuda()
    a1, logits = ea.predict_policy(b, d, params, deterministic=False, key=7, obs_id=ids, return_logits=True)
    a2 = ea.predict_policy(b, d, params, deterministic=False, key=7, obs_id=ids)
    assert torch.equal(a1, a2)                                        # the same (key, obs_id): the same actions
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(2)).cuda()
    a3 = ea.predict_policy(b[perm].contiguous(), d[perm].contiguous(), params, deterministic=False, key=7, obs_id=ids[perm].contiguous())
    assert torch.equal(a3, a1[perm])                                  # the noise belongs to the id, not to the row
    a4 = ea.predict_policy(b, d, params, deterministic=False, key=8, obs_id=ids)
    assert int((a4 != a1).any(1).sum()) > 0                           # another key: other noise
    # obs_id None is the row index
    a5 = ea.predict_policy(b, d, params, deterministic=False, key=7)
    a6 = ea.predict_policy(b, d, params, deterministic=False, key=7, obs_id=torch.arange(M, dtype=torch.int32, device="cuda"))
    assert torch.equal(a5, a6) and not torch.equal(a5, a1)
    # the key's upper half is part of the hash
    assert not torch.equal(ea.predict_policy(b, d, params, deterministic=False, key=7 + (1 << 32)), a5)
    # 2 x 10^5 samples against the summed softmax probabilities of the returned logits: the statistic and bound of test_gpu_policy.py
    pr = torch.cat([torch.softmax(logits[:, :2], 1), torch.softmax(logits[:, 2:], 1)], 1).double().sum(0).cpu().numpy()
    counts, probs = np.zeros(5), np.zeros(5)
    for key in (101, 102, 103, 104, 105):
        a = ea.predict_policy(b, d, params, deterministic=False, key=key).to(torch.int64).cpu().numpy()
        counts += np.array([(a[:, 0] == 0).sum(), (a[:, 0] == 1).sum(), (a[:, 1] == 0).sum(), (a[:, 1] == 1).sum(), (a[:, 1] == 2).sum()])
        probs += pr
    chi2 = float((((counts - probs) ** 2) / np.maximum(probs, 1)).sum())
    print("chi2 %.3f, counts %s, expected %s" % (chi2, counts, probs))
    assert chi2 < 40.0, (chi2, counts, probs)


# ---------------------------------------------------------------- 5. guard zones

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("M", [33, 129])
@pytest.mark.parametrize("offset", [0, 4, 1])    # boards 16-byte aligned, dword aligned, byte aligned: the three staging paths
def test_guard_zones(ea, S, M, offset):
    p = pool(ea, S)
    alloc = GuardedAllocator()
    # the inputs end exactly where their buffers end (4 KB of 0xA5 follow, inside the same allocation: a read past the end faults nothing)
    b = alloc.zeros((M, S, S), dtype=torch.int8, tag="boards", offset=offset)
    d = alloc.zeros((M,), dtype=torch.int8, tag="dice", offset=offset)
    u = alloc.zeros((M, 5), dtype=torch.float32, tag="uniforms")
    ids = alloc.zeros((M,), dtype=torch.int32, tag="obs_id")
    params = alloc.zeros((p["params"].numel(),), dtype=torch.float32, tag="params")
    b.copy_(p["boards"][:M]); d.copy_(p["dice"][:M]); params.copy_(p["params"])
    u.copy_(torch.rand((M, 5), generator=torch.Generator().manual_seed(M)).clamp_(1e-6, 1 - 1e-6))
    ids.copy_(torch.arange(M, dtype=torch.int32) * 7 + 3)
    ref = ea.predict_policy(p["boards"][:M], p["dice"][:M], p["params"], return_logits=True, return_value=True)
    refu = ea.predict_policy(p["boards"][:M], p["dice"][:M], p["params"], deterministic=False, uniforms=u.clone(), return_logits=True)
    refh = ea.predict_policy(p["boards"][:M], p["dice"][:M], p["params"], deterministic=False, key=3, obs_id=ids.clone())
    with alloc.patch(tag="outputs"):            # predict_policy's torch.zeros outputs come out of the guarded allocator
        act, logits, value = ea.predict_policy(b, d, params, return_logits=True, return_value=True)
        act1 = ea.predict_policy(b, d, params)
        actu, logitsu = ea.predict_policy(b, d, params, deterministic=False, uniforms=u, return_logits=True)
        acth = ea.predict_policy(b, d, params, deterministic=False, key=3, obs_id=ids)
    assert all(alloc.owns(t) for t in (act, logits, value, act1, actu, logitsu, acth))
    torch.cuda.synchronize()
    alloc.check("S=%d M=%d offset=%d" % (S, M, offset))
    assert torch.equal(act, ref[0]) and torch.equal(bits(logits), bits(ref[1])) and torch.equal(bits(value), bits(ref[2]))
    assert torch.equal(act1, ref[0]) and torch.equal(actu, refu[0]) and torch.equal(bits(logitsu), bits(refu[1])) and torch.equal(acth, refh)


# ---------------------------------------------------------------- 6. ModelAgent

def test_model_agent_predict_on_the_drop_in_env(ea):
    from classical_policies import ModelAgent
    from envs import EinsteinWuerfeltNichtEnv
    p = pool(ea, 5)
    agent = ModelAgent(p["model"], board_size=5)
    assert torch.equal(agent.params, p["params"])
    env = EinsteinWuerfeltNichtEnv(board_size=5, seed=3)
    obs, _ = env.reset(seed=3)
    for _ in range(6):
        action, state = agent.predict(obs)
        assert state is None and isinstance(action, np.ndarray) and action.shape == (2,)
        batch = agent.predict_batch(obs["board"].astype(np.int8)[None], [obs["dice_roll"]])
        assert np.array_equal(action, batch[0].cpu().numpy())
        with torch.no_grad():
            exp = p["model"].act(torch.as_tensor(obs["board"].astype(np.int8))[None].cuda(), torch.tensor([obs["dice_roll"]], dtype=torch.int8).cuda(),
                                 deterministic=True)[0]
        assert np.array_equal(action, exp[0].cpu().numpy())          # this model's logits are spread: no near-tie on six observations
        obs, _, terminated, truncated, _ = env.step(action)
        if terminated or truncated:
            break
    # a flat parameter vector is a model too; a sampling agent draws other noise per call and per step, the same for the same step
    sampler = ModelAgent(p["params"], board_size=5, deterministic=False, key=9)
    b, d = p["boards"][:4096], p["dice"][:4096]
    f = sampler.policy_fn()
    assert torch.equal(f(b, d, 3), f(b, d, 3)) and not torch.equal(f(b, d, 3), f(b, d, 4))
    assert not torch.equal(sampler.predict_batch(b, d), sampler.predict_batch(b, d))
    assert torch.equal(f(b, d, 0), ea.predict_policy(b, d, p["params"], deterministic=False, key=(9 + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF))


def test_model_agent_in_the_tournament_equals_the_engine_evaluation(ea):
    from classical_policies import ModelAgent
    from ewn_gym_amd.tournament import _policy, evaluate
    p = pool(ea, 5)
    m = p["model"]
    step = evaluate(ModelAgent(m).policy_fn(), {"kind": "random"}, num=64, use_rollout=False)
    eng = evaluate({"kind": "mlp", "model": m}, {"kind": "random"}, num=64)
    assert step["engine"] == "ewn_step" and eng["engine"] == "ewn_policy_eval"
    assert torch.equal(step["scores"], eng["scores"]) and torch.equal(step["lengths"], eng["lengths"])
    # the "mlp" kind of tournament._policy is the same callable
    f = _policy({"kind": "mlp", "model": m}, 3, 12345)
    assert torch.equal(f(p["boards"][:300], p["dice"][:300], 0), ea.predict_policy(p["boards"][:300], p["dice"][:300], p["params"]))


def test_model_agent_from_a_fused_trainer_checkpoint(ea, tmp_path):
    from classical_policies import ModelAgent
    from ewn_gym_amd.a2c import FusedA2CTrainer
    N = 256
    env = ea.VecEWN(N, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=9487)
    env.reset(seeds=torch.arange(N, dtype=torch.int32))
    tr = FusedA2CTrainer(env, n_steps=5, learning_rate=7e-4, seed=1, use_graph=False)
    path = str(tmp_path / "best.pt")
    tr.save(path)
    agent = ModelAgent(path, board_size=5)
    assert torch.equal(agent.params, tr.params)
    p = pool(ea, 5)
    b, d = p["boards"][:300], p["dice"][:300]
    act = agent.predict_batch(b, d)
    assert torch.equal(act, ea.predict_policy(b, d, tr.params))
    obs = {"board": b[0].cpu().numpy().astype(np.int16), "dice_roll": int(d[0])}
    assert np.array_equal(agent.predict(obs)[0], act[0].cpu().numpy())
    with pytest.raises(ValueError):
        ModelAgent(path, board_size=7)
    with pytest.raises(ValueError):
        ModelAgent(tr.model, board_size=7)
