"""A trained policy as the env's opponent for any agent (ewn_step_vs, ewn_step_k_vs).

Three kinds of evidence.  (1) The same step as the kernels that already play this opponent: twin envs from the same seeds, one stepped by
ewn_policy_eval_vs / ewn_step_k_selfplay (K = 1), the other by step() with the recorded agent actions, everything torch.equal after every
step.  (2) An independent replay of step() under outside actions (illegal and out-of-range ones included) with the stateless public calls
and fp32 torch forwards of the opponent, as tests/test_gpu_selfplay.py replays the self-play kernels.  (3) The K-step call against K
step() calls with the recorded actions fed back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.guarded_alloc import GuardedAllocator  # noqa: E402
from tests.test_gpu_selfplay import INFO_INVALID_PLAYER, Tally, f64_bits, finish, make_model, replay_step  # noqa: E402


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def _state_equal(a, b, ctx, shaped=False):
    for name in ("board", "dice", "done", "rng_state"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (ctx, name)
    if shaped:
        assert torch.equal(a.tolerance, b.tolerance), (ctx, "tolerance")
        assert torch.equal(f64_bits(a.prev_score), f64_bits(b.prev_score)), (ctx, "prev_score")


# ---------------------------------------------------------------- (1) the same step as the existing kernels

@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("S,N", [(5, 257), (5, 3000), (7, 257), (7, 3000)])
def test_step_is_the_evaluation_kernels_step(ea, S, N, rng):
    """env A: ewn_policy_eval_vs one step per launch; env B: step() with A's recorded agent actions.  257 lanes end in a partial wave."""
    kw = dict(board_size=S, opponent_policy="random", rng=rng, autoreset=False, philox_key=13)
    A, Bv = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    seeds = torch.as_tensor(np.arange(N, dtype=np.int64) * 7 + 3).to(torch.int32)
    A.reset(seeds=seeds)
    Bv.reset(seeds=seeds)
    pa, po = make_model(S, 5).flat_parameters(), make_model(S, 9).flat_parameters()
    ocb = torch.zeros((N, 3), dtype=torch.int8, device="cuda")
    Bv.set_opponent_model(po, opponent_action=ocb)
    totals = A.alloc_totals()
    opp_moves = 0
    for step in range(12):
        live = A.done == 0
        before = totals["return_sum"].clone()
        act = torch.zeros((1, N, 2), dtype=torch.int8, device="cuda")
        oca = torch.zeros((1, N, 3), dtype=torch.int8, device="cuda")
        A.eval_policy(1, pa, totals, action=act, opponent_params=po, opponent_action=oca)
        _, _, reward, term, _, _ = Bv.step(act[0])
        torch.cuda.synchronize()
        ctx = (S, N, rng, step)
        _state_equal(A, Bv, ctx)
        assert torch.equal(oca[0], ocb), ctx
        assert torch.equal(f64_bits(torch.where(live, reward, torch.zeros_like(reward))), f64_bits(totals["return_sum"] - before)), ctx
        assert torch.equal(term != 0, A.done != 0), ctx
        opp_moves += int((ocb[:, 0] != 0).sum())
    assert opp_moves > N // 4 and bool((A.done != 0).any())


@pytest.mark.parametrize("S,N", [(5, 257), (5, 3000), (7, 257), (7, 3000)])
def test_step_is_the_selfplay_kernels_step_shaped_autoreset_sampling(ea, S, N):
    """env A: ewn_step_k_selfplay, K = 1, shaped env with tolerance 4, auto-reset, a SAMPLING opponent; env B: step().  The opponent's
    noise word depends on the tolerance left and on the stream position before the step: both kernels must agree bit for bit."""
    kw = dict(board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=31, shaped=True, reward=10.0,
              illegal_move_reward=-1.0, illegal_move_tolerance=4, shaped_refresh_on_reset=True)
    A, Bv = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    seeds = (np.arange(N, dtype=np.uint64) * 3 + 11).astype(np.uint32)
    A.reset(seeds=seeds)
    Bv.reset(seeds=seeds)
    pa, po = make_model(S, 5).flat_parameters(), make_model(S, 9).flat_parameters()
    ocb = torch.zeros((N, 3), dtype=torch.int8, device="cuda")
    Bv.set_opponent_model(po, deterministic=False, noise_key=77, opponent_action=ocb)
    traj = A.alloc_rollout(1)
    oca = torch.zeros((1, N, 3), dtype=torch.int8, device="cuda")
    infos = np.zeros(6, dtype=np.int64)
    for step in range(12):
        A.rollout_policy(1, pa, traj=traj, noise_key=3, opponent_params=po, opponent_deterministic=False, opponent_noise_key=77,
                         opponent_action=oca)
        _, _, reward, term, trunc, info = Bv.step(traj["action"][0])
        torch.cuda.synchronize()
        ctx = (S, N, step)
        _state_equal(A, Bv, ctx, shaped=True)
        assert torch.equal(oca[0], ocb), ctx
        assert torch.equal(f64_bits(reward), f64_bits(traj["reward"][0])), ctx
        assert torch.equal(term, traj["terminated"][0]) and torch.equal(trunc, traj["truncated"][0]) and torch.equal(info, traj["info"][0]), ctx
        infos += np.bincount(info.cpu().numpy(), minlength=6)
    assert infos[2] > 0 and infos[4] > 0 and infos[5] > 0, infos       # won, lost, tolerance: resets and shaped rewards were compared


# ---------------------------------------------------------------- (2) independent replay under outside actions

@pytest.mark.parametrize("S,N", [(5, 3000), (7, 3000), (5, 9000)])
def test_step_replayed_with_outside_actions_and_frozen_lanes(ea, S, N):
    """uniformly random [flag, dir] with dir in 0..3: legal moves, moves off the board / of a missing cube, and the direction-3 rule (an
    illegal move, as in ewn_step).  Every lane-step is replayed; the opponent's move must be its model's argmax (near-tie rule of
    tests/test_gpu_selfplay.py, unchanged).  9 000 lanes run the 256-thread blocks.  At the end the frozen lanes are held against a
    twin ewn_step env loaded with the same state."""
    env = ea.VecEWN(N, board_size=S, opponent_policy="minimax", max_depth=6, rng="philox", autoreset=False, philox_key=9, want_terminal_obs=True)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) * 5 + 1).astype(np.uint32))
    opp = make_model(S, 9)
    oc = torch.zeros((N, 3), dtype=torch.int8, device="cuda")
    env.set_opponent_model(opp.flat_parameters(), opponent_action=oc)
    g = torch.Generator(device="cuda").manual_seed(S * 1000 + N)
    tally = Tally()
    n_dir3 = n_inval = 0
    for step in range(10):
        live = env.done == 0
        bo, di = env.board.clone(), env.dice.clone()
        act = torch.stack([torch.randint(0, 2, (N,), generator=g, device="cuda"), torch.randint(0, 4, (N,), generator=g, device="cuda")], 1).to(torch.int8)
        _, _, reward, term, trunc, info = env.step(act)
        torch.cuda.synchronize()
        dir3 = live & (act[:, 1] == 3)
        r = replay_step(ea, opp, 1.0, bo, di, torch.stack([act[:, 0], act[:, 1].clamp(max=2)], 1).contiguous(), oc, live & ~dir3, tally)
        ctx = (S, N, step)
        exp_board = r.board                                        # a direction-3 lane is outside replay_step's `live`: board unchanged
        exp_reward = torch.where(dir3, torch.full_like(r.reward, -1.0), r.reward)
        exp_term = torch.where(dir3 | ~live, torch.ones_like(r.term), r.term)
        exp_trunc = torch.where(dir3, torch.ones_like(r.trunc), r.trunc)
        exp_info = torch.where(dir3, torch.full_like(r.info, INFO_INVALID_PLAYER), r.info)
        assert torch.equal(env.board, exp_board), ctx
        assert torch.equal(f64_bits(reward), f64_bits(exp_reward)), ctx
        assert torch.equal(term, exp_term) and torch.equal(trunc, exp_trunc) and torch.equal(info, exp_info), ctx
        assert torch.equal(env.done != 0, ~live | (exp_term != 0)), ctx
        assert torch.equal(env.dice[~r.cont], r.dice_fixed[~r.cont]), ctx
        assert bool(((env.dice >= 1) & (env.dice <= 6)).all()), ctx
        assert torch.equal(env.terminal_board, env.board) and torch.equal(env.terminal_dice, env.dice), ctx    # no auto-reset
        n_dir3 += int(dir3.sum())
        n_inval += int(r.inval.sum())
    print("step_vs replay S=%d N=%d: %d direction-3 actions, %d other illegal agent moves, near-tie share %.5f"
          % (S, N, n_dir3, n_inval, tally.excused / max(1, tally.played)))
    assert n_dir3 > 0 and n_inval > 0
    finish("step_vs replay S=%d N=%d" % (S, N), tally)             # asserts the EWN_INFO_INVALID_OPP path was taken
    # frozen lanes: what ewn_step does with them
    frozen = env.done != 0
    assert int(frozen.sum()) > N // 4
    twin = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=False, philox_key=9, want_terminal_obs=True)
    twin.load_state_dict({k: v for k, v in env.state_dict().items() if k != "scratch"})
    act = torch.stack([torch.randint(0, 2, (N,), generator=g, device="cuda"), torch.randint(0, 4, (N,), generator=g, device="cuda")], 1).to(torch.int8)
    env.step(act)
    twin.step(act)
    torch.cuda.synchronize()
    for name in ("board", "dice", "done", "rng_state", "terminal_board", "terminal_dice", "terminated", "truncated", "info"):
        assert torch.equal(getattr(env, name)[frozen], getattr(twin, name)[frozen]), name
    assert torch.equal(f64_bits(env.reward)[frozen], f64_bits(twin.reward)[frozen])
    assert bool((oc[frozen] == 0).all())


@pytest.mark.parametrize("S", [5, 7])
def test_mt19937_dice_are_numpys(ea, S):
    """dice_0, opponent dice_0, dice_1, ... of an episode is np.random.seed(seed) followed by consecutive np.random.randint(1, 7) draws:
    the policy opponent draws nothing"""
    from ewn_gym_amd import vec_env as ve
    N = 64
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="mt19937", autoreset=False)
    seeds = np.arange(N, dtype=np.int64) * 7 + 3
    env.reset(seeds=torch.as_tensor(seeds).to(torch.int32))
    opp = make_model(S, 9)
    oc = torch.zeros((N, 3), dtype=torch.int8, device="cuda")
    env.set_opponent_model(opp.flat_parameters(), opponent_action=oc)
    seq = [[int(d)] for d in env.dice.tolist()]
    tally = Tally()
    for step in range(200):
        live = env.done == 0
        if not bool(live.any()):
            break
        bo, di = env.board.clone(), env.dice.clone()
        act = ve.legal_actions(bo, di, player=1)[0][:, 0].clamp(min=0).contiguous()
        env.step(act)
        r = replay_step(ea, opp, 1.0, bo, di, act, oc, live, tally)
        assert torch.equal(env.board, r.board), (S, step)
        rep, cont, odl, ndl = r.replied.tolist(), r.cont.tolist(), oc[:, 0].tolist(), env.dice.tolist()
        for i in range(N):
            if rep[i]:
                seq[i].append(int(odl[i]))
            if cont[i]:
                seq[i].append(int(ndl[i]))
    assert bool((env.done != 0).all())
    env.check_rng()
    for i in range(N):
        np.random.seed(int(seeds[i]))
        exp = [int(np.random.randint(1, 7)) for _ in seq[i]]
        assert exp == seq[i], (i, exp, seq[i])
    assert max(len(s) for s in seq) > 8


# ---------------------------------------------------------------- (3) K steps per launch

KSTEP = [(5, 257, "random", 0), (5, 3000, "random", 0), (7, 257, "random", 0), (7, 3000, "random", 0),
         (5, 257, "sample", 0), (5, 3000, "sample", 0), (7, 257, "sample", 0), (7, 3000, "sample", 0),
         (5, 257, "minimax", 3), (5, 3000, "minimax", 3), (7, 257, "minimax", 3), (7, 3000, "minimax", 3),
         (5, 257, "minimax", 5), (7, 257, "minimax", 5)]


@pytest.mark.parametrize("S,N,agent,depth", KSTEP)
def test_k_steps_are_k_step_calls(ea, S, N, agent, depth):
    from ewn_gym_amd import vec_env as ve
    K, launches = 6, 2
    kw = dict(board_size=S, opponent_policy="mcts", rng="philox", autoreset=True, seed_stride=N, philox_key=21)   # its own opponent: not read
    A, R, Bv = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    seeds = (np.arange(N, dtype=np.uint64) * 3 + 5).astype(np.uint32)
    po = make_model(S, 9).flat_parameters()
    ocb = torch.zeros((N, 3), dtype=torch.int8, device="cuda")
    for e in (A, R, Bv):
        e.reset(seeds=seeds)
    A.set_opponent_model(po)
    R.set_opponent_model(po)
    Bv.set_opponent_model(po, opponent_action=ocb)
    assert A.supports_rollout(agent, depth)
    traj, rec = A.alloc_rollout(K), R.alloc_rollout(K, layout="record")
    totals, rtotals = A.alloc_totals(), R.alloc_totals()
    oca = torch.zeros((K, N, 3), dtype=torch.int8, device="cuda")
    if agent == "random":        # step 0 of the first launch: the action ewn_step_k's RandomAgent plays from the same reset state and key
        plain = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=21)
        plain.reset(seeds=seeds)
        ptraj = plain.alloc_rollout(1)
        plain.rollout(1, agent="random", traj=ptraj)
    exp = {k: torch.zeros_like(v) for k, v in totals.items()}
    for launch in range(launches):
        A.rollout(K, agent=agent, agent_max_depth=depth, traj=traj, totals=totals, opponent_action=oca)
        R.rollout(K, agent=agent, agent_max_depth=depth, traj=rec, totals=rtotals)
        torch.cuda.synchronize()
        if agent == "random" and launch == 0:
            assert torch.equal(traj["action"][0], ptraj["action"][0])
        for name in ("board", "dice", "action", "terminated", "truncated", "info"):
            assert torch.equal(rec[name], traj[name]), ("record layout", name)
        assert torch.equal(f64_bits(rec["reward"]), f64_bits(traj["reward"]))
        assert bool((rec["record"][:, :, S * S + 6:] == 0).all())
        for k in range(K):
            ctx = (S, N, agent, depth, launch, k)
            live = Bv.done == 0
            if agent == "minimax":
                want = ve.predict_minimax(Bv.board, Bv.dice, depth)[0]
                assert torch.equal(traj["action"][k], want), ctx
            _, _, reward, term, trunc, info = Bv.step(traj["action"][k])
            assert torch.equal(Bv.board, traj["board"][k]) and torch.equal(Bv.dice, traj["dice"][k]), ctx
            assert torch.equal(f64_bits(reward), f64_bits(traj["reward"][k])), ctx
            assert torch.equal(term, traj["terminated"][k]) and torch.equal(trunc, traj["truncated"][k]) and torch.equal(info, traj["info"][k]), ctx
            assert torch.equal(ocb, oca[k]), ctx
            exp["return_sum"] += reward
            exp["n_steps"] += live.to(torch.int32)
            exp["n_episodes"] += (term != 0).to(torch.int32)
            exp["n_wins"] += (info == 2).to(torch.int32)
        _state_equal(A, Bv, (S, N, agent, depth, launch))
        _state_equal(R, Bv, (S, N, agent, depth, launch, "record"))
    for name in exp:
        a, b, c = totals[name], exp[name], rtotals[name]
        if a.dtype == torch.float64:
            a, b, c = f64_bits(a), f64_bits(b), f64_bits(c)
        assert torch.equal(a, b) and torch.equal(c, b), name
    assert int(totals["n_episodes"].sum()) > 0 and bool((oca[:, :, 0] != 0).any())


def test_k_steps_shaped_without_autoreset_freeze_like_step(ea):
    """the shaped env (tolerance, prev_score) and frozen lanes through the K-step call, against step()"""
    S, N, K = 5, 700, 6
    kw = dict(board_size=S, opponent_policy="random", rng="philox", autoreset=False, philox_key=3, shaped=True, reward=10.0,
              illegal_move_reward=-1.0, illegal_move_tolerance=2)
    A, Bv = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    seeds = (np.arange(N, dtype=np.uint64) + 50).astype(np.uint32)
    po = make_model(S, 9).flat_parameters()
    for e in (A, Bv):
        e.reset(seeds=seeds)
        e.set_opponent_model(po, deterministic=False, noise_key=5)
    traj = A.alloc_rollout(K)
    for launch in range(3):
        A.rollout(K, agent="sample", traj=traj)
        for k in range(K):
            _, _, reward, term, trunc, info = Bv.step(traj["action"][k])
            assert torch.equal(Bv.board, traj["board"][k]) and torch.equal(f64_bits(reward), f64_bits(traj["reward"][k])), (launch, k)
            assert torch.equal(term, traj["terminated"][k]) and torch.equal(trunc, traj["truncated"][k]) and torch.equal(info, traj["info"][k]), (launch, k)
        _state_equal(A, Bv, launch, shaped=True)
    assert bool((A.done != 0).any()) and bool((A.tolerance < 2).any())


# ---------------------------------------------------------------- guard zones

@pytest.mark.parametrize("S,N", [(5, 257), (7, 257), (5, 9000)])
def test_guard_zones(ea, S, N):
    """exact guard zones around every buffer of both calls: env state and step outputs, the opponent's parameters, its action column,
    trajectory columns / records and totals"""
    alloc = GuardedAllocator()
    try:
        K = 5
        po = make_model(S, 9).flat_parameters()
        for layout in ("columns", "record"):
            with alloc.patch(tag="env"):
                env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, autoreset=True,
                                seed_stride=N, philox_key=5, want_terminal_obs=True)
                totals = env.alloc_totals()
                traj = env.alloc_rollout(K, layout=layout)
            env.reset(seeds=torch.arange(N, dtype=torch.int32))
            o = alloc.zeros(po.numel(), tag="opponent params")
            o.copy_(po)
            oc1 = alloc.zeros((N, 3), dtype=torch.int8, tag="opponent action, one step")
            ock = alloc.zeros((K, N, 3), dtype=torch.int8, tag="opponent action, K steps")
            act = alloc.zeros((N, 2), dtype=torch.int8, tag="actions")
            act[:, 1] = 1
            env.set_opponent_model(o, deterministic=False, noise_key=4, opponent_action=oc1)
            assert alloc.owns(env.board) and alloc.owns(env.rng_state) and alloc.owns(env.tolerance) and alloc.owns(env.terminal_board)
            for _ in range(3):
                env.step(act)
            for agent, depth in (("random", 0), ("sample", 0), ("minimax", 3), ("minimax", 5)):
                env.rollout(K, agent=agent, agent_max_depth=depth, traj=traj, totals=totals, opponent_action=ock)
                env.rollout(K, agent=agent, agent_max_depth=depth)
            torch.cuda.synchronize()
            alloc.check("step_vs S=%d N=%d %s" % (S, N, layout))
            assert bool((ock[:, :, 0] != 0).any()) and int(totals["n_steps"].sum()) > 0
        with alloc.patch(tag="mt env"):
            env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="mt19937", autoreset=False)
            totals = env.alloc_totals()
        env.reset(seeds=torch.arange(N, dtype=torch.int32))
        env.set_opponent_model(o, opponent_action=oc1)
        for _ in range(3):
            env.step(act)
        env.rollout(K, agent="minimax", agent_max_depth=4, totals=totals, opponent_action=ock)
        torch.cuda.synchronize()
        alloc.check("step_vs mt19937 S=%d N=%d" % (S, N))
    finally:
        alloc.clear()


# ---------------------------------------------------------------- the Python surface

def test_set_and_clear_the_model_and_refusals(ea):
    N, S = 300, 5
    kw = dict(board_size=S, opponent_policy="minimax", max_depth=2, rng="philox", autoreset=True, philox_key=4)
    a, b = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    a.reset(seeds=np.arange(N) + 1)
    b.reset(seeds=np.arange(N) + 1)
    p = make_model(S, 3).flat_parameters()
    assert a.supports_step_vs()
    with pytest.raises(ValueError, match="opponent_params"):
        a.set_opponent_model(p[:-1])
    with pytest.raises(ValueError, match="opponent_action"):
        a.set_opponent_model(p, opponent_action=torch.zeros((N, 2), dtype=torch.int8, device="cuda"))
    with pytest.raises(ValueError, match="opponent_action"):
        a.rollout(2, opponent_action=torch.zeros((2, N, 3), dtype=torch.int8, device="cuda"))
    a.set_opponent_model(p)
    assert not a.supports_agent_rollout({"kind": "mcts"}) and a.supports_rollout("minimax", 6) and not a.supports_rollout("mlp")
    with pytest.raises(ea._lib.EwnError, match="agent_rollout"):
        a.agent_rollout(2, {"kind": "mcts"})
    a.set_opponent_model(None)                 # nothing was stepped: the env is the minimax(2) env it was
    act = torch.zeros((N, 2), dtype=torch.int8, device="cuda")
    act[:, 1] = 2
    for _ in range(6):
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    assert torch.equal(a.rng_state, b.rng_state)
    assert not ea.VecEWN(64, board_size=6, opponent_policy="random", rng="philox").supports_step_vs()
    assert not ea.VecEWN(64, opponent_policy="random", rng="mt19937", autoreset=True).supports_step_vs()
    with pytest.raises(ea._lib.EwnError, match="set_opponent_model"):
        ea.VecEWN(64, opponent_policy="random", rng="mt19937", autoreset=True).set_opponent_model(p)
    with pytest.raises(ea._lib.EwnError, match="eval_policy"):
        ea.VecEWN(8, opponent_policy="models/best.pt")          # the constructor keeps refusing a path, with the message it has


def test_the_set_model_is_the_default_opponent_of_the_policy_calls(ea):
    N, S = 257, 5
    kw = dict(board_size=S, opponent_policy="random", rng="philox", autoreset=False, philox_key=8)
    a, b = ea.VecEWN(N, **kw), ea.VecEWN(N, **kw)
    a.reset(seeds=np.arange(N) + 9)
    b.reset(seeds=np.arange(N) + 9)
    pa, po = make_model(S, 5).flat_parameters(), make_model(S, 9).flat_parameters()
    a.set_opponent_model(po)
    ta, tb = a.alloc_totals(), b.alloc_totals()
    a.eval_policy(8, pa, ta)
    b.eval_policy(8, pa, tb, opponent_params=po)
    _state_equal(a, b, "eval_policy default opponent")
    assert torch.equal(ta["n_steps"], tb["n_steps"]) and int(ta["n_steps"].sum()) > N


@pytest.mark.parametrize("shaped", [False, True])
def test_dropin_env_loads_a_checkpoint_as_its_opponent(ea, tmp_path, shaped):
    """envs.EinsteinWuerfeltNichtEnv(opponent_policy=<path>): a seeded N = 1 episode equals lane 0 of a VecEWN run on the same seed"""
    import envs
    from ewn_gym_amd import vec_env as ve
    S = 5
    model = make_model(S, 9)
    path = str(tmp_path / "opp.pt")
    torch.save({"algorithm": "A2C", "fused": True, "params": model.flat_parameters(), "num_timesteps": 0}, path)
    skw = dict(shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10) if shaped else {}
    steps = 0
    for seed in (9487, 11, 12, 13):
        vec = ea.VecEWN(4, board_size=S, opponent_policy="random", rng="mt19937", **skw)
        vec.reset(seeds=[seed, 1, 2, 3])
        vec.set_opponent_model(model.flat_parameters())
        if shaped:   # reference_quirks=True would drop seed, reward and the opponent, as upstream does (envs/minimax_ewn.py:17-19)
            env = envs.MiniMaxHeuristicEnv(board_size=S, seed=seed, opponent_policy=path, reference_quirks=False)
        else:
            env = envs.EinsteinWuerfeltNichtEnv(board_size=S, seed=seed, opponent_policy=path)
        assert env._engine.supports_step_vs() and isinstance(env.opponent_policy, type(model))
        obs = env._obs()
        terminated = False
        for t in range(60):
            assert np.array_equal(obs["board"], vec.board[0].cpu().numpy()) and obs["dice_roll"] == int(vec.dice[0])
            acts = ve.legal_actions(vec.board, vec.dice, player=1)[0][:, 0].clamp(min=0).contiguous()
            obs, reward, terminated, truncated, info = env.step(acts[0].cpu().numpy())
            _, _, r, te, tr, code = vec.step(acts)
            assert reward == float(r[0]) and terminated == bool(te[0]) and truncated == bool(tr[0]), (seed, t)
            assert info.get("message") == ea.INFO_MESSAGES[int(code[0])], (seed, t)
            steps += 1
            if terminated:
                break
        assert terminated
        assert np.array_equal(obs["board"], vec.board[0].cpu().numpy())
    assert steps > 6, steps
    bad = str(tmp_path / "sb3.zip")
    with open(bad, "wb") as f:
        f.write(b"PK\x03\x04 not a checkpoint of these trainers")
    with pytest.raises(NotImplementedError, match="SB3"):
        envs.EinsteinWuerfeltNichtEnv(board_size=S, opponent_policy=bad)


def test_evaluate_vs_model_k_step_and_ply_by_ply_agree(ea):
    from ewn_gym_amd import tournament
    model = make_model(5, 9)
    opp = {"kind": "mlp", "model": model}
    for agent in ({"kind": "random"}, {"kind": "minimax", "max_depth": 3}):
        for rng in ("mt19937", "philox"):
            k = tournament.evaluate_vs_model(agent, opp, num=256, rng=rng)
            p = tournament.evaluate_vs_model(agent, opp, num=256, rng=rng, use_rollout=False)
            assert k["engine"] == "ewn_step_k_vs" and p["engine"] == "ewn_step_vs", (k["engine"], p["engine"])
            assert torch.equal(f64_bits(k["scores"]), f64_bits(p["scores"])) and torch.equal(k["lengths"], p["lengths"]), (agent, rng)
            assert k["wins"] == p["wins"] and k["episodes"] == 256 and int((k["lengths"] > 0).sum()) == 256
            print("evaluate_vs_model %s %s: wins %d, losses %d, forfeits %d of 256, %.1f steps/episode"
                  % (agent, rng, k["wins"], int((k["scores"] < 0).sum()), int((k["scores"] == 0).sum()), k["avg_length"]))
    m = tournament.evaluate_vs_model({"kind": "mcts", "num_simulations": 3, "num_env_copies": 2}, opp, num=64)
    assert m["engine"] == "ewn_step_vs" and m["episodes"] == 64
    h = tournament.evaluate_vs_model({"kind": "minimax", "max_depth": 2, "heuristic": "attk"}, opp, num=64)
    assert h["engine"] == "ewn_step_vs"
    mm = tournament.evaluate_vs_model({"kind": "mlp", "model": model}, opp, num=64)
    assert mm["engine"] == "ewn_policy_eval_vs"
    with pytest.raises(ValueError, match="model agent"):         # evaluate() itself is unchanged
        tournament.evaluate({"kind": "random"}, opp, num=16)


def test_cli_agents_against_an_opponent_model(ea, tmp_path, monkeypatch, capsys):
    import json
    import sys
    from ewn_gym_amd import tournament
    b = str(tmp_path / "b.pt")
    torch.save({"algorithm": "A2C", "fused": True, "params": make_model(5, 9).flat_parameters(), "num_timesteps": 0}, b)
    monkeypatch.setattr(sys, "argv", ["tournament", "--agents", "random", "minimax", "--max_depth", "3", "--opponent_model", b, "--num", "128"])
    tournament.main()
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(out) == {"random vs opponent_model", "minimax vs opponent_model"}
    r = tournament.evaluate_vs_model({"kind": "minimax", "max_depth": 3}, {"kind": "mlp", "model": tournament.load_policy(b)}, num=128)
    row = out["minimax vs opponent_model"]
    assert row["engine"] == "ewn_step_k_vs" and row["episodes"] == 128 and row["wins"] == r["wins"] and row["avg_length"] == r["avg_length"]
