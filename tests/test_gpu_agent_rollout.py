"""ewn_step_k_agent: the MCTS agent (against RandomAgent, minimax and MCTS) and the minimax agent against MCTS, K steps per launch.
The core checks are bit-exactness against the per-step path it replaces (tournament.evaluate(use_rollout=False): predict_mcts /
predict_minimax + ewn_step per ply) and, step by step, against the CPU oracle; then exact guard zones around every buffer the kernel
touches, and the whole tournament matrix in the engine."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from tests.guarded_alloc import GuardedAllocator  # noqa: E402

GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


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


def mcts(ns=3, nc=2):
    return {"kind": "mcts", "num_simulations": ns, "num_env_copies": nc}


def mm(d, h="hybrid"):
    return {"kind": "minimax", "max_depth": d, "heuristic": h}


def _same(a, b):
    assert a["engine"] == "ewn_step_k_agent" and b["engine"] == "ewn_step"
    assert torch.equal(a["scores"].view(torch.int64), b["scores"].view(torch.int64))
    assert torch.equal(a["lengths"], b["lengths"])
    assert a["wins"] == b["wins"] and a["ci95"] == b["ci95"]


CELLS = [
    (mcts(), {"kind": "random"}),
    (mcts(), mm(1, "min_dist")),
    (mcts(2, 2), mm(3, "two_min_dist")),
    (mcts(), mm(4, "attk")),
    (mcts(3, 2), mcts(2, 3)),
    (mm(1, "attk"), mcts()),
    (mm(2, "hybrid"), mcts()),
    (mm(3, "two_min_dist"), mcts(2, 2)),
    (mm(5, "min_dist"), mcts()),
]


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("cell", range(len(CELLS)))
def test_engine_equals_the_per_step_loop(ea, S, rng, cell):
    from ewn_gym_amd.tournament import evaluate
    agent, opp = CELLS[cell]
    chunk = (5, 7, 3)[cell % 3]                 # not a divisor of the game lengths
    kw = dict(num=96 + 37 * (cell % 3), board_size=S, rng=rng, key=1000 + cell)
    a = evaluate(agent, opp, use_rollout=True, chunk=chunk, **kw)
    b = evaluate(agent, opp, use_rollout=False, **kw)
    _same(a, b)
    assert a["lengths"].min().item() >= 1


def test_full_size_mcts_against_minimax5(ea):
    from ewn_gym_amd.tournament import evaluate
    agent, opp = mcts(10, 5), mm(5)
    a = evaluate(agent, opp, num=1024)
    b = evaluate(agent, opp, num=1024, use_rollout=False)
    _same(a, b)


def _agent_vs_oracle(ea, N, lo, hi, K, launches, agent, autoreset=True, layout="columns", key=77, **kw):
    okw = dict(kw)
    opp = okw.pop("opponent_policy")
    env = ea.VecEWN(N, opponent_policy=opp, autoreset=autoreset, seed_stride=N, **okw)
    assert env.supports_agent_rollout(agent)
    seeds = (np.arange(N, dtype=np.uint64) * 7 + 1234).astype(np.uint32)
    env.reset(seeds=seeds)
    orc = po.OracleVecEnv(hi - lo, opponent=opp, autoreset=autoreset, seed_stride=N, lane_offset=lo, **okw)
    ob, od = orc.reset(seeds=seeds[lo:hi])
    ref = ea.VecEWN(hi - lo, opponent_policy=opp, autoreset=autoreset, seed_stride=N, lane_offset=lo, **okw)   # the per-step path
    ref.reset(seeds=seeds[lo:hi])
    traj = env.alloc_rollout(K, layout=layout)
    totals = env.alloc_totals()
    frozen = np.zeros(hi - lo, bool)
    ret = np.zeros(hi - lo)
    nst = np.zeros(hi - lo, np.int64)
    nep = np.zeros(hi - lo, np.int64)
    nwin = np.zeros(hi - lo, np.int64)
    ids = np.arange(lo, hi, dtype=np.uint32)
    for launch in range(launches):
        env.agent_rollout(K, agent, step_base=launch * K, key=key, traj=traj, totals=totals)
        tj = {k: cpu(v[:, lo:hi]) for k, v in traj.items()}
        for k in range(K):
            t = launch * K + k
            if agent["kind"] == "mcts":
                acts = po.predict_mcts(ob, od, agent["num_simulations"], agent["num_env_copies"], key=(key + GOLDEN * (t + 1)) & M64,
                                       obs_id=ids)[0]
            else:
                acts = po.predict_minimax(ob, od, agent["max_depth"], agent["heuristic"])[0]
            live = ~frozen
            ctx = (agent, kw, launch, k)
            assert np.array_equal(tj["action"][k][live], acts[live]), ctx
            ob, od, r, te, tr, info = orc.step(np.where(live[:, None], acts, 0).astype(np.int8))
            ref.step(torch.from_numpy(np.ascontiguousarray(acts, dtype=np.int8)).cuda())
            assert np.array_equal(tj["board"][k], ob), ctx
            assert np.array_equal(tj["dice"][k], od), ctx
            assert np.array_equal(bits(tj["reward"][k]), bits(r)), ctx
            assert np.array_equal(tj["terminated"][k], te) and np.array_equal(tj["truncated"][k], tr), ctx
            assert np.array_equal(tj["info"][k], info), ctx
            ret += np.where(live, r, 0.0)
            nst += live
            nep += live & (te != 0)
            nwin += live & (info == 2)
            if not autoreset:
                frozen |= te != 0
        assert np.array_equal(cpu(env.board[lo:hi]), ob) and np.array_equal(cpu(env.dice[lo:hi]), od), (kw, launch)
        assert np.array_equal(cpu(env.done[lo:hi]) != 0, frozen), (kw, launch)
    assert np.array_equal(bits(cpu(totals["return_sum"][lo:hi])), bits(ret))
    assert np.array_equal(cpu(totals["n_steps"][lo:hi]), nst) and np.array_equal(cpu(totals["n_episodes"][lo:hi]), nep)
    assert np.array_equal(cpu(totals["n_wins"][lo:hi]), nwin)
    # the RNG headers the engine carries are those of ewn_step fed the same actions
    assert torch.equal(env.rng_state.view(-1)[:4 * N].view(N, 4)[lo:hi], ref.rng_state.view(-1)[:4 * (hi - lo)].view(hi - lo, 4))
    return int(nep.sum())


ORACLE_CASES = [
    # N, lo, hi, K, launches, agent, kw
    (257, 0, 257, 3, 3, mcts(3, 2), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2, rng="philox")),
    (257, 0, 257, 1, 4, mm(4, "attk"), dict(opponent_policy="mcts", num_simulations=3, num_env_copies=2, rng="philox",
                                            layout="record")),
    (3000, 1000, 1300, 7, 2, mcts(2, 3), dict(opponent_policy="minimax", max_depth=3, heuristic="min_dist", rng="mt19937",
                                               autoreset=False)),
    (3000, 2800, 3000, 7, 3, mm(2, "two_min_dist"), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2,
                                                          rng="mt19937", autoreset=False, layout="record")),
    (300, 40, 300, 3, 3, mcts(4, 2), dict(opponent_policy="random", rng="philox", board_size=7)),
    (200, 0, 200, 7, 2, mm(3, "hybrid"), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=3, rng="mt19937",
                                               autoreset=False, board_size=7)),
]


@pytest.mark.parametrize("case", range(len(ORACLE_CASES)))
def test_lock_step_against_the_oracle(ea, case):
    N, lo, hi, K, launches, agent, kw = ORACLE_CASES[case]
    kw = dict(kw)
    layout = kw.pop("layout", "columns")
    autoreset = kw.pop("autoreset", True)
    _agent_vs_oracle(ea, N, lo, hi, K, launches, agent, autoreset=autoreset, layout=layout, philox_key=4242, **kw)


@pytest.mark.parametrize("agent,opp", [(mcts(3, 2), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2)),
                                       (mm(3, "attk"), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2)),
                                       (mcts(3, 2), dict(opponent_policy="random"))])
def test_two_half_size_engines_equal_one_full_one(ea, agent, opp):
    """lane_offset enters the MCTS agent's playout stream (obs_id = lane_offset + lane) as it enters the dice and the opponent's"""
    N, K = 300, 5
    seeds = torch.arange(N, dtype=torch.int32) * 3 + 11

    def run(n, off):
        env = ea.VecEWN(n, autoreset=True, seed_stride=N, lane_offset=off, rng="philox", philox_key=99, **opp)
        env.reset(seeds=seeds[off:off + n])
        traj, totals = env.alloc_rollout(K), env.alloc_totals()
        for launch in range(3):
            env.agent_rollout(K, agent, step_base=launch * K, key=5, traj=traj, totals=totals)
        return env, traj, totals

    full = run(N, 0)
    halves = [run(N // 2, 0), run(N // 2, N // 2)]
    for name in ("board", "dice", "done"):
        assert torch.equal(getattr(full[0], name), torch.cat([getattr(h[0], name) for h in halves])), name
    for k in full[1]:
        assert torch.equal(full[1][k], torch.cat([h[1][k] for h in halves], dim=1)), k
    for k in full[2]:
        assert torch.equal(full[2][k], torch.cat([h[2][k] for h in halves])), k
    assert int(full[2]["n_episodes"].sum()) > 0


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("N", [257, 3000])
def test_guard_zones(ea, S, N):
    """every buffer the kernel reads or writes sits between 4 KB of 0xA5 on both sides: board / dice / done / rng (the env's own
    allocations), the totals, the columns and the record trajectory"""
    K = 4
    alloc = GuardedAllocator()
    try:
        for agent, opp, rng, autoreset in ((mcts(2, 2), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2), "philox", True),
                                          (mm(2, "min_dist"), dict(opponent_policy="mcts", num_simulations=2, num_env_copies=2), "mt19937",
                                           False),
                                          (mcts(2, 2), dict(opponent_policy="minimax", max_depth=2), "mt19937", False),
                                          (mcts(2, 2), dict(opponent_policy="random"), "philox", True)):
            with alloc.patch(tag="env"):
                env = ea.VecEWN(N, board_size=S, rng=rng, autoreset=autoreset, philox_key=5, **opp)
                totals = env.alloc_totals()
            env.reset(seeds=torch.arange(N, dtype=torch.int32))
            cols = {"board": alloc.zeros((K, N, S, S), dtype=torch.int8, tag="board"),
                    "dice": alloc.zeros((K, N), dtype=torch.int8, tag="dice"),
                    "action": alloc.zeros((K, N, 2), dtype=torch.int8, tag="action"),
                    "reward": alloc.zeros((K, N), dtype=torch.float64, tag="reward"),
                    "terminated": alloc.zeros((K, N), dtype=torch.uint8, tag="terminated"),
                    "truncated": alloc.zeros((K, N), dtype=torch.uint8, tag="truncated"),
                    "info": alloc.zeros((K, N), dtype=torch.uint8, tag="info")}
            stride = (S * S + 6 + 15) & ~15
            rec = {"record": alloc.zeros((K, N, stride), dtype=torch.uint8, tag="record"),
                   "reward": alloc.zeros((K, N), dtype=torch.float64, tag="rec_reward")}
            for t in list(totals.values()) + [env.board, env.dice, env.done, env.rng_state]:
                assert alloc.owns(t)
            for launch in range(2):
                env.agent_rollout(K, agent, step_base=2 * launch * K, key=3, traj=cols, totals=totals)
                env.agent_rollout(K, agent, step_base=(2 * launch + 1) * K, key=3, traj=rec, totals=totals)
            torch.cuda.synchronize()
            alloc.check("S=%d N=%d %s %s" % (S, N, agent, opp))
            assert int(totals["n_steps"].sum()) > 0
    finally:
        alloc.clear()


def test_malformed_buffers_raise_before_a_launch(ea):
    env = ea.VecEWN(64, opponent_policy="mcts", num_simulations=2, num_env_copies=2, rng="philox")
    env.reset(seeds=torch.arange(64, dtype=torch.int32))
    board = env.board.clone()
    bad = [dict(traj={"reward": torch.zeros((4, 64), dtype=torch.float32, device="cuda")}),
           dict(traj={"action": torch.zeros((2, 64, 2), dtype=torch.int8, device="cuda")}),
           dict(traj={"dice": torch.zeros((4, 64), dtype=torch.int8)}),
           dict(totals={"n_steps": torch.zeros(63, dtype=torch.int32, device="cuda")}),
           dict(totals={"return_sum": torch.zeros((64, 2), dtype=torch.float64, device="cuda")[:, 0]})]
    for b in bad:
        with pytest.raises(ValueError):
            env.agent_rollout(4, mcts(), **b)
    with pytest.raises(ValueError):
        env.agent_rollout(4, {"kind": "random"})
    torch.cuda.synchronize()
    assert torch.equal(env.board, board)


def test_the_whole_matrix_runs_in_the_engine(ea):
    from ewn_gym_amd.tournament import tournament
    t = tournament(num=256)
    assert len(t) == 9
    for k, v in t.items():
        assert v["engine"] != "ewn_step", k
    assert t["mcts vs mcts"]["engine"] == "ewn_step_k_agent" and t["minimax vs mcts"]["engine"] == "ewn_step_k_agent"
