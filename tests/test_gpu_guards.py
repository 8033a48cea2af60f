"""Exact guard zones (tests/guarded_alloc.py: 4 KB of 0xA5 directly in front of and directly behind every buffer, no round-up slack)
around every buffer of the entry points the A2C path runs on: the record trajectory layout through ewn_step_k (one case per kernel
family the dispatcher can pick), ewn_step_k_policy in its three forms, ewn_a2c_grad's scratch and gradient, ewn_a2c_apply on both of
its paths, ewn_roll_dice and FusedA2CTrainer end to end.  Lane counts leave partial last blocks.  The table images the kernels read
are rebuilt through the guarded allocator too and checked after every case."""
import ctypes as C

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


@pytest.fixture(scope="module")
def tables(ea):
    """the search-table images, rebuilt as guarded buffers for this module (the cache is restored afterwards)"""
    from ewn_gym_amd import vec_env
    saved = dict(vec_env._TABLES)
    vec_env._TABLES.clear()
    t = GuardedAllocator()
    try:
        with t.patch(tag="tables"):
            for (S, L) in ((5, 3), (7, 3)):
                assert vec_env.search_tables(S, L, torch.device("cuda")) is not None
        yield t
        t.check("table images")
    finally:
        vec_env._TABLES.clear()
        vec_env._TABLES.update(saved)


@pytest.fixture
def alloc(tables):
    a = GuardedAllocator()
    yield a
    a.clear()


def _seeds(n, off=3):
    return (np.arange(n, dtype=np.uint64) + off).astype(np.uint32)


def _done(alloc, tables, ctx):
    torch.cuda.synchronize()
    alloc.check(ctx)
    tables.check(ctx)


# ---------------------------------------------------------------- ewn_step_k, record layout

REC_CASES = [
    ("slots-T2", 3000, dict(opponent_policy="minimax", max_depth=3, rng="philox"), 2),
    ("slots-T2-257", 257, dict(opponent_policy="minimax", max_depth=3, rng="philox"), 2),
    ("slots-T1", 140000, dict(opponent_policy="minimax", max_depth=3, rng="philox"), 1),
    ("two_min_dist", 3000, dict(opponent_policy="minimax", max_depth=3, heuristic="two_min_dist", rng="philox"), None),
    ("mcts-100", 100, dict(opponent_policy="mcts", num_simulations=3, num_env_copies=2, rng="philox"), None),
    ("mcts-300", 300, dict(opponent_policy="mcts", num_simulations=3, num_env_copies=2, rng="philox"), None),
    ("generic-7x7-L4", 3000, dict(opponent_policy="minimax", max_depth=2, heuristic="attk", rng="philox", board_size=7, cube_layer=4), None),
    ("generic-9x9", 257, dict(opponent_policy="random", rng="philox", board_size=9), None),
    ("mt19937-no-autoreset", 40000, dict(opponent_policy="minimax", max_depth=3, rng="mt19937", autoreset=False), None),
]


@pytest.mark.parametrize("name,n,kw,lanes_per_game", REC_CASES, ids=[c[0] for c in REC_CASES])
def test_record_layout_through_step_k(ea, tables, alloc, name, n, kw, lanes_per_game):
    from ewn_gym_amd._lib import AGENT, EwnRolloutOut, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    kw = dict(kw)
    autoreset = kw.pop("autoreset", True)
    K = 6
    with alloc.patch(tag=name):
        env = ea.VecEWN(n, autoreset=autoreset, seed_stride=n, **kw)
        rec = env.alloc_rollout(K, layout="record")
        cols = env.alloc_rollout(K)
        tot = env.alloc_totals()
    assert env.supports_rollout("random")
    if lanes_per_game is not None:          # the kernel family this case is meant to run
        assert env.lib.ewn_lanes_per_game(C.byref(env.cfg), 1) == lanes_per_game
    env.reset(seeds=_seeds(n))
    # the record alone with totals (rollout()), then the record with every column alongside (the ABI directly: rollout() drops the
    # columns when it sees a record)
    env.rollout(K, traj=rec, totals=tot)
    out = EwnRolloutOut(_ptr(cols["board"]), _ptr(cols["dice"]), _ptr(cols["action"]), _ptr(cols["reward"]), _ptr(cols["terminated"]),
                        _ptr(cols["truncated"]), _ptr(cols["info"]), _ptr(tot["return_sum"]), _ptr(tot["n_steps"]),
                        _ptr(tot["n_episodes"]), _ptr(tot["n_wins"]), _ptr(rec["record"]))
    for _ in range(2):
        check(env.lib.ewn_step_k(C.byref(env.cfg), C.byref(env._st), K, AGENT["random"], 3, C.byref(out), _stream()), "ewn_step_k")
    torch.cuda.synchronize()
    assert torch.equal(rec["action"], cols["action"]) and torch.equal(rec["board"], cols["board"])   # one launch wrote both
    env.rollout(K - 1, traj=rec)           # fewer steps than the buffers hold
    _done(alloc, tables, name)
    assert int(tot["n_steps"].sum()) > 0


SPARSE_CASES = [
    # 8 games per block: a partial last block of 4
    ("mcts-100", 100, dict(opponent_policy="mcts", num_simulations=3, num_env_copies=2, rng="philox")),
    # 256 games per block: one game in the last block
    ("generic-9x9-257", 257, dict(opponent_policy="random", rng="philox", board_size=9)),
]
SPARSE_RUNS = [("reward", "n_wins"), ("terminated", "action", "return_sum")]


@pytest.mark.parametrize("name,n,kw", SPARSE_CASES, ids=[c[0] for c in SPARSE_CASES])
def test_step_k_column_guards_one_at_a_time(ea, tables, alloc, name, n, kw):
    """Every member of ewn_rollout_out is optional on its own in the one-thread-per-game K-step kernels: a call with a few members
    non-NULL writes into them what the call with every member writes, and leaves the same state behind."""
    from ewn_gym_amd._lib import AGENT, EwnRolloutOut, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    K = 6
    members = [f[0] for f in EwnRolloutOut._fields_]
    with alloc.patch(tag=name):
        env = ea.VecEWN(n, seed_stride=n, **kw)
    assert env.supports_rollout("random")

    def run(only):
        with alloc.patch(tag="%s-%s" % (name, "+".join(only or ("all",)))):
            bufs = dict(env.alloc_rollout(K), **env.alloc_totals())
            bufs["record"] = env.alloc_rollout(K, layout="record")["record"]
        env.reset(seeds=_seeds(n))
        out = EwnRolloutOut(*[_ptr(bufs[m]) if only is None or m in only else None for m in members])
        check(env.lib.ewn_step_k(C.byref(env.cfg), C.byref(env._st), K, AGENT["random"], 3, C.byref(out), _stream()), "ewn_step_k")
        torch.cuda.synchronize()
        return bufs, [t.clone() for t in (env.board, env.dice, env.done, env.rng_state)]

    full, state = run(None)
    assert int(full["n_steps"].sum()) > 0 and bool(full["action"].any())
    for only in SPARSE_RUNS:
        got, st = run(only)
        for m in only:
            assert torch.equal(got[m].view(torch.uint8), full[m].view(torch.uint8)), (only, m)
        for a, b in zip(st, state):
            assert torch.equal(a, b), only
    _done(alloc, tables, name)


# ---------------------------------------------------------------- ewn_step_k_policy

def _policy_env(ea, alloc, S, n, tag):
    with alloc.patch(tag=tag):
        env = ea.VecEWN(n, board_size=S, opponent_policy="minimax", max_depth=3, rng="philox", shaped=True, reward=10.0,
                        illegal_move_tolerance=4, shaped_refresh_on_reset=True, autoreset=True, seed_stride=n, philox_key=31)
    env.reset(seeds=_seeds(n, 11))
    return env


def _guarded_params(ea, alloc, env, S, seed=5):
    from tests.test_gpu_policy import make_model
    params = alloc.zeros(env.policy_param_count(), tag="params")
    params.copy_(make_model(S, seed).flat_parameters())
    return params


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("n", [1, 257, 3000, 40000])
def test_policy_rollout_forms(ea, tables, alloc, S, n):
    K = 5
    env = _policy_env(ea, alloc, S, n, "env")
    params = _guarded_params(ea, alloc, env, S)
    with alloc.patch(tag="generic form"):
        traj = env.alloc_rollout(K, layout="record", initial_obs=True)
        tot = env.alloc_totals()
    logits = alloc.zeros((K, n, 5), tag="logits")
    value = alloc.zeros((K, n), tag="value")
    noise = alloc.zeros((K, n, 5), tag="noise")
    with alloc.patch(tag="trainer form"):
        ttraj = env.alloc_rollout(K, layout="record", initial_obs=True)
    with alloc.patch(tag="columns form"):
        ctraj = env.alloc_rollout(K)
        ctot = env.alloc_totals()
    for launch in range(2):
        env.rollout_policy(K, params, traj=traj, totals=tot, noise_key=7, logits=logits, value=value, noise=noise)
        env.rollout_policy(K, params, traj=ttraj, noise_key=7)                       # FusedA2CTrainer's call: records + reward only
        env.rollout_policy(K, params, traj=ctraj, totals=ctot, noise_key=7, value=value)
    _done(alloc, tables, "S=%d n=%d" % (S, n))
    assert bool((noise > 0).all()) and bool((noise < 1).all())


# ---------------------------------------------------------------- ewn_a2c_grad / ewn_a2c_apply

def _a2c_records(ea, alloc, S, n, K):
    env = _policy_env(ea, alloc, S, n, "env")
    params = _guarded_params(ea, alloc, env, S, seed=11)
    with alloc.patch(tag="records"):
        traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    for _ in range(2):
        env.rollout_policy(K, params, traj=traj, noise_key=5)
    return env, params, traj


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("n,K", [(1001, 3), (1000, 3), (1, 5), (31, 5), (40000, 5)])
def test_a2c_grad_scratch_and_gradient(ea, tables, alloc, S, n, K):
    """scratch of exactly ewn_a2c_scratch_bytes bytes, gradient of exactly P + 8 floats; an odd K * N takes k_a2c_reduce (partial is
    then 4-byte aligned only), an even one k_a2c_reduce2.  The scratch's last 64 floats are written by a timing build only
    (ewn_a2c_scratch_bytes): a scratch short by up to 256 bytes goes unnoticed here, one short by 260 does not."""
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    env, params, traj = _a2c_records(ea, alloc, S, n, K)
    P = params.numel()
    nscr = int(check(env.lib.ewn_a2c_scratch_bytes(C.byref(env.cfg), K)))
    scratch = alloc.zeros(nscr, dtype=torch.uint8, tag="scratch")
    grad = alloc.zeros(P + 8, tag="grad")
    hp = EwnA2cHyper(0.97, 0.5, 0.01, 0.5, 7e-4, 0.99, 1e-5, 1)
    for _ in range(2):
        check(env.lib.ewn_a2c_grad(C.byref(env.cfg), K, _ptr(traj["record"]), _ptr(traj["reward"]), _ptr(params), C.byref(hp), _ptr(grad),
                                   _ptr(scratch), _stream()), "ewn_a2c_grad")
    _done(alloc, tables, "S=%d n=%d K=%d" % (S, n, K))
    assert bool(torch.isfinite(grad).all()) and float(grad[:P].abs().max()) > 0


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("offset", [0, 4], ids=["v4", "scalar"])
def test_a2c_apply_buffers(ea, tables, alloc, S, offset):
    """params / sq_avg / grad of exactly P / P / P + 8 floats and grad_norm[1]; offset 4 (one float past a 16-byte boundary) forces
    the scalar k_a2c_apply"""
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.vec_env import _ptr, _stream
    env = ea.VecEWN(64, board_size=S, opponent_policy="random", rng="philox")
    P = env.policy_param_count()
    g = torch.Generator(device="cuda").manual_seed(S)
    params = alloc.zeros(P, tag="params", offset=offset)
    sq = alloc.zeros(P, tag="sq_avg", offset=offset)
    grad = alloc.zeros(P + 8, tag="grad", offset=offset)
    norm = alloc.zeros(1, tag="grad_norm", offset=offset)
    params.copy_(torch.randn(P, device="cuda", generator=g))
    grad.copy_(torch.randn(P + 8, device="cuda", generator=g))
    for mgn in (0.5, 0.0):
        hp = EwnA2cHyper(0.99, 0.5, 0.0, mgn, 7e-4, 0.99, 1e-5, 1)
        for _ in range(2):
            check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    _done(alloc, tables, "S=%d offset=%d" % (S, offset))
    assert float(norm) > 0 and bool((sq > 0).all())


# ---------------------------------------------------------------- ewn_roll_dice

@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("n", [257, 3000])
def test_roll_dice_buffers(ea, tables, alloc, rng, n):
    with alloc.patch(tag="env"):
        env = ea.VecEWN(n, opponent_policy="random", rng=rng, autoreset=True)
    env.reset(seeds=_seeds(n, 17))
    mask = alloc.zeros(n, dtype=torch.uint8, tag="mask")
    mask.copy_(torch.from_numpy((np.arange(n) % 3 != 1).astype(np.uint8)))
    before = env.dice.clone()
    for _ in range(3):
        env.roll_dice(mask)
        env.roll_dice()
    _done(alloc, tables, "%s n=%d" % (rng, n))
    assert int(env.dice.min()) >= 1 and not torch.equal(before, env.dice)


# ---------------------------------------------------------------- the fused trainer end to end

def test_fused_trainer_buffers(ea, tables, alloc):
    from ewn_gym_amd.a2c import FusedA2CTrainer
    n = 3000
    with alloc.patch(tag="trainer"):
        env = ea.VecEWN(n, opponent_policy="minimax", max_depth=3, rng="philox", shaped=True, reward=10.0, illegal_move_reward=-1.0,
                        illegal_move_tolerance=10, shaped_refresh_on_reset=True, autoreset=True, seed_stride=n, philox_key=9487)
        tr = FusedA2CTrainer(env, n_steps=5, learning_rate=7e-4, seed=1, use_graph=False)
    for name, t in (("traj.record", tr.traj["record"]), ("traj.reward", tr.traj["reward"]), ("scratch", tr.scratch), ("grad", tr.grad),
                    ("grad_norm", tr.grad_norm), ("sq_avg", tr.sq_avg)):
        assert alloc.owns(t), name
    env.reset(seeds=_seeds(n, 9487))
    for _ in range(3):
        tr.collect_and_update()
    _done(alloc, tables, "FusedA2CTrainer")
    assert float(tr.grad_norm) > 0
