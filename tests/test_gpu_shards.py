"""A call on N lanes equals the same call on its shards: the engine's multi-GPU design (lanes shard with global lane ids, DESIGN.md
section 5) held against the kernels that carry it in training -- the policy rollouts (ewn_step_k_policy, ewn_step_k_selfplay, the
trainers' instances of both), the evaluation kernels (ewn_policy_eval, ewn_policy_eval_vs), a model as the env's opponent (ewn_step_vs,
ewn_step_k_vs), ewn_predict_random and the PUCT self-play driver.

`whole_and_shards` runs one call sequence on an env of 600 lanes and on envs of 257 and 343 lanes built with lane_offset 0 and 257,
seed_stride 600 and the matching seed slices, and compares every output byte for byte (floats through uint8 views, no tolerance):
neither shard is a multiple of 32 or 64 lanes, and the second starts in the middle of a 32-column tile and of a wave.  Where the
launcher picks a kernel instance by the number of lanes the whole and the shards may run different instances; the headers promise the
same results, and this holds them to it.  Equality alone would pass if nothing depended on the lane id, so the families that sample
run the second shard once more with lane_offset 0 and must then see other samples: the stream really is keyed by the global lane."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_policy import make_model  # noqa: E402

N_LANES, CUT = 600, 257
SHAPED = dict(shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=4, shaped_refresh_on_reset=True)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def end_state(env):
    """the state a launch leaves behind, every entry with the lane in dimension 0.  The RNG buffer is N headers and, for the MT19937
    kind, then N x 3 windows and N reset epochs (csrc/ewn_core.hpp): only the parts are per lane, not the buffer's rows"""
    n, words = env.rng_state.shape
    st = {"board": env.board, "dice": env.dice, "done": env.done}
    if words == 4:
        st["rng_state"] = env.rng_state
    else:
        w, flat = (words - 5) // 3, env.rng_state.view(-1)
        st["rng_header"], st["rng_windows"], st["rng_epoch"] = flat[:4 * n].view(n, 4), flat[4 * n:4 * n + 3 * n * w].view(n, 3 * w), flat[4 * n + 3 * n * w:]
        assert st["rng_epoch"].numel() == n
    if env.prev_score is not None:
        st["prev_score"], st["tolerance"] = env.prev_score, env.tolerance
    return st


def cut(outs, lo, n):
    return {k: t.narrow(dim, lo, n) for k, (t, dim) in outs.items()}


def whole_and_shards(ea, env_kw, play, differs=None, N=N_LANES, c=CUT):
    """play(env, ref, misplaced) runs the family's call sequence on a freshly reset env and returns {name: (tensor, the lane's
    dimension)}; ref is None for the whole and the whole's outputs cut to the env's lanes for a shard (a sequence whose length the whole
    decides reads it there).  differs(outputs) picks the sampled output that must change when the second shard is built with
    lane_offset 0 (misplaced=True).  Returns the whole's outputs."""
    seeds = (np.arange(N, dtype=np.uint64) * 3 + 11).astype(np.uint32)

    def run(n, lane_offset, first, ref=None, misplaced=False):
        env = ea.VecEWN(n, lane_offset=lane_offset, seed_stride=N, **env_kw)
        env.reset(seeds=seeds[first:first + n])
        outs = dict(play(env, ref, misplaced))
        for k, t in end_state(env).items():
            outs["end " + k] = (t.clone(), 0)
        torch.cuda.synchronize()
        return outs

    whole = run(N, 0, 0)
    for n, lo in ((c, 0), (N - c, c)):
        ref = cut(whole, lo, n)
        got = run(n, lo, lo, ref)
        assert sorted(got) == sorted(whole)
        for k, (t, _) in got.items():
            assert same_bytes(t, ref[k]), ("the shard at lane %d differs from the whole" % lo, k)
    if differs is not None:
        ref = cut(whole, c, N - c)
        got = cut(run(N - c, 0, c, ref, True), 0, N - c)
        assert differs(got).numel() > 0 and not same_bytes(differs(got), differs(ref)), "the samples do not depend on the global lane id"
    return {k: t for k, (t, _) in whole.items()}


# ---------------------------------------------------------------- rollout_policy: ewn_step_k_policy and ewn_step_k_selfplay

def rollout_play(S, K, instance, opponent=None, deterministic=False):
    """instance "generic": column trajectory, totals, logits, noise and (where served) value, the opponent's action column;
    "trainer": what the fused trainers pass -- records from the initial observation on and the reward column, nothing else"""
    params = make_model(S, 5).flat_parameters()
    okw = dict(opponent_params=make_model(S, 9).flat_parameters(), opponent_deterministic=False, opponent_noise_key=77) if opponent else {}

    def play(env, ref, misplaced):
        n, f32 = env.N, dict(dtype=torch.float32, device="cuda")
        trainer = instance == "trainer"
        traj = env.alloc_rollout(K, layout="record", initial_obs=True) if trainer else env.alloc_rollout(K)
        totals, extra = None, {}
        if not trainer:
            totals = env.alloc_totals()
            extra = dict(logits=torch.zeros((K, n, 5), **f32), noise=torch.zeros((K, n, 5), **f32))
            if not opponent or env.supports_selfplay_rollout(value=True):
                extra["value"] = torch.zeros((K, n), **f32)
            if opponent:
                extra["opponent_action"] = torch.full((K, n, 3), -7, dtype=torch.int8, device="cuda")
        outs = {}
        for launch in range(LAUNCHES[S]):
            env.rollout_policy(K, params, traj=traj, totals=totals, deterministic=deterministic, noise_key=99, **extra, **okw)
            cols = dict(traj, **extra)               # the record layout's column entries are views of the records: compared twice, harmless
            for name, t in cols.items():
                outs["%d %s" % (launch, name)] = (t.clone(), 1)
        for name, t in (totals or {}).items():
            outs["totals " + name] = (t.clone(), 0)
        return outs
    return play


LAUNCHES = {5: 2, 7: 5}     # consecutive launches: a 7x7 game hardly ends within ten steps, and the last launch is to start past first episodes


def check_window(whole, launches, opponent=False):
    """as the sibling files assert it: the window saw terminations -- before its last launch, which therefore starts from carried state
    and, with auto-reset, from episodes past their first -- and a sampling opponent moved"""
    assert sum(int(whole["%d terminated" % launch].sum()) for launch in range(launches - 1)) > 0
    if opponent:
        assert bool((whole["0 opponent_action"][:, :, 0] > 0).any())


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("opp", ["minimax", "random"])
@pytest.mark.parametrize("instance", ["generic", "trainer"])
def test_rollout_policy(ea, S, opp, instance):
    """ewn_step_k_policy, K = 5, sampled actions, two launches (7x7: five): the shaped env with tolerance and auto-reset against the depth-3 minimax
    opponent (config 4's collector) and against RandomAgent; the generic instance with logits, value and noise, and the trainers'
    instance k_rollout_mlp<S, 0, NT, 1>.  The agent's noise word is keyed by lane_offset + game (csrc/ewn_policy_body.inc)."""
    env_kw = dict(board_size=S, opponent_policy=opp, max_depth=3, rng="philox", autoreset=True, philox_key=9487, **SHAPED)
    whole = whole_and_shards(ea, env_kw, rollout_play(S, 5, instance), differs=lambda o: o["0 action"])
    check_window(whole, LAUNCHES[S])
    if instance == "generic":
        assert int(whole["totals n_steps"].sum()) == LAUNCHES[S] * 5 * N_LANES and int(whole["totals n_episodes"].sum()) > 0


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("shaped", [False, True], ids=["plain", "shaped"])
@pytest.mark.parametrize("instance", ["generic", "trainer"])
def test_rollout_policy_against_a_sampling_model(ea, S, shaped, instance):
    """ewn_step_k_selfplay: a second parameter vector plays the opponent and samples under its own key; its noise word is
    pol_opp_noise_word(..., lane_offset + game, ...).  The generic instance plays the agent's argmax and records the opponent's
    action: at step 0 of the first launch every lane of the misplaced shard has the whole's board, dice and agent action, so an
    opponent action that differs there differs by the opponent's noise alone.  The trainers' instance (k_rollout_mlp_vs<S, NT, 1>)
    samples the agent as well and offers no opponent column: its inequality is the agent's."""
    env_kw = dict(board_size=S, opponent_policy="minimax", max_depth=6, rng="philox", autoreset=True, philox_key=31, **(SHAPED if shaped else {}))
    if instance == "generic":
        play, differs = rollout_play(S, 5, instance, opponent=True, deterministic=True), lambda o: o["0 opponent_action"][0]
    else:
        play, differs = rollout_play(S, 5, instance, opponent=True), lambda o: o["0 action"]
    whole = whole_and_shards(ea, env_kw, play, differs=differs)
    check_window(whole, LAUNCHES[S], opponent=instance == "generic")


# ---------------------------------------------------------------- eval_policy: ewn_policy_eval and ewn_policy_eval_vs

EVAL_STEPS = 200        # tests/test_gpu_selfplay.py's bound on an evaluation's length


def eval_play(S, K, opponent=None):
    """chunks of K steps until every lane of the whole is done (at most EVAL_STEPS steps); a shard runs the whole's number of chunks.
    opponent: None (the env's own), "argmax" or "sample" (a second parameter vector, ewn_policy_eval_vs)"""
    params = make_model(S, 5).flat_parameters()
    okw = dict(opponent_params=make_model(S, 9).flat_parameters(), opponent_deterministic=opponent == "argmax", opponent_noise_key=4321) if opponent else {}

    def play(env, ref, misplaced):
        n = env.N
        totals = env.alloc_totals()
        chunks = None if ref is None else ref["action"].shape[0] // K
        rows_a, rows_o = [], []
        while len(rows_a) < (chunks if chunks is not None else EVAL_STEPS // K):
            a = torch.full((K, n, 2), -7, dtype=torch.int8, device="cuda")
            o = torch.full((K, n, 3), -7, dtype=torch.int8, device="cuda")
            env.eval_policy(K, params, totals, action=a, **(dict(okw, opponent_action=o) if opponent else {}))
            rows_a.append(a)
            rows_o.append(o)
            if chunks is None and bool((env.done != 0).all()):
                break
        outs = {"action": (torch.cat(rows_a), 1)}
        if opponent:
            outs["opponent_action"] = (torch.cat(rows_o), 1)
        for name, t in totals.items():
            outs["totals " + name] = (t.clone(), 0)
        return outs
    return play


def check_evaluation(whole, opponent=False):
    assert bool((whole["end done"] != 0).all()) and int(whole["totals n_episodes"].sum()) == N_LANES
    assert int(whole["totals n_steps"].sum()) > N_LANES and whole["action"].shape[0] > 4          # more than one chunk: carried state
    if opponent:
        assert bool((whole["opponent_action"][:, :, 0] > 0).any())


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
@pytest.mark.parametrize("opp", ["random", "minimax"])
def test_eval_policy(ea, S, rng, opp):
    """ewn_policy_eval: the agent's argmax against the env's own RandomAgent / depth-3 minimax opponent, no auto-reset.  Nothing here
    samples by the lane id (the RandomAgent opponent draws from the lane's seeded stream): equality only."""
    env_kw = dict(board_size=S, opponent_policy=opp, max_depth=3, rng=rng, autoreset=False, philox_key=77)
    check_evaluation(whole_and_shards(ea, env_kw, eval_play(S, 4)))


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
@pytest.mark.parametrize("opponent", ["argmax", "sample"])
def test_eval_policy_against_a_model(ea, S, rng, opponent):
    """ewn_policy_eval_vs.  The sampling opponent's inequality is taken at step 0, where the misplaced shard's lanes have the whole's
    boards, dice and (argmax) agent actions: only the opponent's noise can differ."""
    env_kw = dict(board_size=S, opponent_policy="random", rng=rng, autoreset=False, philox_key=13)
    differs = (lambda o: o["opponent_action"][0]) if opponent == "sample" else None
    check_evaluation(whole_and_shards(ea, env_kw, eval_play(S, 4, opponent), differs=differs), opponent=True)


# ---------------------------------------------------------------- set_opponent_model: ewn_step_vs and ewn_step_k_vs

MODEL_ENVS = {"philox": dict(rng="philox", autoreset=True, philox_key=21), "mt19937": dict(rng="mt19937", autoreset=False)}


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_step_against_a_sampling_model(ea, S, rng):
    """ewn_step_vs, 12 steps driven by sample_legal_actions(t) (itself keyed by the env's lane_offset).  The misplaced shard is driven by
    the whole's recorded actions instead, so that at step 0 only the opponent's noise word (csrc/ewn_step_vs.hpp) can differ."""
    po = make_model(S, 9).flat_parameters()

    def play(env, ref, misplaced):
        oc = torch.zeros((env.N, 3), dtype=torch.int8, device="cuda")
        env.set_opponent_model(po, deterministic=False, noise_key=77, opponent_action=oc)
        outs = {}
        for t in range(12):
            act = ref["%d action" % t].contiguous() if misplaced else env.sample_legal_actions(t).clone()
            res = env.step(act)
            for name, x in zip(("action", "board", "dice", "reward", "terminated", "truncated", "info", "opponent_action"), (act,) + tuple(res) + (oc,)):
                outs["%d %s" % (t, name)] = (x.clone(), 0)
        return outs
    env_kw = dict(board_size=S, opponent_policy="random", **MODEL_ENVS[rng])
    whole = whole_and_shards(ea, env_kw, play, differs=lambda o: o["0 opponent_action"])
    assert sum(int(whole["%d terminated" % t].sum()) for t in range(12)) > 0
    assert sum(int((whole["%d opponent_action" % t][:, 0] > 0).sum()) for t in range(12)) > N_LANES


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
@pytest.mark.parametrize("agent", ["random", "sample", "minimax"])
def test_rollout_against_a_sampling_model(ea, S, rng, agent):
    """ewn_step_k_vs, K = 6, two launches (7x7: five), the stand-in agents (RandomAgent and action_space.sample() are keyed by the lane as well, the
    depth-3 minimax agent by nothing: for it the inequality is step 0's, the opponent's noise alone)"""
    po = make_model(S, 9).flat_parameters()
    K = 6

    def play(env, ref, misplaced):
        env.set_opponent_model(po, deterministic=False, noise_key=77)
        assert env.supports_rollout(agent, 3)
        traj, totals = env.alloc_rollout(K), env.alloc_totals()
        oc = torch.full((K, env.N, 3), -7, dtype=torch.int8, device="cuda")
        outs = {}
        for launch in range(LAUNCHES[S]):
            env.rollout(K, agent=agent, agent_max_depth=3, traj=traj, totals=totals, opponent_action=oc)
            for name, t in dict(traj, opponent_action=oc).items():
                outs["%d %s" % (launch, name)] = (t.clone(), 1)
        for name, t in totals.items():
            outs["totals " + name] = (t.clone(), 0)
        return outs
    env_kw = dict(board_size=S, opponent_policy="random", **MODEL_ENVS[rng])
    differs = (lambda o: o["0 opponent_action"][0]) if agent == "minimax" else (lambda o: o["0 opponent_action"])
    whole = whole_and_shards(ea, env_kw, play, differs=differs)
    check_window(whole, LAUNCHES[S], opponent=True)
    assert int(whole["totals n_steps"].sum()) > 0


# ---------------------------------------------------------------- the stateless calls

@pytest.mark.parametrize("S", [5, 7])
def test_predict_random_on_rows_is_the_rows_of_the_whole_call(ea, S):
    from ewn_gym_amd import vec_env as ve
    N, c = N_LANES, CUT
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=5)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) * 3 + 11).astype(np.uint32))
    env.rollout(3, agent="random")                      # mid-game boards
    b, d = env.board.clone(), env.dice.clone()
    whole = ve.predict_random(b, d, key=5, step=7)
    for lo, hi in ((0, c), (c, N)):
        assert torch.equal(ve.predict_random(b[lo:hi], d[lo:hi], key=5, step=7, lane_offset=lo), whole[lo:hi]), (lo, hi)
    assert not torch.equal(ve.predict_random(b[c:], d[c:], key=5, step=7, lane_offset=0), whole[c:])
    assert not torch.equal(ve.predict_random(b, d, key=5, step=8), whole)


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("fused", [False, True], ids=["staged", "fused"])
def test_selfplay_puct_on_two_shards_gives_the_whole_calls_records(ea, S, fused):
    """70 games: the calls on [0, 33) and [33, 70), the second with game_offset + 33, give the whole call's records -- the root noise
    (selfplay_noise) and the move's Philox draw (ewn_puct_play) both belong to the global game"""
    from tests.test_gpu_puct_selfplay import reset_positions, same_records
    M, c, off = 70, 33, 2 ** 32 + 5
    b, d = reset_positions(ea, S, M)
    params = make_model(S, 5, head_gain=1.0).flat_parameters()
    kw = dict(sims=6, max_plies=16, temp_plies=4, key=11, fused=fused)
    whole = ea.selfplay_puct(b, d, params, game_offset=off, **kw)
    parts = [ea.selfplay_puct(b[lo:hi], d[lo:hi], params, game_offset=off + lo, **kw) for lo, hi in ((0, c), (c, M))]
    joined = {k: torch.cat([p[k] for p in parts], 0 if whole[k].dim() == 1 else 1) for k in whole}
    same_records(joined, whole)
    assert int(whole["live"].sum()) > 4 * M and (S == 7 or bool((whole["winner"] != 0).any()))    # 16 plies end some 5x5 games
    misplaced = ea.selfplay_puct(b[c:], d[c:], params, game_offset=off, **kw)
    assert not torch.equal(misplaced["action"], whole["action"][:, c:])
