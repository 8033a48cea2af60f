"""SearchDistillTrainer (ewn_gym_amd/distill.py): one update is the public calls composed -- rollout_policy, predict_lookahead,
lookahead_targets, sup_grad, ewn_a2c_apply -- bit for bit; reproducibility, the other board and the two-move search, checkpoints and
the SEARCH sub-command of train_a2c end to end."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


def make_env(ea, N, S=5, key=77):
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_tolerance=5,
                    shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=key)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 11).astype(np.uint32))
    return env


def bits(x):
    return x.view(torch.int32)


def test_one_update_is_the_public_calls_composed(ea):
    from ewn_gym_amd._lib import EwnA2cHyper, check
    from ewn_gym_amd.distill import SearchDistillTrainer
    from ewn_gym_amd.vec_env import _ptr, _stream
    N, K = 64, 3
    tr = SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=5)
    assert tr.algorithm == "SEARCH" and tr.plies == 1 and tr.terminal_value == 1.0
    params = tr.params.clone()
    sq = torch.zeros_like(params)
    tr.collect_and_update()
    # by hand, on a second, identically seeded env
    env = make_env(ea, N)
    traj = env.alloc_rollout(K, layout="record", initial_obs=True)
    env.rollout_policy(K, params, traj=traj, noise_key=tr.noise_key)
    assert torch.equal(traj["record"], tr.traj["record"])
    b = traj["obs_board"][:K].reshape(K * N, 5, 5).contiguous()
    d = traj["obs_dice"][:K].reshape(K * N).contiguous()
    _, q = ea.predict_lookahead(b, d, params, terminal_value=1.0, return_q=True)
    tp, tv, w = ea.lookahead_targets(q, 0.0)
    grad = ea.sup_grad(b, d, tp, tv, params, weight=w, pi_coef=1.0, vf_coef=0.5)
    assert torch.equal(bits(grad), bits(tr.grad))
    hp = EwnA2cHyper(0.0, 0.5, 0.0, 0.5, 7e-4, 0.99, 1e-5, 1)
    norm = torch.zeros(1, device="cuda")
    check(env.lib.ewn_a2c_apply(C.byref(env.cfg), _ptr(params), _ptr(sq), _ptr(grad), C.byref(hp), _ptr(norm), _stream()), "ewn_a2c_apply")
    assert torch.equal(bits(params), bits(tr.params)) and torch.equal(bits(sq), bits(tr.sq_avg))
    assert float(norm) == tr.stats_dict()["grad_norm"] > 0
    assert torch.equal(tr.model.flat_parameters(), tr.params)          # the module views the flat vector
    assert tr.num_timesteps == K * N


def test_reproducible_and_sane(ea):
    from ewn_gym_amd.distill import SearchDistillTrainer
    N, K = 64, 3
    out = []
    for _ in range(2):
        tr = SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=9)
        for it in range(5):
            tr.collect_and_update()
            assert tr.num_timesteps == (it + 1) * K * N
            st = tr.stats_dict()
            assert all(math.isfinite(v) for v in st.values()), st
            assert 0.0 <= st["agreement"] <= 1.0 and 0.0 < st["live_fraction"] <= 1.0 and st["grad_norm"] > 0 and st["entropy"] > 0
            assert set(st) >= {"policy_loss", "value_loss", "entropy", "agreement", "grad_norm", "live_fraction"}
        out.append(tr.params.clone())
    assert torch.equal(bits(out[0]), bits(out[1]))


@pytest.mark.parametrize("S,N,K,plies", [(7, 33, 2, 1), (5, 8, 2, 2)])
def test_other_board_and_two_moves(ea, S, N, K, plies):
    from ewn_gym_amd.distill import SearchDistillTrainer
    tr = SearchDistillTrainer(make_env(ea, N, S=S), n_steps=K, plies=plies, temperature=0.5 if plies == 1 else 0.0, seed=2)
    before = tr.params.clone()
    tr.collect_and_update()
    st = tr.stats_dict()
    assert all(math.isfinite(v) for v in st.values()) and st["live_fraction"] > 0 and not torch.equal(before, tr.params)
    assert bool(torch.isfinite(tr.params).all())
    assert tr.learn(K * N)["grad_norm"] > 0 and tr.num_timesteps == 2 * K * N


def test_checkpoints(ea, tmp_path):
    from classical_policies import ValueSearchAgent
    from envs import EinsteinWuerfeltNichtEnv
    from ewn_gym_amd import tournament
    from ewn_gym_amd.a2c import FusedA2CTrainer
    from ewn_gym_amd.distill import SearchDistillTrainer
    N, K = 64, 3
    tr = SearchDistillTrainer(make_env(ea, N), n_steps=K, plies=2, terminal_value=0.75, seed=4)
    tr.collect_and_update()
    path = str(tmp_path / "search.pt")
    tr.best_score = 0.25
    tr.save(path)
    other = SearchDistillTrainer(make_env(ea, N), n_steps=K, seed=99)
    assert other.plies == 1 and not torch.equal(other.params, tr.params)
    other.load(path)
    assert torch.equal(bits(other.params), bits(tr.params)) and torch.equal(bits(other.sq_avg), bits(tr.sq_avg))
    assert other.terminal_value == 0.75 and other.plies == 2 and other.num_timesteps == K * N and other.best_score == 0.25
    assert torch.equal(other.model.flat_parameters(), tr.params)
    model = tournament.load_policy(path)
    assert torch.equal(model.flat_parameters(), tr.params)
    agent = ValueSearchAgent(model, board_size=5)
    env = EinsteinWuerfeltNichtEnv(board_size=5, seed=3)
    obs, _ = env.reset(seed=3)
    for _ in range(60):
        action, _ = agent.predict(obs)
        obs, _, terminated, truncated, _ = env.step(action)
        if terminated or truncated:
            break
    assert terminated or truncated                                       # one whole episode
    a2c = FusedA2CTrainer(make_env(ea, N), n_steps=K, seed=1)
    p_a2c = str(tmp_path / "a2c.pt")
    a2c.save(p_a2c)
    with pytest.raises(ValueError, match="not written by the search-distillation trainer"):
        other.load(p_a2c)
    with pytest.raises(ValueError, match="fused A2C"):
        a2c.load(path)


def test_train_a2c_search_end_to_end(ea, tmp_path):
    """one epoch of the SEARCH sub-command with tiny numbers, in a fresh child process"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SEARCH", "--num_envs", "64", "--n_steps", "3", "--epoch_num", "1",
                        "--timesteps_per_epoch", "384", "--eval_episode_num", "16", "--eval_opponent", "random", "--plies", "1",
                        "--temperature", "0.5", "--terminal_value", "1.0", "--save_dir", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert any(x.get("trainer") == "SearchDistillTrainer" for x in lines)
    ep = [x for x in lines if "epoch" in x]
    assert len(ep) == 1 and ep[0]["timesteps"] == 384 and 0.0 <= ep[0]["agreement"] <= 1.0 and math.isfinite(ep[0]["policy_loss"])
    sd = torch.load(os.path.join(str(tmp_path), "best.pt"), map_location="cpu", weights_only=True)
    assert sd["algorithm"] == "SEARCH" and sd["fused"] and sd["plies"] == 1 and sd["terminal_value"] == 1.0
