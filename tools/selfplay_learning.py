"""The learning signal of self-play, measured: a policy trained by FusedA2CTrainer(opponent="self") for a fixed small budget, then its
argmax against the argmax of its own INITIAL parameters in ewn_policy_eval_vs over 1 024 episodes (MT19937-compat dice, seeds 0..1023).

    python tools/selfplay_learning.py [--updates 400] [--lanes 8192] [--every 50]

A win is a score above 0.  An opponent that forfeits by an illegal move ends the episode with reward 0 (envs/ewn.py:469-473): not a win.
DESIGN.md section 4g holds the measured figures and why no test asserts a bar on them."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic, FusedA2CTrainer  # noqa: E402
from ewn_gym_amd.tournament import evaluate, wilson  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--updates", type=int, default=400)
ap.add_argument("--lanes", type=int, default=8192)
ap.add_argument("--every", type=int, default=50)
a = ap.parse_args()
N, key = a.lanes, 9487
env = ea.VecEWN(N, opponent_policy="random", rng="philox", shaped=True, reward=10.0, illegal_move_reward=-1.0, illegal_move_tolerance=10,
                shaped_refresh_on_reset=True, autoreset=True, seed_stride=N, philox_key=key)
env.reset(seeds=(np.arange(N, dtype=np.uint64) + key).astype(np.uint32))
tr = FusedA2CTrainer(env, n_steps=5, learning_rate=7e-4, seed=1, opponent="self", opponent_update_every=a.every)
first = ActorCritic(5, 6).cuda()
first.load_flat_parameters(tr.params.clone())
for _ in range(a.updates):
    tr.collect_and_update()
torch.cuda.synchronize()
r = evaluate({"kind": "mlp", "model": tr.model}, {"kind": "mlp", "model": first}, num=1024, rng="mt19937")
assert r["engine"] == "ewn_policy_eval_vs"
losses, forfeits = int((r["scores"] < 0).sum()), int((r["scores"] == 0).sum())
lo, hi = wilson(r["wins"], 1024)
print("self-play, %d updates x %d lanes: trained vs initial parameters over 1024 episodes: wins %d, losses %d, opponent forfeits (score 0) "
      "%d; win rate %.4f (Wilson 95%% %.4f-%.4f)" % (a.updates, N, r["wins"], losses, forfeits, r["win_rate"], lo, hi))
