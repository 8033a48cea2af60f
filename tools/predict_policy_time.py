"""Timing of the stateless policy call.

  python tools/predict_policy_time.py [--runs 5]

Per board (5x5, 7x7) and batch (M = 1, 1 024, 65 536): predict_policy (ewn_predict_policy, deterministic, actions only, and with logits and
value) against the torch forward it replaces (model.act(deterministic=True)), alternated in the same process on the same observations.
Each figure is the median of `--runs` timed windows after warm-up, a window being `launches` back-to-back calls between two device
events with a synchronisation before and after; microseconds per call.  Prints one JSON line per row.  No pass bar: the comparison
is against torch in the same run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ewn_gym_amd as ea  # noqa: E402
from ewn_gym_amd.a2c import ActorCritic  # noqa: E402


def observations(S, M):
    """M observations of real play: a 16-step random-agent rollout of min(M, 4 096) games, repeated up to M"""
    N = min(M, 4096)
    env = ea.VecEWN(N, board_size=S, opponent_policy="random", rng="philox", autoreset=True, seed_stride=N, philox_key=7)
    env.reset(seeds=(np.arange(N, dtype=np.uint64) + 9487).astype(np.uint32))
    traj = env.alloc_rollout(16)
    env.rollout(16, agent="random", traj=traj)
    idx = torch.arange(M, device="cuda") % (16 * N)
    return traj["board"].reshape(-1, S, S)[idx].contiguous(), traj["dice"].reshape(-1)[idx].contiguous()


def timed(fn, launches, runs):
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / launches)
    return [round(statistics.median(out), 2), round(min(out), 2), round(max(out), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    for S in (5, 7):
        torch.manual_seed(9)
        model = ActorCritic(S, 6).cuda()
        params = model.flat_parameters()
        for M in (1, 1024, 65536):
            b, d = observations(S, M)
            fns = {"predict_policy": lambda: ea.predict_policy(b, d, params),
                   "predict_policy logits+value": lambda: ea.predict_policy(b, d, params, return_logits=True, return_value=True),
                   "torch model.act": lambda: model.act(b, d, deterministic=True)}
            launches = 200 if M <= 1024 else 50
            for fn in fns.values():                                       # warm-up
                for _ in range(10):
                    fn()
            rows = {}
            for _ in range(2):                                            # alternate the three, keep the later pass
                for name, fn in fns.items():
                    rows[name] = timed(fn, launches, a.runs)
            same = bool(torch.equal(fns["predict_policy"](), fns["torch model.act"]()[0]))
            print(json.dumps({"board": S, "M": M, "us_per_call_median_min_max": rows, "actions_equal_torch": same}), flush=True)


if __name__ == "__main__":
    main()
