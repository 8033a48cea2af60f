"""PPO on the vectorised env: the `PPO` sub-command of the reference's train.py (train.py:39-49, 178-183).

The reference builds `stable_baselines3.PPO("MultiInputPolicy", env, batch_size=..., learning_rate=..., tanh)` and leaves
everything else at SB3's defaults.  SB3 is not vendored, not pinned and not installed here, so -- exactly as for
`ewn_gym_amd.a2c` -- its arithmetic is **parity unpinned**: this module follows SB3's documented PPO defaults
  * clipped surrogate objective, clip_range 0.2, no value-function clipping;
  * GAE(lambda 0.95), gamma 0.99, advantages normalised per minibatch;
  * n_epochs 10 passes over the rollout buffer in shuffled minibatches;
  * vf_coef 0.5, ent_coef 0, max_grad_norm 0.5, Adam(eps 1e-5), lr 3e-4;
  * the same two 64-64 tanh networks and action heads as A2C (`a2c.ActorCritic`),
and is tested for its own maths (tests/test_a2c_cpu.py: with one epoch, one minibatch and no normalisation the first PPO
step IS the A2C policy gradient), not against SB3.

What differs from SB3 by construction: the rollout buffer is n_steps x LANES (tens of thousands of lanes instead of
a handful of SubprocVecEnv workers), observations never leave the GPU, and `batch_size` counts samples of that
buffer (default: a quarter of it, i.e. four minibatches per epoch; train.py's `-b 8` would mean 10^5 optimiser steps
per rollout here).  Multi-GPU: as in A2C, ONE flattened-gradient all-reduce per optimiser step.

Two trainers: PPOTrainer (torch forward per step + ewn_step, eager autograd per minibatch) and FusedPPOTrainer (the same arithmetic in the
engine: ewn_step_k_policy + ewn_ppo_prepare / _shuffle / _grad / _apply, one hipGraph per update).
"""
import ctypes as C

import torch
import torch.nn as nn

from ._args import _ptr, _stream
from .a2c import A2CTrainer, FusedTrainer, all_reduce_gradients, n_step_returns


class PPOTrainer(A2CTrainer):
    algorithm = "PPO"

    def __init__(self, env, n_steps=32, batch_size=None, n_epochs=10, learning_rate=3e-4, gamma=0.99, gae_lambda=0.95,
                 clip_range=0.2, normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=None,
                 hidden=64, device=None, use_graph=True):
        super().__init__(env, n_steps=n_steps, learning_rate=learning_rate, gamma=gamma, gae_lambda=gae_lambda, ent_coef=ent_coef,
                         vf_coef=vf_coef, max_grad_norm=max_grad_norm, seed=seed, hidden=hidden, device=device, use_graph=use_graph)
        self.opt = torch.optim.Adam(self.model.parameters(), lr=learning_rate, eps=1e-5)
        total = n_steps * env.N
        self.batch_size = max(1, total // 4) if batch_size is None else int(batch_size)
        if self.batch_size > total:
            raise ValueError("batch_size %d exceeds the rollout buffer (n_steps x lanes = %d)" % (self.batch_size, total))
        self.n_epochs, self.clip_range, self.normalize_advantage = n_epochs, clip_range, normalize_advantage
        # minibatch order: the same on every rank is fine (each rank shuffles its own lanes), but it must not be the sampling stream
        self.perm_gen = torch.Generator(device=self.device)
        self.perm_gen.manual_seed((0 if seed is None else int(seed)) * 31 + 17)

    def ppo_loss(self, boards, dices, acts, old_logp, adv, ret):
        """(loss, policy_loss, value_loss, entropy, clip_fraction) of one minibatch -- SB3 PPO.train's inner body"""
        logp, ent, value = self.model.evaluate_actions(boards, dices, acts)
        if self.normalize_advantage and adv.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(logp - old_logp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - self.clip_range, 1.0 + self.clip_range)).mean()
        value_loss = torch.nn.functional.mse_loss(ret, value)
        entropy_loss = -ent.mean()
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        clip_frac = ((ratio - 1.0).abs() > self.clip_range).float().mean()
        return loss, policy_loss, value_loss, -entropy_loss, clip_frac

    def collect_and_update(self):
        env, T, N = self.env, self.n_steps, self.env.N
        self._collect()   # the n-step rollout, one hipGraph replay after the first (A2CTrainer._collect)
        boards = self._boards.reshape(T * N, env.S, env.S)
        dices, acts = self._dices.reshape(T * N), self._acts.reshape(T * N, 2)
        with torch.no_grad():
            _, _, last_value = self.model(env.board, env.dice)
            adv, ret = n_step_returns(self._rews, self._vals, self._dones, last_value, self.gamma, self.gae_lambda)
            old_logp, _, _ = self.model.evaluate_actions(boards, dices, acts)   # the behaviour policy's log-probabilities
        adv, ret = adv.reshape(-1), ret.reshape(-1)
        params = list(self.model.parameters())
        last = None
        for _ in range(self.n_epochs):
            perm = torch.randperm(T * N, device=self.device, generator=self.perm_gen)
            for lo in range(0, T * N - self.batch_size + 1, self.batch_size):   # whole minibatches only (SB3 drops nothing: its sizes divide)
                idx = perm[lo:lo + self.batch_size]
                loss, pl, vl, en, cf = self.ppo_loss(boards[idx], dices[idx], acts[idx], old_logp[idx], adv[idx], ret[idx])
                self.opt.zero_grad(set_to_none=False)
                loss.backward()
                all_reduce_gradients(params)
                nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.opt.step()
                last = (loss, pl, vl, en)
        self.num_timesteps += T * N
        stats = torch.stack([last[0].detach(), last[1].detach(), last[2].detach(), last[3].detach(), self._rews.mean(), self._dones.sum()])
        self._last_stats = stats
        return stats


class FusedPPOTrainer(FusedTrainer):
    """PPOTrainer's update with the whole loop in the engine: the n-step rollout is ONE kernel (ewn_step_k_policy), then
    ewn_ppo_prepare (behaviour-policy log-probabilities, values, GAE advantages and returns of every sample), ewn_ppo_shuffle (every
    epoch's minibatch order, on the device) and per minibatch ewn_ppo_grad (value pass, policy pass, reduction) + ewn_ppo_apply
    (global-norm clip + Adam) -- no torch operator on the training path; with several ranks one all-reduce of the flat gradient between
    grad and apply per minibatch.  Same knobs, defaults and arithmetic as PPOTrainer; the flat parameters and the loop are
    a2c.FusedTrainer's, the Adam state lives in two more flat tensors and the step count in a device int32 (which also keys the shuffle:
    a replayed graph draws a new order every update)."""

    algorithm = "PPO"
    _use_instead = ": use PPOTrainer"

    def __init__(self, env, n_steps=32, batch_size=None, n_epochs=10, learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=None, use_graph=True, opponent=None,
                 opponent_update_every=100, opponent_deterministic=False):
        from . import _lib
        super().__init__(env, n_steps, seed, use_graph, opponent, opponent_update_every, opponent_deterministic)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.step = torch.zeros(1, dtype=torch.int32, device=self.device)   # Adam steps taken; also keys the shuffle
        total = self.n_steps * env.N
        self.batch_size = max(1, total // 4) if batch_size is None else int(batch_size)
        if not 1 <= self.batch_size <= total:
            raise ValueError("batch_size %d outside [1, n_steps x lanes = %d]" % (self.batch_size, total))
        self.n_epochs = int(n_epochs)
        self.n_minibatches = total // self.batch_size          # whole minibatches only, as PPOTrainer
        self.hyper = _lib.EwnPpoHyper(float(gamma), float(gae_lambda), float(clip_range), float(vf_coef), float(ent_coef), float(max_grad_norm),
                                      float(learning_rate), 0.9, 0.999, 1e-5, int(bool(normalize_advantage)), int(self.world))
        nscr = _lib.check(self.lib.ewn_ppo_scratch_bytes(C.byref(env.cfg), self.n_steps, self.batch_size), "ewn_ppo_scratch_bytes")
        self.scratch = torch.zeros(int(nscr), dtype=torch.uint8, device=self.device)
        self.samples = torch.zeros((total, 4), dtype=torch.float32, device=self.device)   # {old log pi, adv, ret, old value} per sample
        self.perm = torch.zeros((self.n_epochs, total), dtype=torch.int32, device=self.device)
        self.shuffle_key = ((0 if seed is None else int(seed)) * 31 + 17) & 0xFFFFFFFFFFFFFFFF

    def launches_per_update(self):
        """kernel launches of one update: rollout, prepare, shuffle, then per minibatch 3 (grad) + 1 (apply)"""
        return 3 + 4 * self.n_epochs * self.n_minibatches

    def _launch(self):
        from ._lib import check
        env, lib = self.env, self.lib
        K, total, B = self.n_steps, self.n_steps * env.N, self.batch_size
        cfg, hp = C.byref(env.cfg), C.byref(self.hyper)
        rec, params, samples, grad, scratch = _ptr(self.traj["record"]), _ptr(self.params), _ptr(self.samples), _ptr(self.grad), _ptr(self.scratch)
        env.rollout_policy(K, self.params, traj=self.traj, noise_key=self.noise_key, **self._opponent_kwargs())
        check(lib.ewn_ppo_prepare(cfg, K, rec, _ptr(self.traj["reward"]), params, hp, samples, _stream()), "ewn_ppo_prepare")
        check(lib.ewn_ppo_shuffle(total, self.n_epochs, self.shuffle_key, _ptr(self.step), _ptr(self.perm), _stream()), "ewn_ppo_shuffle")
        base = self.perm.data_ptr()
        for e in range(self.n_epochs):
            for m in range(self.n_minibatches):
                idx = C.c_void_p(base + 4 * (e * total + m * B))
                check(lib.ewn_ppo_grad(cfg, K, rec, samples, params, hp, idx, B, grad, scratch, _stream()), "ewn_ppo_grad")
                self._all_reduce_grad()                       # per optimiser step
                check(lib.ewn_ppo_apply(cfg, params, _ptr(self.exp_avg), _ptr(self.exp_avg_sq), _ptr(self.step), grad, hp,
                                        _ptr(self.grad_norm), _stream()), "ewn_ppo_apply")

    def stats_dict(self):
        """PPOTrainer's keys (the last minibatch's losses) plus clip_fraction, approx_kl (mean of (r - 1) - log r) and grad_norm"""
        g = self.grad[-8:].tolist()
        n = float(self.batch_size * self.world)
        pl, en, cf, kl, vl = g[0] / n, g[1] / n, g[2] / n, g[3] / n, g[4] / n
        return {"loss": pl + self.hyper.vf_coef * vl - self.hyper.ent_coef * en, "policy_loss": pl, "value_loss": vl, "entropy": en,
                "mean_reward": float(self.traj["reward"].mean()), "episodes": int(self.traj["terminated"].sum()),
                "clip_fraction": cf, "approx_kl": kl, "grad_norm": float(self.grad_norm)}

    def _state(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step, "noise_key": self.noise_key,
                "shuffle_key": self.shuffle_key}

    def _load_state(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step.copy_(sd["step"])
        self.noise_key, self.shuffle_key = int(sd["noise_key"]), int(sd["shuffle_key"])   # the run continues with its own streams

    def _load_foreign(self, path, sd):
        """a checkpoint of PPOTrainer: its module state and Adam state mapped onto the flat vectors"""
        algo = sd.get("algorithm", "A2C")
        if algo != self.algorithm:
            raise ValueError("checkpoint %s was written by the %s trainer, this is the %s trainer" % (path, algo, self.algorithm))
        self.model.load_state_dict(sd["model"])   # copies into the views of self.params
        state = sd["opt"]["state"]
        off, step = 0, 0
        for i, p in enumerate(self.model.parameters()):
            st = state.get(i)
            sl = slice(off, off + p.numel())
            self.exp_avg[sl].copy_(st["exp_avg"].reshape(-1) if st else 0.0)
            self.exp_avg_sq[sl].copy_(st["exp_avg_sq"].reshape(-1) if st else 0.0)
            if st:
                step = int(st["step"])
            off += p.numel()
        self.step.fill_(step)
