"""ModelAgent: a trained actor-critic behind the `predict(obs) -> (action, None)` surface of this package -- what
`model.predict(obs, deterministic=True)` is upstream (train.py:89, eval_A2C.py), ply by ply against an env.  The network runs in
libewn_hip.so (ewn_predict_policy: the rollout kernel's arithmetic on the matrix pipe), not in torch."""
import os

import numpy as np

from classical_policies.base import PolicyBase, obs_arrays


def _on_device(boards, dice, S, dev, other_size):
    """boards (M,S,S), dice (M,) device or host arrays -> int8 tensors [M, S, S] and [M] on dev; other_size: the agent's sentence about
    boards of another size, their shape left open"""
    import torch
    b = torch.as_tensor(np.asarray(boards) if not isinstance(boards, torch.Tensor) else boards)
    d = torch.as_tensor(np.asarray(dice) if not isinstance(dice, torch.Tensor) else dice)
    if b.numel() % (S * S) != 0 or b.shape[-1] != S:
        raise ValueError(other_size % list(b.shape))
    return b.to(dev).to(torch.int8).reshape(-1, S, S).contiguous(), d.to(dev).to(torch.int8).reshape(-1).contiguous()


class _PlainPolicyFn:
    """policy_fn of an agent whose predict_batch needs no step: named before ModelAgent in the bases, it replaces that one's keyed
    policy_fn"""

    def policy_fn(self):
        """(board, dice, t) -> actions, the callable tournament.evaluate takes"""
        return lambda b, d, t: self.predict_batch(b, d)


class ModelAgent(PolicyBase):
    def __init__(self, model_or_path, board_size=5, cube_layer=3, deterministic=True, key=0):
        """model_or_path: an a2c.ActorCritic, its flat fp32 parameter vector (ActorCritic.flat_parameters() order), or the path of a
        checkpoint of any of the trainers (tournament.load_policy).  deterministic=False samples from the policy, keyed by `key`."""
        import torch
        import ewn_gym_amd
        from ewn_gym_amd.tournament import flat_policy_params, load_policy
        self._ea = ewn_gym_amd
        self.board_size, self.cube_layer, self.deterministic, self.key = board_size, cube_layer, bool(deterministic), int(key)
        self._calls = 0
        n = ewn_gym_amd._lib.load().ewn_policy_param_count(board_size, cube_layer)
        if n < 0:
            raise ValueError("ModelAgent: no policy network for %dx%d boards with cube_layer %d" % (board_size, board_size, cube_layer))
        m = model_or_path
        if isinstance(m, (str, os.PathLike)):
            m = load_policy(m, board_size, cube_layer)         # raises ValueError on a checkpoint of another geometry
        if isinstance(m, torch.Tensor):
            params = m.detach().reshape(-1).to(torch.float32)
        else:
            if getattr(m, "S", board_size) != board_size:
                raise ValueError("ModelAgent: the model plays %dx%d boards, the agent is built for %dx%d" % (m.S, m.S, board_size, board_size))
            params = flat_policy_params(m)
        if params.numel() != n:
            raise ValueError("ModelAgent: %d parameters, a %dx%d actor-critic has %d" % (params.numel(), board_size, board_size, n))
        self.params = params.to("cuda").contiguous()

    def _on_device(self, boards, dice):
        S = self.board_size
        return _on_device(boards, dice, S, self.params.device, "ModelAgent: boards of shape %%s, the model plays %dx%d" % (S, S))

    def predict_batch(self, boards, dice, key=None, obs_id=None, return_logits=False, return_value=False):
        """boards (M,S,S), dice (M,) device or host arrays -> int8 (M,2) device tensor (with the logits / values if asked for).  A
        sampling agent draws under `key`; None: the agent's key advanced once per call, so that repeated calls differ."""
        b, d = self._on_device(boards, dice)
        if key is None:
            key = (self.key + self._calls * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
            self._calls += 1
        return self._ea.predict_policy(b, d, self.params, deterministic=self.deterministic, key=key, obs_id=obs_id,
                                       return_logits=return_logits, return_value=return_value, cube_layer=self.cube_layer)

    def predict(self, obs, **kwargs):
        b, d = obs_arrays(obs)
        return self.predict_batch(b, d)[0].cpu().numpy(), None     # np.array([flag, dir]), like SB3's model.predict

    def policy_fn(self):
        """(board, dice, t) -> actions, the callable tournament.evaluate takes; a sampling agent keys step t as
        key + 0x9E3779B97F4A7C15 * (t + 1), like the MCTS agent of tournament._policy"""
        return lambda b, d, t: self.predict_batch(b, d, key=(self.key + 0x9E3779B97F4A7C15 * (t + 1)) & 0xFFFFFFFFFFFFFFFF)


def _leaf_table(who, table, board_size, name="endgame_table"):
    """endgame_table= (or `name`=) of a searching agent: None, an EndgameTable, or the path of a saved one (loaded once), for the
    agent's boards"""
    from ewn_gym_amd.endgame import EndgameTable, _accept_table
    if table is None:
        return None
    return _accept_table(who, table, board_size, "the table is for %%dx%%d boards, the agent plays %dx%d" % (board_size, board_size),
                         name=name, load=EndgameTable.load)


class ValueSearchAgent(_PlainPolicyFn, ModelAgent):
    """The trained actor-critic searching one move ahead with its own value net (ewn_predict_lookahead): one agent move,
    the opponent's best reply under every dice, the critic at the next agent-to-move state -- plain expectiminimax, no pruning.  This
    project's counterpart of the reference's AlphaZeroMinimaxAgent (classical_policies/minimax.py:96-223: expectiminimax whose leaf
    is a network's value), on the network the trainers here produce.  Always deterministic: the first maximum of Q.  plies=2: two
    moves ahead (agent, reply, agent, reply, critic).  endgame_table (an ewn_gym_amd.EndgameTable or the path of a
    saved one): a leaf that the table covers is worth its exact value instead of the critic's."""

    def __init__(self, model_or_path, board_size=5, cube_layer=3, terminal_value=1.0, plies=1, endgame_table=None):
        if plies not in (1, 2):
            raise ValueError("ValueSearchAgent: plies must be 1 or 2, got %r" % (plies,))
        super().__init__(model_or_path, board_size=board_size, cube_layer=cube_layer, deterministic=True)
        self.terminal_value = float(terminal_value)
        self.plies = int(plies)
        self.endgame_table = _leaf_table("ValueSearchAgent", endgame_table, board_size)

    def predict_batch(self, boards, dice, return_q=False):
        """boards (M,S,S), dice (M,) device or host arrays -> int8 (M,2) device tensor (and the float32 (M,2,3) Q if asked for)"""
        b, d = self._on_device(boards, dice)
        return self._ea.predict_lookahead(b, d, self.params, terminal_value=self.terminal_value, return_q=return_q,
                                          cube_layer=self.cube_layer, plies=self.plies, endgame_table=self.endgame_table)


class PuctAgent(_PlainPolicyFn, ModelAgent):
    """The trained actor-critic behind a PUCT search of `sims` simulations (ewn_gym_amd.predict_puct): the policy head
    says where to look, the value head what a leaf is worth, chance nodes take the dice in a fixed stratified order.  This project's
    counterpart of the reference's AlphaZeroMCTSAgent (classical_policies/alpha_zero/MCTS.py), on the network the trainers here
    produce.  Always deterministic: a win on the board, else the most visited move.  sims=0 plays the first legal move unless one wins.
    endgame_table (an ewn_gym_amd.EndgameTable or the path of a saved one): a leaf that the table covers is worth its exact value
    instead of the value head's.  fused=True: the search of a batch is one kernel launch (ewn_puct_search, DESIGN.md
    4r) instead of 2 sims + 3: the same moves; not together with endgame_table.  leaves=2..32: the search of a batch is the one launch
    of ewn_puct_search_wide, up to that many leaves per tree and round: fewer rounds, other trees, so not always the
    moves of leaves=1; not together with endgame_table.  leaf_table (a table or the path of a saved one, loaded once): endgame_table's
    exact leaves with the search of a batch in the one launch of ewn_puct_search_eg; fused is not read; not together
    with endgame_table or leaves > 1."""

    def __init__(self, model_or_path, board_size=5, cube_layer=3, sims=64, c_puct=1.5, terminal_value=1.0, endgame_table=None, fused=False,
                 leaves=1, leaf_table=None):
        from ewn_gym_amd.search import _fused_table, _leaf_table_alone, _puct_numbers
        from ewn_gym_amd.wide import _NO_TABLE, _leaves_alone
        self.sims = _puct_numbers("PuctAgent", sims, c_puct, terminal_value)
        _fused_table("PuctAgent", fused, endgame_table)
        self.leaves = _leaves_alone("PuctAgent", leaves, endgame_table=(endgame_table is not None, _NO_TABLE))
        _leaf_table_alone("PuctAgent", leaf_table, endgame_table, self.leaves)
        self.fused = bool(fused)
        self.c_puct, self.terminal_value = float(c_puct), float(terminal_value)
        super().__init__(model_or_path, board_size=board_size, cube_layer=cube_layer, deterministic=True)
        self.endgame_table = _leaf_table("PuctAgent", endgame_table, board_size)
        self.leaf_table = _leaf_table("PuctAgent", leaf_table, board_size, name="leaf_table")

    def predict_batch(self, boards, dice, return_visits=False, return_q=False, return_value=False):
        """boards (M,S,S), dice (M,) device or host arrays -> int8 (M,2) device tensor (and the int32 (M,2,3) root visits, the float32
        (M,2,3) q and the float32 (M,) root value if asked for)"""
        b, d = self._on_device(boards, dice)
        return self._ea.predict_puct(b, d, self.params, sims=self.sims, c_puct=self.c_puct, terminal_value=self.terminal_value,
                                     return_visits=return_visits, return_q=return_q, return_value=return_value,
                                     cube_layer=self.cube_layer, endgame_table=self.endgame_table, fused=self.fused, leaves=self.leaves,
                                     leaf_table=self.leaf_table)


class EndgameAgent(_PlainPolicyFn, PolicyBase):
    """The exact move wherever an endgame table covers the position, `fallback`'s elsewhere.  table: an
    ewn_gym_amd.EndgameTable or the path of a saved one; fallback: any policy of this package with predict_batch(boards, dice).
    The fallback is asked for ALL rows of a batch and the exact actions are laid over its answer with one torch.where: no row
    selection, so no host synchronisation and the same launches whatever the positions are; a sampling fallback therefore draws
    for the covered rows too."""

    def __init__(self, table, fallback):
        import ewn_gym_amd
        from ewn_gym_amd.endgame import EndgameTable, _accept_table
        table = _accept_table("EndgameAgent", table, None, None, name="table", load=EndgameTable.load)
        if not callable(getattr(fallback, "predict_batch", None)):
            raise ValueError("EndgameAgent: fallback must offer predict_batch(boards, dice), got %s" % type(fallback).__name__)
        fs = getattr(fallback, "board_size", table.board_size)
        if fs != table.board_size:
            raise ValueError("EndgameAgent: the table is for %dx%d boards, the fallback plays %dx%d" % (
                table.board_size, table.board_size, fs, fs))
        self._ea = ewn_gym_amd
        self.table, self.fallback, self.board_size = table, fallback, table.board_size

    def predict_batch(self, boards, dice, return_covered=False):
        """boards (M,S,S), dice (M,) device or host arrays -> int8 (M,2) device tensor (and the bool (M,) covered mask if asked for)"""
        import torch
        S = self.board_size
        b, d = _on_device(boards, dice, S, self.table.table.device, "EndgameAgent: boards of shape %%s, the table is for %dx%d" % (S, S))
        exact, covered = self.table.lookup(b, d)
        acts = torch.where(covered[:, None], exact, self.fallback.predict_batch(b, d).to(torch.int8))
        return (acts, covered) if return_covered else acts

    def predict(self, obs, **kwargs):
        b, d = obs_arrays(obs)
        return self.predict_batch(b, d)[0].cpu().numpy(), None
