"""PlayoutSearchAgent: a PUCT tree search with uniform priors and random playouts at the leaves (ewn_gym_amd.predict_playout_search,
DESIGN.md 4t) -- plain MCTS with chance nodes, the classical player between MctsAgent (flat Monte-Carlo: playouts under each root
move, no tree) and PuctAgent (the same tree on a trained network).  The reference has no such agent; the constructor takes
(cube_layer, board_size) first like its classical ones."""
import numpy as np

from classical_policies.base import PolicyBase, obs_arrays


class PlayoutSearchAgent(PolicyBase):
    def __init__(self, cube_layer, board_size, sims=64, playouts=64, c_puct=1.5, seed=None, endgame_table=None):
        """sims simulations per move, `playouts` random playouts per leaf; seed: of the playouts' key (None: fresh entropy).
        endgame_table: an EndgameTable for the agent's boards or the path of a saved one (loaded once): the leaves it covers are
        worth their exact value and run no playouts (ewn_gym_amd.predict_playout_search_exact)."""
        import ewn_gym_amd
        from ewn_gym_amd.playout_search import KEY_PLY, _numbers
        self._ea, self._ply = ewn_gym_amd, KEY_PLY
        self.cube_layer, self.board_size = cube_layer, board_size
        self.sims, self.playouts, _, _ = _numbers("PlayoutSearchAgent", sims, playouts, c_puct, 0, 0)
        self.c_puct = float(c_puct)
        if ewn_gym_amd._lib.load().ewn_puct_tree_bytes(board_size, cube_layer, self.sims) < 0:
            raise ValueError("PlayoutSearchAgent: no search tree for %dx%d boards with cube_layer %d (served: cube_layer 3 on 5x5 and 7x7)" % (
                board_size, board_size, cube_layer))
        from classical_policies.model import _leaf_table
        self.endgame_table = _leaf_table("PlayoutSearchAgent", endgame_table, board_size)
        self.key = int(np.random.SeedSequence(seed).generate_state(2, np.uint32).view(np.uint64)[0])
        self._calls = 0

    def predict_batch(self, boards, dice, key=None, obs_id0=0, return_visits=False, return_q=False, return_value=False, return_leaf_counts=False):
        """boards (M,S,S), dice (M,) device or host arrays -> int8 (M,2) device tensor (and the int32 (M,2,3) root visits, the float32
        (M,2,3) q and the float32 (M,) root value if asked for; return_leaf_counts, with an endgame_table only: and the int32 (M,2)
        leaves the table and the playouts valued).  The playouts draw under `key`; None: the agent's key advanced once per call,
        so that repeated calls differ."""
        import torch
        S = self.board_size
        b = torch.as_tensor(np.asarray(boards) if not isinstance(boards, torch.Tensor) else boards)
        d = torch.as_tensor(np.asarray(dice) if not isinstance(dice, torch.Tensor) else dice)
        if b.numel() % (S * S) != 0 or b.shape[-1] != S:
            raise ValueError("PlayoutSearchAgent: boards of shape %s, the agent plays %dx%d" % (list(b.shape), S, S))
        b, d = b.to("cuda").to(torch.int8).reshape(-1, S, S).contiguous(), d.to("cuda").to(torch.int8).reshape(-1).contiguous()
        if key is None:
            key = (self.key + self._calls * self._ply) & 0xFFFFFFFFFFFFFFFF
            self._calls += 1
        if self.endgame_table is not None:
            return self._ea.predict_playout_search_exact(b, d, self.endgame_table, sims=self.sims, playouts=self.playouts, c_puct=self.c_puct,
                                                         key=key, obs_id0=obs_id0, return_visits=return_visits, return_q=return_q,
                                                         return_value=return_value, return_leaf_counts=return_leaf_counts,
                                                         cube_layer=self.cube_layer)
        if return_leaf_counts:
            raise ValueError("PlayoutSearchAgent: return_leaf_counts goes with an endgame_table")
        return self._ea.predict_playout_search(b, d, sims=self.sims, playouts=self.playouts, c_puct=self.c_puct, key=key, obs_id0=obs_id0,
                                               return_visits=return_visits, return_q=return_q, return_value=return_value,
                                               cube_layer=self.cube_layer)

    def predict(self, obs, **kwargs):
        b, d = obs_arrays(obs)
        return self.predict_batch(b, d)[0].cpu().numpy(), None

    def policy_fn(self):
        """(board, dice, t) -> actions, the callable tournament.evaluate takes: episode m is observation id m, step t draws under
        key + KEY_PLY * (t + 1) -- the MCTS agent's scheme of tournament._policy, with a stride of its own"""
        return lambda b, d, t: self.predict_batch(b, d, key=(self.key + self._ply * (t + 1)) & 0xFFFFFFFFFFFFFFFF)
