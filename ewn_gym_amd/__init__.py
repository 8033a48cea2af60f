"""ewn_gym_amd: MI355X-native vectorised EinStein-wuerfelt-nicht env step + opponent search.

Only what the hot path needs: csrc/ (HIP kernels + C ABI), the ctypes binding, and
VecEWN (the batched engine the drop-in `envs` / `classical_policies` packages wrap).
"""
from ._lib import EwnError, INFO_MESSAGES, LIB_PATH  # noqa: F401
from .vec_env import VecEWN, apply_action, evaluate, legal_actions, playout_wins, predict_mcts, predict_minimax, predict_random  # noqa: F401
from .search import (lookahead_expand, lookahead_reduce, lookahead_targets, predict_lookahead, predict_policy, sup_grad,  # noqa: F401
                     predict_puct, puct_advance, puct_begin, puct_result, puct_tree_views, puct_play, selfplay_noise, selfplay_outcomes,
                     selfplay_puct, puct_search)
from .endgame import EndgameTable  # noqa: F401
from .games import selfplay_puct_games  # noqa: F401
from .playout_search import playout_search, predict_playout_search  # noqa: F401
from .wide import puct_search_wide  # noqa: F401
from .playout_exact import playout_search_exact, predict_playout_search_exact  # noqa: F401
from .puct_exact import puct_search_exact  # noqa: F401
from .games_exact import selfplay_puct_games_exact  # noqa: F401
from .arena import arena_puct, arena_puct_games  # noqa: F401

__all__ = ["VecEWN", "EwnError", "INFO_MESSAGES", "legal_actions", "apply_action", "playout_wins", "evaluate", "predict_minimax", "predict_random",
           "predict_mcts", "predict_policy", "predict_lookahead", "lookahead_expand", "lookahead_reduce", "lookahead_targets", "sup_grad", "EndgameTable",
           "predict_puct", "puct_begin", "puct_advance", "puct_result", "puct_tree_views",
           "puct_play", "selfplay_noise", "selfplay_outcomes", "selfplay_puct", "puct_search", "selfplay_puct_games",
           "playout_search", "predict_playout_search", "puct_search_wide", "playout_search_exact", "predict_playout_search_exact",
           "puct_search_exact", "selfplay_puct_games_exact", "arena_puct", "arena_puct_games"]
