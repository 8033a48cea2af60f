"""Drop-in for the reference's `classical_policies` package
(classical_policies/__init__.py:1-4): same class names, constructor signatures and
`predict(obs, **kw) -> (action, None)` contract; every search runs in libewn_hip.so.

AlphaZeroAgent / AlphaZeroMinimaxAgent are out of scope (un-vendored weights, SURVEY
section 2 rows 12-14): they exist as names that raise on construction.  The search whose
leaf is a network's value exists for the networks trained here: ValueSearchAgent (one-ply
lookahead on the actor-critic's own value net, ewn_predict_lookahead) and PuctAgent (a PUCT search on
both of its heads, ewn_gym_amd.predict_puct: the counterpart of AlphaZeroMCTSAgent), beside ModelAgent.
EndgameAgent plays the exact move where an endgame table covers the position and a fallback policy elsewhere.
PlayoutSearchAgent is PuctAgent's tree without a network: uniform priors, random playouts at the leaves (plain MCTS with chance nodes).
"""
from classical_policies.base import PolicyBase
from classical_policies.random_policy import RandomAgent
from classical_policies.minimax import ExpectiMinimaxAgent, AlphaZeroMinimaxAgent
from classical_policies.mcts import MctsAgent
from classical_policies.alpha_zero import AlphaZeroAgent
from classical_policies.model import EndgameAgent, ModelAgent, PuctAgent, ValueSearchAgent
from classical_policies.playout_search import PlayoutSearchAgent

# the names BASELINE.json's north_star uses
RandomPolicy = RandomAgent
MiniMaxPolicy = ExpectiMinimaxAgent
MCTSPolicy = MctsAgent

__all__ = ["PolicyBase", "RandomAgent", "ExpectiMinimaxAgent", "MctsAgent", "AlphaZeroAgent", "AlphaZeroMinimaxAgent",
           "RandomPolicy", "MiniMaxPolicy", "MCTSPolicy", "ModelAgent", "ValueSearchAgent", "PuctAgent", "EndgameAgent",
           "PlayoutSearchAgent"]
