"""The rows of the stateless flat Monte-Carlo and RandomAgent queries that the engine defines itself: a finished observation
(six -1 win counters, action (0, 0)) and an observation without a legal move ((0, 0)).  The oracle plays such rows out, so the
contract is the engine's own; the live rows beside them stay pinned to the oracle.  One geometry per state width and playout
kind: byte-per-cube playouts, generic playouts on one and on two words of cube positions, the mask-free state of 9x9."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import pyoracle as po  # noqa: E402
from tests.test_gpu_parity import _random_positions, cpu, ea  # noqa: E402,F401

GEOMS = [(5, 3), (7, 4), (8, 5), (9, 3)]


def _positions(S, L):
    """Four live positions, then four finished ones: TOP_LEFT home, BOTTOM_RIGHT home, no negative cube, no positive cube."""
    b, d = _random_positions(S, L, 8, 900 + S + L, max_steps=30)
    done = b[4:].copy()
    done[0][done[0] == 1] = 0
    done[0, S - 1, S - 1] = 1      # TOP_LEFT already home
    done[1][done[1] == -1] = 0
    done[1, 0, 0] = -1             # BOTTOM_RIGHT already home
    done[2][done[2] < 0] = 0       # no negative cube left
    done[3][done[3] > 0] = 0       # no positive cube left
    b = np.concatenate([b[:4], done])
    d[4] = 1                       # the dice names the cube on the bottom-right corner: TOP_LEFT has no move
    return b, d


@pytest.mark.parametrize("S,L", GEOMS)
def test_predict_mcts_live_rows_vs_oracle_and_finished_rows(ea, S, L):
    b, d = _positions(S, L)
    acts, wins = ea.predict_mcts(b, d, num_simulations=5, num_env_copies=1, key=31 * S + L, cube_layer=L)
    oa, ow = po.predict_mcts(b[:4], d[:4], num_simulations=5, num_env_copies=1, key=31 * S + L, cube_layer=L)
    assert np.array_equal(cpu(wins)[:4], ow) and np.array_equal(cpu(acts)[:4], oa)
    assert (cpu(wins)[4:] == -1).all()
    assert (cpu(acts)[4:] == 0).all()


@pytest.mark.parametrize("S,L", GEOMS)
def test_predict_random_on_finished_rows(ea, S, L):
    b, d = _positions(S, L)
    acts = cpu(ea.predict_random(b, d, key=17 * S + L, step=3, cube_layer=L))
    la, n, _, _, _ = po.legal_actions(b, d, player=1, cube_layer=L)
    assert n[4] == 0 and n[7] == 0 and (n[:4] > 0).all()      # both kinds of row are present
    for m in range(8):
        if n[m] == 0:
            assert tuple(acts[m]) == (0, 0), m
        else:
            assert any(tuple(acts[m]) == tuple(la[m, i]) for i in range(n[m])), m
