"""The slot-task K-step kernel's derived LDS tables (one fused entry per position byte: legal mask, destinations and real cells of
a cube's moves for either side; a replier cube's search setup side by side) against the CPU oracle.  Each block builds them from the
table image it has copied in, so every board size, heuristic image and depth variant feeds the builder something else.
Every byte of every row on a window of at most 300 lanes, at the smallest lane counts at which the launcher picks the kernel
(65 537 games at two lanes per game, 131 073 at one); the window ends on the last game, so the grid's partial block builds and uses
its tables too.  With auto-reset on, a case passes only if more episodes ended inside the window than it has lanes: the launches
of a case are as many as the oracle needs for that at the case's K (counted on the oracle alone, before any GPU run)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_rollout import _rollout_vs_oracle  # noqa: E402

N2, N1, W = 65537, 131073, 300      # games at two lanes per game / at one; lanes checked

MM = dict(opponent_policy="minimax", rng="philox")

# id -> (games, window, K, launches, arguments)
CASES = {
    # 64-bit masks, the 48-byte reply entries, and the image padding of the larger boards
    "6x6-record-two-lanes": (N2, W, 12, 2, dict(MM, layout="record", board_size=6, max_depth=3, philox_key=606)),
    "6x6-record-one-lane": (N1, W, 12, 2, dict(MM, layout="record", board_size=6, max_depth=3, philox_key=616)),
    # real cells up to 63 in the chosen root's packed move
    "8x8": (N2, W, 10, 3, dict(MM, layout="record", board_size=8, max_depth=3, philox_key=808)),
    # other images and the other image variant feed the builder; max_depth 1 and 2 leave the search by its early return
    "min_dist": (N2, W, 12, 2, dict(MM, layout="record", max_depth=3, heuristic="min_dist", philox_key=31)),
    "attk": (N2, W, 12, 2, dict(MM, layout="record", max_depth=3, heuristic="attk", philox_key=33)),
    "max_depth=1": (N2, W, 12, 2, dict(MM, layout="record", max_depth=1, philox_key=1)),
    "max_depth=2": (N2, W, 12, 2, dict(MM, layout="record", max_depth=2, philox_key=2)),
    "max_depth=4": (N2, W, 12, 2, dict(MM, layout="record", max_depth=4, philox_key=4)),
    # the opponent's move of the max_depth 5 / 6 instances
    "max_depth=5": (N2, 96, 4, 3, dict(MM, layout="record", max_depth=5, philox_key=5)),
    # the numpy-dice instance of the kernel: the same boundary code in another instantiation, lanes freeze
    "mt19937-no-autoreset": (N1, W, 8, 1, dict(opponent_policy="minimax", rng="mt19937", autoreset=False, layout="record", max_depth=3)),
    # destinations of 255 and illegal-move terminations out of the fused entry
    "sample-agent": (N2, W, 16, 2, dict(MM, agent="sample", layout="record", max_depth=3, philox_key=314)),
    # captures on both sides, own-cube captures, auto-resets; the record instance and the generic-trajectory instance
    "default-record": (N2, W, 24, 2, dict(MM, layout="record", max_depth=3, philox_key=2025)),
    "default-columns": (N2, W, 24, 2, dict(MM, layout="columns", max_depth=3, philox_key=2026)),
}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ewn_gym_amd
    return ewn_gym_amd


@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_on_the_last_lanes(ea, case):
    N, w, K, launches, kw = CASES[case]
    n = _rollout_vs_oracle(ea, N, N - w, N, K, launches, **kw)
    if kw.get("autoreset", True):
        assert n > w, (case, n)
