"""tests/data_parallel.py, the replay driver of tests/test_gpu_data_parallel.py, on a toy trainer whose two-rank run is computed by
hand.  The toy has what the driver touches of a fused trainer: a flat `grad` with a tail, an `_all_reduce_grad()` between gradient and
apply, and an update that divides the summed gradient by the world size.  Last, the one piece of the shard contract that runs without a
GPU: selfplay_puct's root noise belongs to the global game."""
import pytest

torch = pytest.importorskip("torch")

from tests.data_parallel import record_gradients, rehearse  # noqa: E402


class Toy:
    """rank r's local gradient at w is a[r] * w + b[r], the tail holds (r + 1) * sum(w); apply: w -= lr * grad / world.  Every number
    of the sequence below is a dyadic fraction: float64 holds them exactly"""
    A = (1.0, 2.0)
    B = ((1.0, 0.0), (0.0, 1.0))

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.params = torch.tensor([1.0, 2.0], dtype=torch.float64)
        self.grad = torch.zeros(3, dtype=torch.float64)
        self.updates = 0

    def _all_reduce_grad(self):
        raise AssertionError("the driver must replace the collective")

    def collect_and_update(self):
        self.grad[:2] = self.A[self.rank] * self.params + torch.tensor(self.B[self.rank], dtype=torch.float64)
        self.grad[2] = (self.rank + 1) * self.params.sum()
        self._all_reduce_grad()
        self.params -= 0.5 * self.grad[:2] / self.world
        self.updates += 1


# by hand, w0 = (1, 2):                 rank 0          rank 1          sum             w after
#   step 0                              (2, 2)          (2, 5)          (4, 7)          (0, 0.25)
#   step 1                              (1, 0.25)       (0, 1.5)        (1, 1.75)       (-0.25, -0.1875)
#   step 2                              (0.75, -0.1875) (-0.5, 0.625)   (0.25, 0.4375)  (-0.3125, -0.296875)
# tails: 3 + 6, 0.25 + 0.5, -0.4375 - 0.875
SUMS = [[4.0, 7.0, 9.0], [1.0, 1.75, 0.75], [0.25, 0.4375, -1.3125]]
FINAL = [-0.3125, -0.296875]


def run_all(steps):
    def run(ranks):
        for tr in ranks:                      # rank 0 to its end, then rank 1: they never meet
            for _ in range(steps):
                tr.collect_and_update()
        return "done"
    return run


def test_the_rehearsal_is_the_hand_computed_two_rank_run():
    built = []

    def build():
        built.append([Toy(0, 2), Toy(1, 2)])
        return built[-1]
    ranks, sums, returned = rehearse(build, run_all(3), 3)
    assert returned == "done" and len(built) == 4 and ranks is built[-1]      # three recording passes and the final one, fresh ranks each
    assert [s.tolist() for s in sums] == SUMS
    for tr in ranks:
        assert tr.params.tolist() == FINAL and tr.updates == 3
        assert tr.grad.tolist() == SUMS[2]                                    # the last step's summed gradient, tail included
    # a recording pass leaves the ranks of that pass on their own: pass 0's rank 0 took three purely local steps
    alone = Toy(0, 2)
    alone._all_reduce_grad = lambda: None
    for _ in range(3):
        alone.collect_and_update()
    assert built[0][0].params.tolist() == alone.params.tolist() != FINAL


def test_fewer_steps_give_the_prefix_and_the_order_of_the_ranks_does_not_matter():
    def run(ranks):
        for _ in range(2):
            for tr in reversed(ranks):        # interleaved, rank 1 first
                tr.collect_and_update()
    ranks, sums, returned = rehearse(lambda: [Toy(0, 2), Toy(1, 2)], run, 2)
    assert returned is None and [s.tolist() for s in sums] == SUMS[:2]
    assert all(tr.params.tolist() == [-0.25, -0.1875] for tr in ranks)


def test_a_run_of_another_length_is_refused():
    with pytest.raises(AssertionError, match="never reached optimiser step 2"):
        rehearse(lambda: [Toy(0, 2), Toy(1, 2)], run_all(2), 3)
    with pytest.raises(AssertionError, match="more than the 2 optimiser steps"):
        rehearse(lambda: [Toy(0, 2), Toy(1, 2)], run_all(3), 2)


def test_record_gradients_keeps_a_copy_per_step():
    tr = Toy(0, 1)
    seen = record_gradients(tr)
    for _ in range(2):
        tr.collect_and_update()
    assert [g.tolist() for g in seen] == [[2.0, 2.0, 3.0], [1.0, 1.0, 1.0]]   # w1 = (1, 2) - 0.5 * (2, 2) = (0, 1); g = w + (1, 0)
    assert seen[0].data_ptr() != tr.grad.data_ptr()


def test_selfplay_noise_rows_belong_to_global_games():
    """the root noise of selfplay_puct: row m is the noise of game game_offset + m, whatever call draws it and across a block border"""
    from ewn_gym_amd.search import NOISE_BLOCK, selfplay_noise
    for first in (0, 5, NOISE_BLOCK - 20, 2 ** 32 + 5):
        whole = selfplay_noise(70, 1.0, 11, first, 3, device="cpu")
        assert whole.shape == (70, 6) and whole.dtype == torch.float32 and bool((whole > 0).all())
        a, b = selfplay_noise(33, 1.0, 11, first, 3, device="cpu"), selfplay_noise(37, 1.0, 11, first + 33, 3, device="cpu")
        assert torch.equal(torch.cat([a, b]), whole) and whole.is_contiguous() and b.is_contiguous()
        assert not torch.equal(selfplay_noise(37, 1.0, 11, first, 3, device="cpu"), b)        # other games, other noise
        assert not torch.equal(selfplay_noise(70, 1.0, 11, first, 4, device="cpu"), whole)    # other ply
        assert not torch.equal(selfplay_noise(70, 1.0, 12, first, 3, device="cpu"), whole)    # other key
