"""Data-parallel ranks rehearsed in one process, one after the other (tests/test_gpu_data_parallel.py).

A fused trainer calls `_all_reduce_grad()` once per optimiser step, between its gradient kernel and its apply kernel; with several
ranks that call sums the flat gradient (loss sums in the tail included) over the ranks.  The ranks here never run at the same time, so
the sum is built by replay, which the trainers allow because they are bit-reproducible: pass p builds fresh ranks, gives them the
recorded sums at the optimiser steps before p -- so that they arrive at step p in the state real ranks would have there -- and at
step p only keeps each rank's local gradient.  The kept gradients are added and recorded, and pass p + 1 gets one step further.  The
pass after the last recorded step runs with every sum known: its ranks end where real ranks would."""


def record_gradients(trainer):
    """replace `trainer._all_reduce_grad` by a recorder -> the list that receives a copy of `trainer.grad` at every optimiser step"""
    seen = []
    trainer._all_reduce_grad = lambda: seen.append(trainer.grad.clone())
    return seen


def _exchange(trainer, rank, sums, local):
    step = [0]

    def all_reduce():
        s = step[0]
        step[0] += 1
        if s < len(sums):
            trainer.grad.copy_(sums[s])
        elif s == len(sums):
            local[rank] = trainer.grad.clone()      # and `grad` stays local: what this pass does from here on is thrown away
    return all_reduce


def rehearse(build, run, steps):
    """build() -> a list of fresh rank trainers, the same ones at every call; run(ranks) drives them through the same `steps` optimiser
    steps each, in any order, and may return something.  Returns (ranks, sums, returned): the ranks of the last pass, in which every
    optimiser step applied the summed gradient, the `steps` sums, and what run() returned in that pass."""
    sums = []
    for p in range(steps + 1):
        ranks = build()
        local = [None] * len(ranks)
        for r, tr in enumerate(ranks):
            tr._all_reduce_grad = _exchange(tr, r, sums, local)
        returned = run(ranks)
        if p == steps:
            if any(g is not None for g in local):
                raise AssertionError("run() took more than the %d optimiser steps it was rehearsed for" % steps)
            return ranks, sums, returned
        if any(g is None for g in local):
            raise AssertionError("a rank never reached optimiser step %d" % p)
        total = local[0].clone()
        for g in local[1:]:
            total += g
        sums.append(total)
