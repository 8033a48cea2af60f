"""PUCT priors and leaf values on saturated network outputs (pu_evaluate, csrc/ewn_puct.hpp): the cases, on the host.
A network that puts nearly all its mass on illegal moves leaves every legal softmax product in the fp32 denormals or at zero; the
definition -- the product normalised over the legal edges, that is the softmax of l_f + l_r over the legal edges -- is as well
defined there as anywhere.  This file builds the positions, the logit vectors and the values that tests/test_gpu_puct_saturated.py
feeds to every PUCT kernel, and checks on the host (a) that every constructed position has the legal-edge set it is named after, by
tests/test_gpu_puct.py's edges(), (b) that the cases have teeth: a numpy float32 transcription of the arithmetic pu_evaluate had
before it looked at its sum (maxima over all entries, normalisation over the legal ones) leaves P_TOL against prior64 or is NaN on
pairs of each saturated group and stays within P_TOL on the controls, and (c) that the float64 reference is finite and sums to 1 on
every pair and that the Model of the definition runs every pair to the end of a budget of 12, with, in every saturated group,
evaluated nodes whose float64 legal mass before the normalisation lies below 2^-126, the smallest normal fp32 number.
Non-finite logits and a NaN value are outside the contract and are not among the cases.  No kernel runs here."""
import itertools

import numpy as np
import pytest

pytest.importorskip("torch")

from tests.test_gpu_puct import F, P_TOL, Model, degenerate, edges, prior64  # noqa: E402

SIMS = 12
GS = (24, 44, 48, 52, 56, 64, 80, 88, 96, 104, 112, 128, 250)
VALUES = (0.0, 0.25, -0.5, 1.0, -1.0, 1.5, -64.0, 3e38, -3e38, 1e-40, float("inf"), float("-inf"))
TERMINAL_VALUES = (1.0, 0.75, 10.0)
SATURATED = ("A", "B", "C", "D")
OFFSET = 8192
TINY = 2.0 ** -126


# ---------------------------------------------------------------- 1. positions

def position_specs(S):
    """[(name, {(x, y): cube}, dice, the legal edges a = 3 f + r)]: the agent moves right (r 0), down (r 1) or down-right (r 2), so
    a cube on the last row can only go right and one on the last column only down.  No move captures, wins or leaves the board"""
    e = S - 1
    opp = {(0, e): -1, (0, e - 1): -4}
    return [("one legal edge", {(e, 1): 5, (0, e): -1, (1, e): -3}, 3, [0]),                  # test_gpu_puct_fused.py's planted row 5
            ("three legal edges", {(1, 1): 3, **opp}, 3, [0, 1, 2]),                           # one cube, named by the dice
            ("two constrained cubes", {(e, 0): 2, (e, 2): 5, **opp}, 3, [0, 3]),               # either side of the dice, both on the last row
            ("different directions", {(e, 1): 2, (1, e): 5, **opp}, 3, [0, 4]),                # the last row and the last column
            ("mixed", {(e, 1): 2, (1, 1): 5, **opp}, 3, [0, 3, 4, 5])]                         # the last row and the interior


def positions(S):
    """(boards int8 [5, S, S], dice int8 [5]) of position_specs, as boards_of lays them out"""
    sp = position_specs(S)
    b = np.zeros((len(sp), S, S), np.int8)
    for i, (_, cells, _, _) in enumerate(sp):
        for (x, y), v in cells.items():
            b[i, x, y] = v
    return b, np.array([d for _, _, d, _ in sp], np.int8)


# ---------------------------------------------------------------- 2. logit vectors

def vectors():
    """[(group, g, float32 [5])]: integers of magnitude at most 256 (group D: 8192 more), exact in bf16 and fp32"""
    out = []
    for g in GS:
        heads = []
        for i in range(3):                                     # (A) one direction at -g
            r = [0, 0, 0]
            r[i] = -g
            heads.append(("A", r))
        for i, j, _ in itertools.permutations(range(3)):       # (B) two directions at -g and -g + 1: a ratio of e between them
            r = [0, 0, 0]
            r[i], r[j] = -g, -g + 1
            heads.append(("B", r))
        out += [(grp, g, [0, 0] + r) for grp, r in heads]
        for flags in ([0, -g], [-g, 0]):                       # (C) the flag head saturated as well: the heads multiply
            out += [("C", g, flags + r) for _, r in heads]
        if g in (24, 104):                                     # (D) a common offset
            out += [("D", g, [OFFSET + x for x in [0, 0] + r]) for grp, r in heads if grp == "B"]
    out += [("E", 0, [0.5, -0.25, 1.0, -2.0, 0.75]), ("E", 0, [-1.5, 0.25, 0.125, 2.0, -0.5])]        # (E) ordinary controls
    return [(grp, g, np.array(v, F)) for grp, g, v in out]


VECTORS = vectors()


def mass64(logits, kind, one):
    """prior64's sum over the legal edges before it normalises"""
    l = logits.astype(np.float64)
    pf, pr = np.exp(l[:2] - l[:2].max()), np.exp(l[2:] - l[2:].max())
    pf, pr = pf / pf.sum(), pr / pr.sum()
    return sum((pr[a % 3] if one else pf[a // 3] * pr[a % 3]) for a in range(6) if kind[a])


def former32(logits, kind, one):
    """the arithmetic pu_evaluate had for every node, operation for operation in np.float32 with denormals kept: both softmaxes
    relative to the maximum of all their entries, the product per edge, the sum over the legal edges in index order, the division"""
    l = logits.astype(F)
    with np.errstate(all="ignore"):
        mf = l[1] if l[1] > l[0] else l[0]
        f0, f1 = np.exp(F(l[0] - mf)), np.exp(F(l[1] - mf))
        sf = F(f0 + f1)
        mr = l[3] if l[3] > l[2] else l[2]
        mr = l[4] if l[4] > mr else mr
        r = [np.exp(F(l[2] - mr)), np.exp(F(l[3] - mr)), np.exp(F(l[4] - mr))]
        sr = F(F(r[0] + r[1]) + r[2])
        pf, pr = [F(f0 / sf), F(f1 / sf)], [F(x / sr) for x in r]
        raw = np.zeros(6, F)
        for a in range(6):
            if kind[a]:
                raw[a] = pr[a % 3] if one else F(pf[a // 3] * pr[a % 3])
        s = F(0)
        for a in range(6):
            s = F(s + raw[a])
        return np.array([F(raw[a] / s) if kind[a] else F(0) for a in range(6)], F)


_TEETH = {}


def teeth(S):
    """per (position, vector) of the constructed positions: max |former32 - prior64|, NaN where former32 is"""
    if S not in _TEETH:
        b, d = positions(S)
        err = np.zeros((len(b), len(VECTORS)))
        for i in range(len(b)):
            kind, _, one = edges(b[i], int(d[i]))
            for k, (_, _, lg) in enumerate(VECTORS):
                err[i, k] = np.abs(former32(lg, kind, one).astype(np.float64) - prior64(lg, kind, one)).max()
        _TEETH[S] = err
    return _TEETH[S]


def failing_pairs(S):
    """[(position, vector)] of groups A, B and C on which the former arithmetic leaves P_TOL or is NaN"""
    err = teeth(S)
    return [(i, k) for k, (grp, _, _) in enumerate(VECTORS) if grp in "ABC" for i in range(err.shape[0]) if not err[i, k] <= P_TOL]


# ---------------------------------------------------------------- (a) legal-edge sets

@pytest.mark.parametrize("S", [5, 7])
def test_every_position_has_the_legal_edges_it_is_named_after(S):
    b, d = positions(S)
    for i, (name, _, _, want) in enumerate(position_specs(S)):
        kind, b1, one = edges(b[i], int(d[i]))
        assert not degenerate(b[i]) and (b[i] < 0).any() and b[i][0, 0] == 0, name
        assert np.nonzero(kind)[0].tolist() == want and (kind[kind != 0] == 2).all(), (name, kind)
        assert one == (int((b[i] > 0).sum()) == 1), name
    k0, k1 = edges(b[2], 3)[0], edges(b[3], 3)[0]
    assert [a % 3 for a in np.nonzero(k0)[0]] == [0, 0] and [a % 3 for a in np.nonzero(k1)[0]] == [0, 1]      # one direction; two


def test_the_vectors():
    groups = [grp for grp, _, _ in VECTORS]
    assert {grp: groups.count(grp) for grp in "ABCDE"} == {"A": 39, "B": 78, "C": 234, "D": 12, "E": 2}
    for grp, g, lg in VECTORS:
        assert lg.dtype == F and lg.shape == (5,) and np.isfinite(lg).all()
        if grp in "ABC":
            assert np.array_equal(lg, np.round(lg)) and np.abs(lg).max() == g <= 256
        if grp == "D":
            assert np.array_equal(lg, np.round(lg)) and lg.max() == OFFSET and lg.min() == OFFSET - g
    assert len(VALUES) == 12 and not any(np.isnan(v) for v in VALUES) and F(1e-40) > 0 and np.isfinite(F(3e38))


# ---------------------------------------------------------------- (b) teeth

@pytest.mark.parametrize("S", [5, 7])
def test_the_former_arithmetic_fails_on_every_saturated_group_and_holds_on_the_controls(S):
    err = teeth(S)
    fails = failing_pairs(S)
    for grp in "ABC":
        cols = [k for k, v in enumerate(VECTORS) if v[0] == grp]
        bad = [(i, k) for i, k in fails if k in cols]
        nan = sum(bool(np.isnan(err[i, k])) for i, k in bad)
        worst = max((err[i, k] for i, k in bad if not np.isnan(err[i, k])), default=0.0)
        print("S=%d group %s: %d of %d pairs leave P_TOL, %d of them NaN, the largest finite error %.3g" % (
            S, grp, len(bad), err.shape[0] * len(cols), nan, worst))
        assert bad and nan > 0
        assert min(VECTORS[k][1] for _, k in bad) >= 44                            # ... and not before the arithmetic runs out
    for k, (grp, _, _) in enumerate(VECTORS):
        if grp == "E":
            assert (err[:, k] <= P_TOL).all(), err[:, k]
    small = [k for k, (grp, g, _) in enumerate(VECTORS) if grp in "AB" and g <= 80]
    assert (err[:, small] <= P_TOL).all()                                          # one head at e^-80 is still healthy


# ---------------------------------------------------------------- (c) the reference and the Model

@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("group", list("ABCDE"))
def test_the_reference_is_finite_and_the_model_runs_every_pair(S, group):
    b, d = positions(S)
    c, inv_tv, tiny, nodes = F(1.5), F(1), 0, 0
    for k, (grp, g, lg) in enumerate(VECTORS):
        if grp != group:
            continue
        for i in range(len(b)):
            V = F(VALUES[(k + i) % len(VALUES)])
            m = Model(b[i], d[i], SIMS)
            gp = np.zeros((SIMS + 1, 6), F)
            for _ in range(SIMS + 1):
                j = m.pending
                if j >= 0:                                     # every evaluated node of every tree
                    kind, _, one = edges(m.t["board"][j], int(m.t["dice"][j]))
                    p64 = prior64(lg, kind, one)
                    assert np.isfinite(p64).all() and abs(p64.sum() - 1.0) <= 1e-12 and not p64[kind == 0].any(), (i, k, j, p64)
                    tiny += mass64(lg, kind, one) < TINY
                    nodes += 1
                    gp[j] = p64.astype(F)
                with np.errstate(all="ignore"):
                    m.advance(lg, V, c, inv_tv, gp)
            assert m.pending == -1 and m.done == SIMS and int(m.t["n"][0].sum()) == SIMS and not m.degenerate, (i, k)
            assert np.isfinite(m.t["w"]).all() and (np.abs(m.t["w"]) <= m.t["n"]).all()
    print("S=%d group %s: %d evaluated nodes, %d of them with a float64 legal mass below 2^-126" % (S, group, nodes, tiny))
    assert nodes > 0 and (tiny > 0) == (group in SATURATED)
