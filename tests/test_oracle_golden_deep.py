"""The CPU oracle and the two Python models of the kernel searches against the UNMODIFIED reference (oracle/gen_golden_deep.py) where
the deep search code lives: max_depth 1-6 on the constructed positions of tests/test_gpu_search_d5.py, few-cube endgames included
(G15), trajectories against minimax(4-6) opponents on 5x5 .. 8x8 (G16), and heuristics, searches and trajectories on 9x9 .. 11x11
(G18).  G17 (the evaluation loop with a deep agent) is a GPU matter: tests/test_gpu_golden_deep.py.

G15 stores no boards.  make_positions() regenerates them from the oracle's own play and their sha256 is compared: when a change to
the oracle moves the positions the hash test FAILS (it never skips) and the fixture is regenerated where the reference is."""
import hashlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import test_d5_closed_form_model as d5m
from tests import test_gpu_search_keys as d3m
from tests.test_gpu_search_d5 import M_POS, SIZES, positions
from tests.test_oracle_golden import _check_traj

THIN = 2 * M_POS // 3
OTHER = ("min_dist", "attk", "two_min_dist")
HEURS = ("hybrid",) + OTHER


def position_hash(S):
    b, d = positions(S)
    return hashlib.sha256(b.astype(np.int8).tobytes() + d.astype(np.int8).tobytes()).hexdigest()


_G15 = {}


def g15_size(golden, S):
    """one board size of G15 with its compact form (oracle/gen_golden_deep.py) written out:
    {"sha256": of the positions, "res": {"depth/heuristic": {"idx": [position, ...], "out": [[a0, a1, value hex], ...]}}}"""
    if S not in _G15:
        g = golden("g15_deep_search.json")
        assert (g["n"], g["thin"]) == (M_POS, THIN)
        g = g["sizes"][str(S)]
        res = {}
        for key, r in g["res"].items():
            rec = [r["out"][i:i + 3] for i in range(0, len(r["out"]), 3)]
            res[key] = {"idx": [i for lo, hi in r["idx"] for i in range(lo, hi)],
                        "out": [[int(c[0]) // 3, int(c[0]) % 3, g["values"][int(c[1:], 36)]] for c in rec]}
        _G15[S] = {"sha256": g["sha256"], "res": res}
    return _G15[S]


def expand_traj(rec):
    """a trajectory record in G6's format: every step's board rebuilt from the cells the step changed"""
    board, steps = list(rec["board0"]), []
    for a0, a1, dice, r, term, trunc, msg, changed in rec["steps"]:
        for cell, cube in zip(changed[::2], changed[1::2]):
            board[cell] = cube
        steps.append({"a": [a0, a1], "board": list(board), "dice": dice, "r": r, "term": term, "trunc": trunc, "msg": msg})
    return {**rec, "steps": steps}


def dense(cells, S):
    """the S x S int8 board of [cell, cube, cell, cube, ...]"""
    b = np.zeros(S * S, np.int8)
    b[cells[::2]] = cells[1::2]
    return b.reshape(S, S)


@pytest.mark.parametrize("S", SIZES)
def test_g15_positions_are_the_ones_the_reference_searched(golden, S):
    assert position_hash(S) == g15_size(golden, S)["sha256"], \
        "make_positions(%d, %d) moved: regenerate tests/golden/g15_deep_search.json with oracle/gen_golden_deep.py" % (S, M_POS)


@pytest.mark.parametrize("S", SIZES)
def test_g15_layout_and_record_counts(golden, S):
    """which positions carry a golden, per key: a fixture that shrank fails here"""
    res = g15_size(golden, S)["res"]
    thinned, mid = list(range(THIN, M_POS)), list(range(64))
    assert res["5/hybrid"]["idx"] == list(range(M_POS))
    assert sorted(res["6/hybrid"]["idx"]) == mid + thinned
    for depth in (1, 2, 3, 4):
        assert res["%d/hybrid" % depth]["idx"] == thinned
    for h in OTHER:
        for depth in (3, 4, 5):
            assert sorted(res["%d/%s" % (depth, h)]["idx"]) == mid + thinned[:128]
        assert res["6/%s" % h]["idx"] == thinned[128:176]
    assert all(len(r["idx"]) == len(r["out"]) for r in res.values())
    hyb = sum(len(r["out"]) for k, r in res.items() if k.endswith("/hybrid"))
    oth = sum(len(r["out"]) for k, r in res.items() if not k.endswith("/hybrid"))
    assert hyb >= 1024 + 405 + 4 * 342 and oth >= 3 * (3 * 192 + 48), (hyb, oth)


@pytest.mark.parametrize("S", SIZES)
def test_g15_oracle_equals_the_reference(golden, S):
    """po.predict_minimax on every record: action and root-value bits"""
    g = g15_size(golden, S)
    assert position_hash(S) == g["sha256"]
    b, d = positions(S)
    n = {"hybrid": 0, "other": 0}
    for key, r in g["res"].items():
        depth, h = key.split("/")
        idx = np.array(r["idx"])
        acts, vals, _ = po.predict_minimax(b[idx], d[idx], int(depth), h)
        for j, (a0, a1, v) in enumerate(r["out"]):
            assert acts[j].tolist() == [a0, a1], (S, key, int(idx[j]), b[idx[j]], d[idx[j]])
            assert float(vals[j]).hex() == float.fromhex(v).hex(), (S, key, int(idx[j]), float(vals[j]).hex(), v)
        n["hybrid" if h == "hybrid" else "other"] += len(r["out"])
    assert n["hybrid"] >= 1024 + 405 + 4 * 342 and n["other"] >= 3 * (3 * 192 + 48), n


_SEEN = {}


def _models_against_the_reference(golden, S):
    """d5_closed_form on 5/hybrid and 6/hybrid, d3_model on 3/hybrid, against the reference's records; -> the cases they met"""
    if S in _SEEN:
        return _SEEN[S]
    g = g15_size(golden, S)
    assert position_hash(S) == g["sha256"]
    b, d = positions(S)
    seen5, seen3 = dict.fromkeys(d5m.CASES, 0), dict.fromkeys(d3m.CASES, 0)
    for key, model in (("5/hybrid", lambda i: d5m.d5_closed_form(b[i], int(d[i]), 5, seen5)),
                       ("6/hybrid", lambda i: d5m.d5_closed_form(b[i], int(d[i]), 6, seen5)),
                       ("3/hybrid", lambda i: d3m.d3_model(b[i], int(d[i]), seen3))):
        r = g["res"][key]
        for i, (a0, a1, v) in zip(r["idx"], r["out"]):
            a, val = model(i)
            assert (int(a[0]), int(a[1])) == (a0, a1), (S, key, i, b[i], d[i])
            assert float(val).hex() == float.fromhex(v).hex(), (S, key, i, float(val).hex(), v)
    _SEEN[S] = seen5, seen3
    return _SEEN[S]


@pytest.mark.parametrize("S", SIZES)
def test_g15_python_models_equal_the_reference(golden, S):
    """the closed form of d5c_search and the key model of d3_search, pinned to the reference itself and not only through the oracle"""
    seen5, seen3 = _models_against_the_reference(golden, S)
    print("S=%d d5_closed_form %s" % (S, seen5))
    print("S=%d d3_model %s" % (S, seen3))


def test_g15_positions_contain_every_case_of_both_models(golden):
    """every situation the kernels treat on a path of their own occurs among the positions that carry a reference result"""
    tot5, tot3 = dict.fromkeys(d5m.CASES, 0), dict.fromkeys(d3m.CASES, 0)
    for S in SIZES:
        seen5, seen3 = _models_against_the_reference(golden, S)
        for c in tot5:
            tot5[c] += seen5[c]
        for c in tot3:
            tot3[c] += seen3[c]
    print("d5_closed_form", tot5)
    print("d3_model", tot3)
    assert all(tot5[c] > 0 for c in d5m.CASES), [c for c in d5m.CASES if tot5[c] == 0]
    assert all(tot3[c] > 0 for c in d3m.CASES), [c for c in d3m.CASES if tot3[c] == 0]


def _traj_groups(recs):
    """trajectories of one configuration together, in the order of their first record"""
    out = {}
    for r in recs:
        out.setdefault((r["S"], r["L"], r["opp"], r.get("depth"), r.get("heuristic")), []).append(r)
    return out


G16_GROUPS = [(5, 3, 6, "hybrid", 4), (6, 3, 5, "hybrid", 4), (6, 3, 4, "attk", 4), (6, 3, 5, "two_min_dist", 2), (7, 3, 5, "hybrid", 3),
              (7, 3, 4, "two_min_dist", 3), (8, 3, 4, "min_dist", 3), (8, 3, 5, "hybrid", 2), (8, 3, 6, "hybrid", 1)]


def g16_trajs(golden):
    return [expand_traj(r) for r in golden("g16_deep_traj.json")]


def test_g16_trajectories_deep_minimax_opponent(golden):
    g = g16_trajs(golden)
    groups = _traj_groups(g)
    assert [(S, L, dep, h, len(recs)) for (S, L, opp, dep, h), recs in groups.items()] == G16_GROUPS
    for rec in g:
        assert rec["opp"] == "minimax" and len(rec["steps"]) > 0 and rec["steps"][-1]["term"]
        _check_traj(rec, "minimax", max_depth=rec["depth"], heuristic=rec["heuristic"])
    assert sum(len(r["steps"]) for r in g) >= 200


LARGE = [(9, 3), (10, 4), (11, 5)]


_G18 = {}


def _g18(golden, S, L):
    """one geometry of G18 with its compact form written out in the layout of G12:
    {"eval": [{"board", "hybrid", ...}], "minimax": [{"board", "dice", "res": {key: [a0, a1, value hex]}}], "traj": [as G6]}"""
    if (S, L) not in _G18:
        grp = [g for g in golden("g18_large_boards.json") if (g["S"], g["L"]) == (S, L)]
        assert len(grp) == 1
        g = grp[0]
        ev = [dict(zip(("board", "hybrid", "min_dist", "two_min_dist", "attk"), [dense(r[0], S).reshape(-1).tolist()] + r[1:]))
              for r in g["eval"]]
        mm = g["minimax"]
        recs = [{"board": ev[p]["board"], "dice": d, "res": {k: out[i] for k, out in mm["res"].items() if i < len(out)}}
                for i, (p, d) in enumerate(zip(mm["pos"], mm["dice"]))]
        _G18[S, L] = {"eval": ev, "minimax": recs, "traj": [expand_traj(r) for r in g["traj"]]}
    return _G18[S, L]


@pytest.mark.parametrize("S,L", LARGE)
def test_g18_heuristics_on_large_boards(golden, S, L):
    recs = _g18(golden, S, L)["eval"]
    assert len(recs) >= 40
    boards = np.array([r["board"] for r in recs], np.int8).reshape(-1, S, S)
    for h in HEURS:
        vals = po.evaluate(boards, h, cube_layer=L)
        assert [float(v).hex() for v in vals] == [float.fromhex(r[h]).hex() for r in recs], h


@pytest.mark.parametrize("S,L", LARGE)
def test_g18_searches_on_large_boards(golden, S, L):
    recs = _g18(golden, S, L)["minimax"]
    keys = sorted({k for r in recs for k in r["res"]})
    assert keys == sorted(["%d/%s" % (d, h) for d in (1, 2, 3) for h in ("hybrid", "attk")] + ["4/hybrid"])
    n = 0
    for key in keys:
        sub = [r for r in recs if key in r["res"]]
        assert len(sub) == (10 if key == "4/hybrid" else len(recs))
        d, h = key.split("/")
        acts, vals, _ = po.predict_minimax(np.array([r["board"] for r in sub], np.int8).reshape(-1, S, S), [r["dice"] for r in sub],
                                           int(d), h, cube_layer=L)
        for i, r in enumerate(sub):
            a0, a1, v = r["res"][key]
            assert acts[i].tolist() == [a0, a1] and float(vals[i]).hex() == float.fromhex(v).hex(), (S, L, key, i)
            n += 1
    assert n >= 6 * 40 + 10


@pytest.mark.parametrize("S,L", LARGE)
def test_g18_trajectories_on_large_boards(golden, S, L):
    recs = _g18(golden, S, L)["traj"]
    assert [(opp, dep, len(rs)) for (_, _, opp, dep, _), rs in _traj_groups(recs).items()] == [("random", None, 4), ("minimax", 2, 2), ("minimax", 3, 2)]
    for rec in recs:
        if rec["opp"] == "random":
            _check_traj(rec, "random")
        else:
            _check_traj(rec, "minimax", max_depth=rec["depth"], heuristic=rec["heuristic"])
