"""The HIP kernels against the UNMODIFIED reference's own results (oracle/gen_golden_deep.py), where the other GPU tests compare with
the CPU oracle: max_depth 1-6 searches on the constructed positions of tests/test_gpu_search_d5.py (G15), trajectories against
minimax(4-6) opponents (G16), the evaluation loop with a minimax(3-6) agent (G17) and 9x9 .. 11x11 boards (G18).  Bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import _run_group, bits, cpu
from tests.test_gpu_search_d5 import SIZES, positions
from tests.test_gpu_search_keys import ea  # noqa: F401  (the module-scoped GPU fixture)
from tests.test_oracle_golden_deep import G16_GROUPS, HEURS, LARGE, OTHER, _g18, _traj_groups, g15_size, g16_trajs, position_hash

pytestmark = pytest.mark.gpu

G15_KEYS = ["%d/hybrid" % d for d in (1, 2, 3, 4, 5, 6)] + ["%d/%s" % (d, h) for h in OTHER for d in (3, 4, 5, 6)]


@pytest.mark.parametrize("key", G15_KEYS)
@pytest.mark.parametrize("S", SIZES)
def test_g15_predict_equals_the_reference(ea, golden, S, key):
    """ea.predict_minimax, one lane per position.  5/h and 6/h: d5c_search<S, 1> on its two table variants (the looped d5_search for
    'two_min_dist'); 3/h and 4/h: d3_search on its two variants; few-cube endgames in every one of them"""
    g = g15_size(golden, S)
    assert position_hash(S) == g["sha256"]
    b, d = positions(S)
    r = g["res"][key]
    depth, h = key.split("/")
    idx = np.array(r["idx"])
    acts, vals = ea.predict_minimax(b[idx], d[idx], int(depth), h)
    exp_a = np.array([o[:2] for o in r["out"]], np.int8)
    exp_v = np.array([float.fromhex(o[2]) for o in r["out"]])
    bad = np.flatnonzero((cpu(acts) != exp_a).any(axis=1) | (bits(cpu(vals)) != bits(exp_v)))
    assert bad.size == 0, (S, key, bad.size, idx[bad[:5]].tolist(), b[idx[bad[:1]]], d[idx[bad[:1]]])


def _assert_lean_step_kernel(ea, n, **kw):
    """ewn_step serves this configuration with the table-driven k_step_d3 (a generic kernel answers 0 lanes per game)"""
    probe = ea.VecEWN(n, rng="mt19937", **kw)
    assert probe.lib.ewn_lanes_per_game(C.byref(probe.cfg), 0) > 0, kw


@pytest.mark.parametrize("S,L,depth,heur,nseed", G16_GROUPS, ids=lambda v: str(v))
def test_g16_trajectories_deep_minimax_opponent(ea, golden, S, L, depth, heur, nseed):
    """the trajectories of one configuration lane-parallel through ewn_step on MT19937 dice"""
    recs = _traj_groups(g16_trajs(golden))[(S, L, "minimax", depth, heur)]
    assert len(recs) == nseed
    kw = dict(max_depth=depth, heuristic=heur)
    _assert_lean_step_kernel(ea, nseed, board_size=S, cube_layer=L, opponent_policy="minimax", **kw)
    _run_group(ea, recs, "minimax", **kw)


G17_RUNS = [(5, 4, "random", None, 32), (5, 5, "random", None, 16), (5, 5, "minimax", 3, 8), (5, 6, "random", None, 4),
            (7, 3, "random", None, 16), (7, 5, "random", None, 4)]


@pytest.mark.parametrize("run", G17_RUNS, ids=lambda v: "-".join(str(x) for x in v))
def test_g17_tournament_with_deep_agents_matches_the_reference(ea, golden, run):
    """eval_minimax.py:16-50 with a minimax(3-6) agent, the whole loop on the device (the AGENT = 2 instances of the K-step kernel):
    per-episode scores and lengths identical to the reference's, and to the per-step loop's"""
    import torch
    from ewn_gym_amd.tournament import evaluate
    g = golden("g17_eval_loop_deep.json")
    assert [(r["S"], r["agent_depth"], r["opp"], r["opp_depth"], len(r["scores"])) for r in g] == G17_RUNS
    rec = g[G17_RUNS.index(run)]
    opp = {"kind": rec["opp"]}
    if rec["opp_depth"]:
        opp["max_depth"] = rec["opp_depth"]
    agent = {"kind": "minimax", "max_depth": rec["agent_depth"]}
    kw = dict(num=len(rec["scores"]), board_size=rec["S"], rng="mt19937")
    r = evaluate(agent, opp, **kw)
    assert r["engine"] == "ewn_step_k"
    assert r["scores"].cpu().tolist() == rec["scores"]
    assert r["lengths"].cpu().tolist() == rec["lengths"]
    slow = evaluate(agent, opp, use_rollout=False, **kw)
    assert slow["engine"] == "ewn_step" and torch.equal(slow["scores"], r["scores"]) and torch.equal(slow["lengths"], r["lengths"])


@pytest.mark.parametrize("S,L", LARGE)
def test_g18_large_boards(ea, golden, S, L):
    """9x9 .. 11x11 on the generic kernels: the four heuristics, depth 1-4 searches, trajectories vs RandomAgent and minimax(2 / 3)"""
    grp = _g18(golden, S, L)
    boards = np.array([r["board"] for r in grp["eval"]], np.int8).reshape(-1, S, S)
    for h in HEURS:
        exp = np.array([float.fromhex(r[h]) for r in grp["eval"]])
        assert np.array_equal(bits(cpu(ea.evaluate(boards, h, cube_layer=L))), bits(exp)), h
    recs = grp["minimax"]
    for key in sorted({k for r in recs for k in r["res"]}):
        sub = [r for r in recs if key in r["res"]]
        d, h = key.split("/")
        acts, vals = ea.predict_minimax(np.array([r["board"] for r in sub], np.int8).reshape(-1, S, S), [r["dice"] for r in sub],
                                        int(d), h, cube_layer=L)
        acts, vals = cpu(acts), cpu(vals)
        for i, r in enumerate(sub):
            a0, a1, v = r["res"][key]
            assert acts[i].tolist() == [a0, a1] and float(vals[i]).hex() == float.fromhex(v).hex(), (S, L, key, i)
    for (_, _, opp, depth, heur), rs in _traj_groups(grp["traj"]).items():
        _run_group(ea, rs, opp, **({} if opp == "random" else dict(max_depth=depth, heuristic=heur)))
