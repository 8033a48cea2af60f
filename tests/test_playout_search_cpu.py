"""The playout-valued PUCT search on the host (ewn_playout_search): the header of its own and the export, what the
entry point refuses before anything is launched and the order it looks at it in (pu_refuse's arguments, geometry and empty batch;
the pointers; then sims, the tree's alignment, playouts, c_puct, blocks), the bindings' ValueErrors, signatures and defaults, the
`__all__` of both packages, the tournament's spec kind and parser options.  No kernel runs here.

model_trees() is the definition restated without a GPU: the numpy tree of tests/test_gpu_puct.py (Model) with pu_evaluate's uniform
priors computed in numpy fp32 and oracle/pyoracle.playout_wins as the leaf values.  Here a small case of it is checked for the
properties of a finished search; tests/test_gpu_playout_search.py compares the kernel's trees with it field by field."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
INT_MAX = 2 ** 31 - 1
M_LAST = INT_MAX // 64
NAN, INF = float("nan"), float("inf")
KEY_STEP = 0x9E3779B97F4A7C15
MASK64 = 0xFFFFFFFFFFFFFFFF
F = np.float32


def p(a):
    return None if a is None else C.c_void_p(a)


def search(board_size=5, cube_layer=3, M=4, sims=8, rounds=-1, playouts=64, c_puct=1.5, key=0, obs_id0=0, blocks=0, boards=16, dice=16,
           tree=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_playout_search(board_size, cube_layer, M, sims, rounds, playouts, c_puct, key, obs_id0, blocks, p(boards), p(dice),
                                          p(tree), None)


def test_the_entry_point_is_declared_in_its_own_header_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_playout_search.h")).read()
    assert re.search(r"^int ewn_playout_search\(", hdr, re.M) and '#include "ewn_hip.h"' in hdr
    assert "ewn_playout_search" not in open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert _lib.EXPORTS_PLAYOUT_SEARCH == ["ewn_playout_search"] and "ewn_playout_search" not in _lib.EXPORTS
    at = lib.ewn_playout_search.argtypes
    assert len(at) == 14 and lib.ewn_playout_search.restype is C.c_int
    assert all(at[i] is C.c_int for i in (0, 1, 2, 3, 4, 5, 9)) and at[6] is C.c_float and at[7] is C.c_uint64 and at[8] is C.c_uint32
    assert all(at[i] is C.c_void_p for i in (10, 11, 12, 13))
    assert lib.ewn_abi_version() == 4                                             # the export is additive
    assert int(re.search(r"#define EWN_PLAYOUT_SEARCH_MAX_PLAYOUTS (\d+)", hdr).group(1)) == 4096
    import importlib
    from ewn_gym_amd import build as b
    ps = importlib.import_module("ewn_gym_amd.playout_search")    # the package's attribute of that name is the function
    assert int(re.search(r"#define EWN_PLAYOUT_SEARCH_MAX_BLOCKS (\d+)", hdr).group(1)) == ps.PLAYOUT_SEARCH_MAX_BLOCKS
    assert ps.PLAYOUT_SEARCH_MAX_PLAYOUTS == 4096 and ps.KEY_STEP == KEY_STEP
    assert "ewn_playout_search.hip" not in b.FILE_FLAGS and any(s.endswith("ewn_playout_search.hip") for s in b.SRC)   # no matrix code, no flag
    assert any(d.endswith("ewn_playout_search.h") for d in b.DEPS)
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_playout_search.hip")).read()
    assert "pol_launch_kernel(k_playout_search<S>" in src and "getenv" not in src


@pytest.mark.parametrize("name", ["boards", "dice", "tree"])
def test_missing_pointer(name):
    assert search(**{name: None}) == ENULL
    assert search(board_size=7, **{name: None}) == ENULL
    for kw in ({"sims": 4097}, {"sims": -1}, {"playouts": 0}, {"playouts": 4097}, {"c_puct": NAN}, {"c_puct": -1.0}, {"blocks": -1},
               {"blocks": 4097}, {"M": M_LAST}):                               # the pointers come before the values
        assert search(**kw, **{name: None}) == ENULL, kw


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert search(M=0) == OK
    assert search(M=0, boards=None, dice=None, tree=None) == OK
    assert search(M=0, board_size=7, sims=4097, playouts=0, c_puct=NAN, blocks=-5, tree=18) == OK       # before the values


def test_refusals_and_their_order():
    lib = _lib.load()
    assert search(M=-1) == EINVAL and search(M=-1, board_size=6) == EINVAL   # M < 0 comes first
    assert search(M=M_LAST + 1) == EINVAL and search(M=INT_MAX) == EINVAL and search(M=M_LAST + 1, tree=None) == EINVAL
    assert search(M=M_LAST, board_size=6) == EUNSUPPORTED                    # in range: the geometry is looked at next
    for S in (6, 8):
        assert search(board_size=S) == EUNSUPPORTED and search(board_size=S, M=0) == EUNSUPPORTED
        assert search(board_size=S, tree=None) == EUNSUPPORTED               # the geometry is looked at before the pointers
    for L in (2, 4):
        assert search(cube_layer=L) == EUNSUPPORTED and search(board_size=7, cube_layer=L) == EUNSUPPORTED
    for S in range(3, 12):                                                   # ... exactly where ewn_policy_param_count is unsupported
        for L in range(1, 5):
            assert (search(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    bad = [("sims", (-1, 4097, INT_MAX, -INT_MAX)), ("tree", (18, 17, 19)), ("playouts", (0, -1, 4097, INT_MAX)),
           ("c_puct", (NAN, INF, -INF, -0.5)), ("blocks", (-1, 4097, INT_MAX))]
    for name, values in bad:
        for v in values:
            assert search(**{name: v}) == EINVAL and search(board_size=7, **{name: v}) == EINVAL, (name, v)
            assert search(board_size=6, **{name: v}) == EUNSUPPORTED and search(M=0, **{name: v}) == OK, (name, v)
            assert search(rounds=0, **{name: v}) == EINVAL                   # whatever the rounds
    # the order among the values cannot be read off the code (all EWN_EINVAL); what is accepted at their edges is checked up to the
    # pointers: a call whose values are all in range and whose tree is missing is refused for the pointer alone
    for kw in ({"sims": 0}, {"sims": 4096}, {"playouts": 1}, {"playouts": 4096}, {"c_puct": 0.0}, {"blocks": 1}, {"blocks": 4096},
               {"rounds": -7}, {"rounds": INT_MAX}, {"key": 2 ** 64 - 1}, {"obs_id0": 2 ** 32 - 1}):
        assert search(tree=None, **kw) == ENULL, kw


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.playout_search import playout_search, predict_playout_search
    assert ewn_gym_amd.playout_search is playout_search and ewn_gym_amd.predict_playout_search is predict_playout_search
    assert {"playout_search", "predict_playout_search"} <= set(ewn_gym_amd.__all__) and ewn_gym_amd.__all__[0] == "VecEWN"
    sig = inspect.signature(playout_search)
    assert list(sig.parameters) == ["boards", "dice", "sims", "playouts", "c_puct", "key", "obs_id0", "rounds", "blocks", "cube_layer", "out"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [64, 1.5, 0, 0, None, None, 3, None]
    sig = inspect.signature(predict_playout_search)
    assert list(sig.parameters) == ["boards", "dice", "sims", "playouts", "c_puct", "key", "obs_id0", "return_visits", "return_q", "return_value",
                                    "chunk", "cube_layer"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [64, 64, 1.5, 0, 0, False, False, False, 1024, 3]
    boards, dice = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    for f, who in ((lambda **kw: playout_search(boards, dice, **{"sims": 8, **kw}), "playout_search"),
                   (lambda **kw: predict_playout_search(boards, dice, **kw), "predict_playout_search")):
        for sims in (-1, 4097, 2.0, None):
            with pytest.raises(ValueError, match="%s: sims" % who):
                f(sims=sims)
        for n in (0, -1, 4097, 1.5, None):
            with pytest.raises(ValueError, match="%s: playouts" % who):
                f(playouts=n)
        for c in (NAN, -1.0, INF):
            with pytest.raises(ValueError, match="%s: c_puct" % who):
                f(c_puct=c)
        with pytest.raises(ValueError, match="%s: key" % who):
            f(key=1.5)
        for o in (-1, 2 ** 32, 0.5):
            with pytest.raises(ValueError, match="%s: obs_id0" % who):
                f(obs_id0=o)
        with pytest.raises(ValueError, match="%s: boards.*GPU" % who):           # everything well-formed, but host tensors
            f()
    for rounds in (-1, 1.5, "2"):
        with pytest.raises(ValueError, match="playout_search: rounds"):
            playout_search(boards, dice, 8, rounds=rounds)
    for blocks in (0, -1, 4097, 2.0):
        with pytest.raises(ValueError, match="playout_search: blocks"):
            playout_search(boards, dice, 8, blocks=blocks)
    with pytest.raises(ValueError, match="predict_playout_search: chunk"):
        predict_playout_search(boards, dice, chunk=0)
    with pytest.raises(ValueError, match="playout_search: no policy network for 6x6"):
        playout_search(torch.zeros((4, 6, 6), dtype=torch.int8), dice, 8)
    with pytest.raises(ValueError, match="playout_search: boards"):
        playout_search(torch.zeros((4, 5, 4), dtype=torch.int8), dice, 8)
    with pytest.raises(ValueError, match="playout_search: dice"):
        playout_search(boards, torch.ones(3, dtype=torch.int8), 8)


def test_the_agent_the_spec_kind_and_the_parser():
    pytest.importorskip("torch")
    import classical_policies
    from classical_policies import PlayoutSearchAgent
    from ewn_gym_amd import tournament
    assert "PlayoutSearchAgent" in classical_policies.__all__ and issubclass(PlayoutSearchAgent, classical_policies.PolicyBase)
    sig = inspect.signature(PlayoutSearchAgent.__init__)
    assert list(sig.parameters)[:6] == ["self", "cube_layer", "board_size", "sims", "playouts", "c_puct"]
    assert [sig.parameters[k].default for k in ("sims", "playouts", "c_puct")] == [64, 64, 1.5]
    a = PlayoutSearchAgent(3, 5, sims=8, playouts=16, c_puct=2.0, seed=3)
    assert (a.sims, a.playouts, a.c_puct, a.board_size, a.cube_layer) == (8, 16, 2.0, 5, 3)
    assert a.key == PlayoutSearchAgent(3, 5, seed=3).key != PlayoutSearchAgent(3, 5, seed=4).key
    assert all(callable(getattr(a, n)) for n in ("predict", "predict_batch", "policy_fn")) and callable(a.policy_fn())
    for kw, word in (({"sims": -1}, "sims"), ({"sims": 4097}, "sims"), ({"playouts": 0}, "playouts"), ({"c_puct": NAN}, "c_puct")):
        with pytest.raises(ValueError, match="PlayoutSearchAgent: %s" % word):
            PlayoutSearchAgent(3, 5, **kw)
    with pytest.raises(ValueError, match="PlayoutSearchAgent: no search tree for 6x6"):
        PlayoutSearchAgent(3, 6)
    assert callable(tournament._policy({"kind": "playout_search", "sims": 8, "playouts": 16, "c_puct": 1.0}, 3, 0))
    assert callable(tournament._policy({"kind": "playout_search"}, 3, 0))
    for spec, word in (({"sims": 5000}, "sims"), ({"playouts": 0}, "playouts"), ({"c_puct": -1.0}, "c_puct")):
        with pytest.raises(ValueError, match="playout_search: %s" % word):
            tournament._policy({"kind": "playout_search", **spec}, 3, 0)
    sig = inspect.signature(tournament.tournament)
    assert sig.parameters["names"].default == ("random", "minimax", "mcts")       # the default names stay
    assert [sig.parameters[k].default for k in ("sims", "playouts", "c_puct")] == [64, 64, 1.5]
    ap = tournament._parser()
    d = ap.parse_args([])
    assert (d.agents, d.sims, d.playouts, d.c_puct) == (["random", "minimax", "mcts"], 64, 64, 1.5)
    d = ap.parse_args(["--agents", "random", "playout_search", "--sims", "16", "--playouts", "8", "--c_puct", "2.5"])
    assert (d.agents, d.sims, d.playouts, d.c_puct) == (["random", "playout_search"], 16, 8, 2.5)
    assert ap.parse_args(["--model", "best.pt", "--puct", "64"]).puct == 64       # the older options stand beside them


# ---------------------------------------------------------------- the definition without a GPU

def uniform_prior(kind, one):
    """pu_evaluate's priors on five zero logits, in its own fp32 arithmetic: softmax(0, 0) = 1/2, softmax(0, 0, 0) = fl(1/3)"""
    pf, pr = F(1) / (F(1) + F(1)), F(1) / ((F(1) + F(1)) + F(1))
    raw = np.array([F(0) if kind[a] == 0 else pr if one else F(pf * pr) for a in range(6)], F)
    s = F(F(F(F(F(raw[0] + raw[1]) + raw[2]) + raw[3]) + raw[4]) + raw[5])
    return np.array([F(0) if kind[a] == 0 else F(raw[a] / s) for a in range(6)], F)


def model_trees(boards, dice, sims, playouts, key, obs_id0, c_puct=1.5, rounds=None, spare=None):
    """The definition on the CPU -> tests.test_gpu_puct.Model per observation after `rounds` rounds (None: all sims + 1).
    spare: a live position that stands in the playout call where a tree has no pending leaf (default: observation 0's board)"""
    from oracle import pyoracle
    from tests.test_gpu_puct import Model, edges
    M, S = boards.shape[0], boards.shape[1]
    spare = boards[0] if spare is None else spare
    models = [Model(boards[m], dice[m], sims) for m in range(M)]
    P = np.zeros((M, sims + 1, 6), F)
    for r in range(sims + 1 if rounds is None else min(rounds, sims + 1)):
        rows = np.stack([spare] * obs_id0 + [mod.leaf()[0] if mod.pending >= 0 else spare for mod in models]).astype(np.int8)
        w = pyoracle.playout_wins(rows, 1, playouts, key=(key + r * KEY_STEP) & MASK64)[obs_id0:]
        value = (2 * w - playouts).astype(F) / F(playouts)
        for m, mod in enumerate(models):
            if mod.pending >= 0:
                kind, _, one = edges(mod.t["board"][mod.pending], int(mod.t["dice"][mod.pending]))
                P[m, mod.pending] = uniform_prior(kind, one)
            mod.advance(np.zeros(5, F), value[m], F(c_puct), F(1), P[m])
    return models


def test_the_definition_on_the_cpu():
    """The numpy tree model imports without a GPU (it needs torch for its own module's imports only); a small case of the definition
    with the CPU oracle's playouts: a finished search's counts, and values that are shares of `playouts` playouts."""
    pytest.importorskip("torch")
    try:
        from tests.test_gpu_puct import Model  # noqa: F401
    except Exception as exc:                                   # said, and the case left out
        pytest.skip("the numpy tree model of tests/test_gpu_puct.py does not import here: %r" % (exc,))
    from oracle import pyoracle
    S, sims, n = 5, 12, 16
    env = pyoracle.OracleVecEnv(3, opponent="random", rng="philox", philox_key=5)
    b0, d0 = env.reset(seeds=np.arange(3, dtype=np.uint32) + 40)
    boards = np.concatenate([b0, np.zeros((1, S, S), np.int8)]).astype(np.int8)
    boards[3, 1, 1] = 2                                        # one side empty: a degenerate tree
    dice = np.concatenate([d0, [3]]).astype(np.int8)
    models = model_trees(boards, dice, sims, n, key=2 ** 64 - 3, obs_id0=2)
    for mod in models[:3]:
        assert not mod.degenerate and mod.done == sims and mod.pending == -1 and 1 < mod.count <= sims + 1
        assert int(mod.t["n"][0].sum()) == sims
        w = mod.t["w"][0].astype(np.float64) * n               # sums of (2 w - n) / n and of +-1: multiples of 1 / n up to rounding
        assert np.abs(w - np.round(w)).max() < 1e-3
        kind = mod.t["kind"][0]
        assert np.array_equal(mod.t["p"][0] > 0, kind != 0) and abs(float(mod.t["p"][0].sum()) - 1.0) < 1e-6
        assert len(set(mod.t["p"][0][kind != 0].tolist())) == 1                   # uniform over the legal edges
    assert models[3].degenerate and models[3].count == 1 and models[3].done == 0
    again = model_trees(boards, dice, sims, n, key=2 ** 64 - 3, obs_id0=2)
    assert all(np.array_equal(a.t["w"], b.t["w"]) and np.array_equal(a.t["n"], b.t["n"]) for a, b in zip(models, again))
    other = model_trees(boards, dice, sims, n, key=2 ** 64 - 3, obs_id0=3)         # the row index keys the playouts
    assert any(not np.array_equal(a.t["w"], b.t["w"]) for a, b in zip(models[:3], other[:3]))
