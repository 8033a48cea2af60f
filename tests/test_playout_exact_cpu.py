"""The playout tree search with exact endgame values at covered leaves, on the host (ewn_playout_search_eg): the header
of its own and the export, what the entry refuses before anything is launched and the order it looks at it in (ewn_playout_search's,
the table among the pointers and the table's own values last), the bindings' ValueErrors, signatures and `__all__`, the agent's
keyword, the spec's key and the parser's option.  No kernel runs here: every pointer is a small fake address and every call returns
before a launch."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

from ewn_gym_amd import _lib
from tests.test_playout_search_cpu import EINVAL, ENULL, EUNSUPPORTED, INF, INT_MAX, M_LAST, NAN, OK, ROOT, p


def search(board_size=5, cube_layer=3, M=4, sims=8, rounds=-1, playouts=64, c_puct=1.5, key=0, obs_id0=0, blocks=0, max_cubes=2, max_total=4,
           table=16, boards=16, dice=16, tree=16, leaf_counts=16):
    return _lib.load().ewn_playout_search_eg(board_size, cube_layer, M, sims, rounds, playouts, c_puct, key, obs_id0, blocks, max_cubes, max_total,
                                             p(table), p(boards), p(dice), p(tree), p(leaf_counts), None)


def test_the_entry_point_is_declared_in_its_own_header_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_playout_search_eg.h")).read()
    assert re.search(r"^int ewn_playout_search_eg\(", hdr, re.M) and '#include "ewn_playout_search.h"' in hdr
    for other in ("ewn_hip.h", "ewn_playout_search.h", "ewn_puct_wide.h"):
        assert "ewn_playout_search_eg" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert _lib.EXPORTS_PLAYOUT_SEARCH_EG == ["ewn_playout_search_eg"]
    lists = [_lib.EXPORTS, _lib.EXPORTS_PLAYOUT_SEARCH, _lib.EXPORTS_PUCT_WIDE, _lib.EXPORTS_PLAYOUT_SEARCH_EG]
    assert sum(len(x) for x in lists) == len(set().union(*lists))                 # pairwise disjoint
    at = lib.ewn_playout_search_eg.argtypes
    assert len(at) == 18 and lib.ewn_playout_search_eg.restype is C.c_int
    assert all(at[i] is C.c_int for i in (0, 1, 2, 3, 4, 5, 9, 10, 11)) and at[6] is C.c_float and at[7] is C.c_uint64 and at[8] is C.c_uint32
    assert all(at[i] is C.c_void_p for i in range(12, 18))
    assert lib.ewn_abi_version() == 4                                             # the export is additive
    from ewn_gym_amd import build as b
    assert any(d.endswith("ewn_playout_search_eg.h") for d in b.DEPS)
    assert "ewn_playout_search.hip" not in b.FILE_FLAGS                           # still no matrix code, no flag
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_playout_search.hip")).read()
    assert "pol_launch_kernel(k_playout_search<S, true>" in src and "getenv" not in src and "<<<" not in src
    shared = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_endgame.hpp")).read()
    unit = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_endgame.hip")).read()
    for fn in ("EWN_DEV float eg_move(", "EWN_DEV bool eg_position("):            # one copy, in the shared header
        assert shared.count(fn) == 1 and fn not in unit and fn not in src, fn
    assert "eg_position<S>(" in unit and "eg_position<S>(" in src and "eg_move<S>(" in src


@pytest.mark.parametrize("name", ["table", "boards", "dice", "tree"])
def test_missing_pointer(name):
    assert search(**{name: None}) == ENULL
    assert search(board_size=7, max_total=3, **{name: None}) == ENULL
    for kw in ({"sims": 4097}, {"sims": -1}, {"playouts": 0}, {"playouts": 4097}, {"c_puct": NAN}, {"c_puct": -1.0}, {"blocks": -1},
               {"blocks": 4097}, {"M": M_LAST}, {"max_cubes": 0}, {"max_cubes": 4}, {"max_total": 1}, {"max_total": 5}):
        assert search(**kw, **{name: None}) == ENULL, kw                       # the pointers come before every value, the table's too


def test_leaf_counts_may_be_missing():
    assert search(leaf_counts=None, tree=None) == ENULL                        # accepted up to the pointer that is missing
    assert search(leaf_counts=None, max_cubes=0) == EINVAL
    assert search(leaf_counts=18) == EINVAL and search(leaf_counts=17) == EINVAL   # given: 4-byte aligned


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert search(M=0) == OK
    assert search(M=0, table=None, boards=None, dice=None, tree=None, leaf_counts=None) == OK
    assert search(M=0, board_size=7, sims=4097, playouts=0, c_puct=NAN, blocks=-5, tree=18, max_cubes=9, max_total=-1, table=3) == OK


def test_refusals_and_their_order():
    lib = _lib.load()
    assert search(M=-1) == EINVAL and search(M=-1, board_size=6) == EINVAL   # M < 0 comes first
    assert search(M=M_LAST + 1) == EINVAL and search(M=INT_MAX) == EINVAL and search(M=M_LAST + 1, tree=None) == EINVAL
    assert search(M=M_LAST, board_size=6) == EUNSUPPORTED                    # in range: the geometry is looked at next
    for S in (6, 8):
        assert search(board_size=S) == EUNSUPPORTED and search(board_size=S, M=0) == EUNSUPPORTED
        assert search(board_size=S, table=None) == EUNSUPPORTED              # the geometry is looked at before the pointers
    for L in (2, 4):
        assert search(cube_layer=L) == EUNSUPPORTED and search(board_size=7, cube_layer=L) == EUNSUPPORTED
    for S in range(3, 12):                                                   # ... exactly where ewn_playout_search is unsupported
        for L in range(1, 5):
            assert (search(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    bad = [("sims", (-1, 4097, INT_MAX, -INT_MAX)), ("tree", (18, 17, 19)), ("playouts", (0, -1, 4097, INT_MAX)),
           ("c_puct", (NAN, INF, -INF, -0.5)), ("blocks", (-1, 4097, INT_MAX)), ("max_cubes", (0, -1, 4, INT_MAX)),
           ("max_total", (1, 0, 5, INT_MAX)), ("table", (18, 17, 19))]
    for name, values in bad:
        for v in values:
            assert search(**{name: v}) == EINVAL, (name, v)
            assert search(board_size=6, **{name: v}) == EUNSUPPORTED and search(M=0, **{name: v}) == OK, (name, v)
            assert search(rounds=0, **{name: v}) == EINVAL                   # whatever the rounds
            if name != "table":
                assert search(table=None, **{name: v}) == ENULL, (name, v)   # a missing table is a missing pointer: before the values
    assert search(max_cubes=3, max_total=7) == EINVAL and search(board_size=7, max_cubes=2, max_total=5) == EINVAL   # eg_params_ok's T <= 2 K
    # what is accepted at the values' edges, checked up to the pointers
    for kw in ({"sims": 0}, {"sims": 4096}, {"playouts": 1}, {"playouts": 4096}, {"c_puct": 0.0}, {"blocks": 1}, {"blocks": 4096},
               {"rounds": -7}, {"rounds": INT_MAX}, {"key": 2 ** 64 - 1}, {"obs_id0": 2 ** 32 - 1}, {"max_cubes": 1, "max_total": 2},
               {"max_cubes": 3, "max_total": 6}, {"max_cubes": 2, "max_total": 3}):
        assert search(tree=None, **kw) == ENULL, kw


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.playout_exact import playout_search_exact, predict_playout_search_exact
    assert ewn_gym_amd.playout_search_exact is playout_search_exact and ewn_gym_amd.predict_playout_search_exact is predict_playout_search_exact
    assert {"playout_search_exact", "predict_playout_search_exact"} <= set(ewn_gym_amd.__all__) and ewn_gym_amd.__all__[0] == "VecEWN"
    sig = inspect.signature(playout_search_exact)
    assert list(sig.parameters) == ["boards", "dice", "sims", "endgame_table", "playouts", "c_puct", "key", "obs_id0", "rounds", "blocks",
                                    "cube_layer", "out", "return_leaf_counts"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[4:]] == [64, 1.5, 0, 0, None, None, 3, None, False]
    sig = inspect.signature(predict_playout_search_exact)
    assert list(sig.parameters) == ["boards", "dice", "endgame_table", "sims", "playouts", "c_puct", "key", "obs_id0", "return_visits", "return_q",
                                    "return_value", "return_leaf_counts", "chunk", "cube_layer"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [64, 64, 1.5, 0, 0, False, False, False, False, 1024, 3]
    boards, dice = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    table = object()                                           # never reached: everything below is refused before the table is looked at
    for f, who in ((lambda **kw: playout_search_exact(boards, dice, **{"sims": 8, "endgame_table": table, **kw}), "playout_search_exact"),
                   (lambda **kw: predict_playout_search_exact(boards, dice, table, **kw), "predict_playout_search_exact")):
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
        with pytest.raises(ValueError, match="playout_search_exact: rounds"):
            playout_search_exact(boards, dice, 8, table, rounds=rounds)
    for blocks in (0, -1, 4097, 2.0):
        with pytest.raises(ValueError, match="playout_search_exact: blocks"):
            playout_search_exact(boards, dice, 8, table, blocks=blocks)
    with pytest.raises(ValueError, match="predict_playout_search_exact: chunk"):
        predict_playout_search_exact(boards, dice, table, chunk=0)
    with pytest.raises(ValueError, match="playout_search_exact: no policy network for 6x6"):
        playout_search_exact(torch.zeros((4, 6, 6), dtype=torch.int8), dice, 8, table)
    with pytest.raises(ValueError, match="playout_search_exact: dice"):
        playout_search_exact(boards, torch.ones(3, dtype=torch.int8), 8, table)


def test_the_agent_keyword_the_spec_key_and_the_parser_option(monkeypatch, capsys):
    pytest.importorskip("torch")
    from classical_policies import PlayoutSearchAgent
    from ewn_gym_amd import tournament
    sig = inspect.signature(PlayoutSearchAgent.__init__)
    assert list(sig.parameters) == ["self", "cube_layer", "board_size", "sims", "playouts", "c_puct", "seed", "endgame_table"]
    assert sig.parameters["endgame_table"].default is None and sig.parameters["seed"].default is None
    assert "return_leaf_counts" in inspect.signature(PlayoutSearchAgent.predict_batch).parameters
    a = PlayoutSearchAgent(3, 5, sims=8, seed=3)
    assert a.endgame_table is None and a.key == PlayoutSearchAgent(3, 5, seed=3, endgame_table=None).key
    with pytest.raises(ValueError, match="PlayoutSearchAgent: endgame_table must be an EndgameTable or the path of a saved one, got int"):
        PlayoutSearchAgent(3, 5, endgame_table=5)
    with pytest.raises(ValueError, match="playout_search: endgame_table must be an EndgameTable or the path of a saved one, got int"):
        tournament._policy({"kind": "playout_search", "endgame_table": 5}, 3, 0)
    with pytest.raises(ValueError, match="playout_search: sims"):              # the numbers are still refused first
        tournament._policy({"kind": "playout_search", "sims": 5000, "endgame_table": 5}, 3, 0)
    assert callable(tournament._policy({"kind": "playout_search", "endgame_table": None}, 3, 0))
    sig = inspect.signature(tournament.tournament)
    assert sig.parameters["playout_table"].default is None and list(sig.parameters)[-1] == "playout_table"
    with pytest.raises(ValueError, match="tournament: playout_table must be an EndgameTable or the path of a saved one, got int"):
        tournament.tournament(("random", "playout_search"), num=1, playout_table=5)
    ap = tournament._parser()
    d = ap.parse_args([])
    assert d.playout_table is None and d.endgame_table is None
    d = ap.parse_args(["--agents", "random", "playout_search", "--playout_table", "t.pt"])
    assert (d.agents, d.playout_table, d.endgame_table) == (["random", "playout_search"], "t.pt", None)
    for argv, text in ((["--endgame_table", "t.pt"], "--endgame_table goes with --model"),         # its meaning and its refusal stay
                       (["--agents", "random", "playout_search", "--endgame_table", "t.pt"], "--endgame_table goes with --model"),
                       (["--agents", "random", "mcts", "--playout_table", "t.pt"], "--playout_table goes with playout_search")):
        monkeypatch.setattr(sys, "argv", ["tournament"] + argv)
        with pytest.raises(SystemExit):
            tournament.main()
        assert text in capsys.readouterr().err
