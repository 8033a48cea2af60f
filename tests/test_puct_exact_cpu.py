"""The one-launch PUCT search with exact endgame values at covered leaves, on the host (ewn_puct_search_eg): the header
of its own and the export, the one copy of the table code, what the entry refuses before anything is launched and the order it looks
at it in (ewn_puct_search's, the table among the pointers; then tile and blocks, the table's values, the alignments), the bindings'
ValueErrors and signatures, leaf_table= at every level, the spec's key and both parsers' options.  No kernel runs here: every
pointer is a small fake address and every call returns before a launch."""
import ctypes as C
import glob
import inspect
import os
import re
import sys

import pytest

from ewn_gym_amd import _lib
from tests.test_puct_fused_cpu import EINVAL, ENULL, EUNSUPPORTED, INF, INT_MAX, M_LAST, NAN, OK, ROOT, p


def search(board_size=5, cube_layer=3, M=4, sims=8, rounds=-1, c_puct=1.5, terminal_value=1.0, boards=16, dice=16, params=16, root_noise=16,
           noise_eps=0.25, tile=0, blocks=0, max_cubes=2, max_total=4, table=16, tree=16, leaf_counts=16):
    return _lib.load().ewn_puct_search_eg(board_size, cube_layer, M, sims, rounds, c_puct, terminal_value, p(boards), p(dice), p(params),
                                          p(root_noise), noise_eps, tile, blocks, max_cubes, max_total, p(table), p(tree), p(leaf_counts), None)


def test_the_entry_point_is_declared_in_its_own_header_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_puct_exact.h")).read()
    assert re.search(r"^int ewn_puct_search_eg\(", hdr, re.M) and '#include "ewn_hip.h"' in hdr
    for other in ("ewn_hip.h", "ewn_playout_search.h", "ewn_playout_search_eg.h", "ewn_puct_wide.h"):
        assert "ewn_puct_search_eg" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert _lib.EXPORTS_PUCT_EXACT == ["ewn_puct_search_eg"]
    lists = [_lib.EXPORTS, _lib.EXPORTS_PLAYOUT_SEARCH, _lib.EXPORTS_PUCT_WIDE, _lib.EXPORTS_PLAYOUT_SEARCH_EG, _lib.EXPORTS_PUCT_EXACT]
    assert sum(len(x) for x in lists) == len(set().union(*lists))                 # pairwise disjoint
    at = lib.ewn_puct_search_eg.argtypes
    assert len(at) == 20 and lib.ewn_puct_search_eg.restype is C.c_int
    assert all(at[i] is C.c_int for i in (0, 1, 2, 3, 4, 12, 13, 14, 15)) and all(at[i] is C.c_float for i in (5, 6, 11))
    assert all(at[i] is C.c_void_p for i in (7, 8, 9, 10, 16, 17, 18, 19))
    assert lib.ewn_abi_version() == 4                                             # the export is additive
    from ewn_gym_amd import build as b
    assert any(d.endswith("ewn_puct_exact.h") for d in b.DEPS)
    assert b.FILE_FLAGS["ewn_puct_fused.hip"] == ["-fno-slp-vectorize"]           # no new flag ...
    assert not any("exact" in os.path.basename(s) and "puct" in os.path.basename(s) for s in b.SRC)   # ... and no new translation unit
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_fused.hip")).read()
    assert "pol_launch_kernel(k_puct_search<S, NOISE, true>" in src and "template <int S, bool NOISE, bool EG = false>" in src
    assert src.count("getenv") == 1 and "<<<" not in src                          # EWN_PUCT_TILE stays ewn_puct_search's alone
    assert src.index("getenv") < src.index("int ewn_puct_search_eg(")


def test_one_copy_of_the_table_code_in_the_tree():
    csrc = os.path.join(ROOT, "ewn_gym_amd", "csrc")
    texts = {f: open(f).read() for f in glob.glob(os.path.join(csrc, "*"))}
    for fn in ("EWN_DEV float eg_move(", "EWN_DEV bool eg_position("):
        assert [os.path.basename(f) for f, t in texts.items() if fn in t] == ["ewn_endgame.hpp"], fn
        assert texts[os.path.join(csrc, "ewn_endgame.hpp")].count(fn) == 1
    src = texts[os.path.join(csrc, "ewn_puct_fused.hip")]
    assert "eg_position<S>(" in src and "eg_move<S>(" in src and '#include "ewn_endgame.hpp"' in src


@pytest.mark.parametrize("name", ["boards", "dice", "params", "tree", "table"])
def test_missing_pointer(name):
    assert search(**{name: None}) == ENULL
    assert search(board_size=7, max_total=3, **{name: None}) == ENULL
    for kw in ({"sims": 4097}, {"sims": -1}, {"terminal_value": NAN}, {"c_puct": -1.0}, {"noise_eps": 2.0}, {"noise_eps": NAN}, {"M": M_LAST},
               {"root_noise": None}, {"tile": -1}, {"tile": 33}, {"blocks": -1}, {"blocks": 257}, {"max_cubes": 0}, {"max_cubes": 4},
               {"max_total": 1}, {"max_total": 5}, {"leaf_counts": 18}):
        assert search(**kw, **{name: None}) == ENULL, kw                       # the pointers come before every value, the table's too


def test_leaf_counts_and_root_noise_may_be_missing():
    assert search(leaf_counts=None, tree=None) == ENULL                        # accepted up to the pointer that is missing
    assert search(leaf_counts=None, max_cubes=0) == EINVAL
    assert search(leaf_counts=18) == EINVAL and search(leaf_counts=17) == EINVAL   # given: 4-byte aligned
    assert search(root_noise=None, leaf_counts=None, tree=None) == ENULL and search(root_noise=None, tile=33) == EINVAL


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert search(M=0) == OK
    assert search(M=0, table=None, boards=None, dice=None, params=None, root_noise=None, tree=None, leaf_counts=None) == OK
    assert search(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, noise_eps=NAN, tile=-3, blocks=999, tree=18, max_cubes=9,
                  max_total=-1, table=3, leaf_counts=5) == OK


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
    for S in range(3, 12):                                                   # ... exactly where ewn_puct_search is unsupported
        for L in range(1, 5):
            assert (search(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    bad = [("sims", (-1, 4097, INT_MAX, -INT_MAX)), ("tree", (18, 17, 19)), ("terminal_value", (NAN, INF, -INF, 0.0, -1.0)),
           ("c_puct", (NAN, INF, -INF, -0.5)), ("noise_eps", (NAN, INF, -INF, -0.001, 1.001)), ("tile", (-1, 33, INT_MAX)),
           ("blocks", (-1, 257, INT_MAX)), ("max_cubes", (0, -1, 4, INT_MAX)), ("max_total", (1, 0, 5, INT_MAX)), ("table", (18, 17, 19)),
           ("leaf_counts", (18, 17, 19))]
    for name, values in bad:
        for v in values:
            assert search(**{name: v}) == EINVAL, (name, v)
            assert search(board_size=6, **{name: v}) == EUNSUPPORTED and search(M=0, **{name: v}) == OK, (name, v)
            assert search(rounds=0, **{name: v}) == EINVAL                   # whatever the rounds
            if name != "table":
                assert search(table=None, **{name: v}) == ENULL, (name, v)   # a missing table is a missing pointer: before the values
    for eps in (NAN, 2.0, -1.0):                                             # without root noise the weight is not looked at
        assert search(noise_eps=eps, root_noise=None, tree=None) == ENULL and search(noise_eps=eps, root_noise=None, max_cubes=0) == EINVAL
    assert search(max_cubes=3, max_total=7) == EINVAL and search(board_size=7, max_cubes=2, max_total=5) == EINVAL   # eg_params_ok's T <= 2 K
    # what is accepted at the values' edges, checked up to the pointers
    for kw in ({"sims": 0}, {"sims": 4096}, {"c_puct": 0.0}, {"noise_eps": 0.0}, {"noise_eps": 1.0}, {"tile": 1}, {"tile": 32}, {"blocks": 1},
               {"blocks": 256}, {"rounds": -7}, {"rounds": INT_MAX}, {"max_cubes": 1, "max_total": 2}, {"max_cubes": 3, "max_total": 6},
               {"max_cubes": 2, "max_total": 3}, {"terminal_value": 10.0}):
        assert search(tree=None, **kw) == ENULL, kw


def test_the_entry_reads_no_environment_variable(monkeypatch):
    monkeypatch.setenv("EWN_PUCT_TILE", "33")                                # ewn_puct_search's alone, and out of its range at that
    assert search(tree=None) == ENULL and search(tile=33) == EINVAL and search(M=0) == OK


def test_the_binding_checks_its_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.puct_exact import puct_search_exact
    assert ewn_gym_amd.puct_search_exact is puct_search_exact and "puct_search_exact" in ewn_gym_amd.__all__
    assert ewn_gym_amd.__all__[0] == "VecEWN"
    sig = inspect.signature(puct_search_exact)
    assert list(sig.parameters) == ["boards", "dice", "params", "sims", "leaf_table", "c_puct", "terminal_value", "root_noise", "noise_eps",
                                    "rounds", "tile", "blocks", "cube_layer", "out", "return_leaf_counts"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[5:]] == [1.5, 1.0, None, 0.25, None, None, None, 3, None, False]
    psig = inspect.signature(ewn_gym_amd.puct_search)                               # the pinned signature stays
    assert list(psig.parameters) == ["boards", "dice", "params", "sims", "c_puct", "terminal_value", "root_noise", "noise_eps", "rounds",
                                     "cube_layer", "out"]
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, eta, z = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.ones((4, 6)), torch.zeros(n)
    table = object()                                           # the numbers are refused before the table is looked at
    f = lambda **kw: puct_search_exact(boards, dice, z, **{"sims": 8, "leaf_table": table, **kw})   # noqa: E731
    for sims in (-1, 4097, 2.0, None):
        with pytest.raises(ValueError, match="puct_search_exact: sims"):
            f(sims=sims)
    for c in (NAN, -1.0):
        with pytest.raises(ValueError, match="puct_search_exact: c_puct"):
            f(c_puct=c)
    for tv in (NAN, 0.0, INF):
        with pytest.raises(ValueError, match="puct_search_exact: terminal_value"):
            f(terminal_value=tv)
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match="puct_search_exact: noise_eps"):
            f(root_noise=eta, noise_eps=eps)
    for rounds in (-1, 1.5, "2"):
        with pytest.raises(ValueError, match="puct_search_exact: rounds"):
            f(rounds=rounds)
    for tile in (0, -1, 33, 2.0):
        with pytest.raises(ValueError, match=r"puct_search_exact: tile must be None or an integer in 1\.\.32"):
            f(tile=tile)
    for blocks in (0, -1, 257, 2.0):
        with pytest.raises(ValueError, match=r"puct_search_exact: blocks must be None or an integer in 1\.\.256"):
            f(blocks=blocks)
    with pytest.raises(ValueError, match="puct_search_exact: leaf_table must be an EndgameTable, got object"):
        f()
    with pytest.raises(ValueError, match="puct_search_exact: leaf_table must be an EndgameTable, got NoneType"):
        f(leaf_table=None)
    with pytest.raises(ValueError):
        puct_search_exact(torch.zeros((4, 6, 6), dtype=torch.int8), dice, z, 8, table)


def test_leaf_table_at_every_level(monkeypatch):
    torch = pytest.importorskip("torch")
    from classical_policies.model import PuctAgent
    from ewn_gym_amd.distill import PuctSelfPlayTrainer, SearchDistillTrainer
    from ewn_gym_amd.search import predict_puct, selfplay_puct
    from ewn_gym_amd.tournament import _policy, evaluate_model
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, z = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    for f in (predict_puct, selfplay_puct, PuctAgent.__init__, PuctSelfPlayTrainer.__init__):
        assert inspect.signature(f).parameters["leaf_table"].default is None, f
        assert list(inspect.signature(f).parameters)[-1] == "leaf_table", f      # behind every keyword there was
    assert "leaf_table" not in inspect.signature(SearchDistillTrainer.__init__).parameters          # out of scope
    assert inspect.signature(evaluate_model).parameters["puct_table"].default is None
    t = object()                                               # never looked at: every refusal below comes before the table, tensors or GPU
    for f, who in ((predict_puct, "predict_puct"), (selfplay_puct, "selfplay_puct")):
        with pytest.raises(ValueError, match="%s: leaf_table does not go with endgame_table" % who):
            f(boards, dice, z, sims=4, leaf_table=t, endgame_table=t)
        with pytest.raises(ValueError, match="%s: leaf_table does not go with leaves=4" % who):
            f(boards, dice, z, sims=4, leaf_table=t, leaves=4)
        with pytest.raises(ValueError, match="%s: leaf_table must be an EndgameTable, got object" % who):   # fused is not read
            f(boards, dice, z, sims=4, leaf_table=t, fused=True)
        with pytest.raises(ValueError, match="%s: sims" % who):                  # the numbers are still refused first
            f(boards, dice, z, sims=-1, leaf_table=t, endgame_table=t)
        # the old refusal and its text stay
        with pytest.raises(ValueError, match="%s: fused=True does not take an endgame_table: the exact-leaf substitution is the staged "
                                             "path's" % who):
            f(boards, dice, z, sims=4, fused=True, endgame_table=t)
        with pytest.raises(ValueError, match="%s: params.*GPU" % who):           # without a table: the usual checks
            f(boards, dice, z, sims=4)
    with pytest.raises(ValueError, match="PuctAgent: leaf_table does not go with endgame_table"):    # before the model is looked at
        PuctAgent(z, sims=4, leaf_table="nowhere.pt", endgame_table="elsewhere.pt")
    with pytest.raises(ValueError, match="PuctAgent: leaf_table does not go with leaves=2"):
        PuctAgent(z, sims=4, leaf_table="nowhere.pt", leaves=2)
    with pytest.raises(ValueError, match="PuctAgent: fused=True does not take an endgame_table"):
        PuctAgent(z, sims=4, fused=True, endgame_table="nowhere.pt")
    real = torch.Tensor.to                 # the constructor on a host without a device: its parameters stay where they are
    monkeypatch.setattr(torch.Tensor, "to", lambda t, *a, **k: t if a[:1] == ("cuda",) else real(t, *a, **k))
    assert PuctAgent(z, sims=4).leaf_table is None and PuctAgent(z, sims=4, fused=True).leaf_table is None
    with pytest.raises(ValueError, match="PuctAgent: leaf_table must be an EndgameTable or the path of a saved one, got int"):
        PuctAgent(z, sims=4, leaf_table=5)
    with pytest.raises(ValueError, match="PuctAgent: leaf_table must be an EndgameTable or the path of a saved one, got int"):
        _policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaf_table": 5}, 3, 0)
    with pytest.raises(ValueError, match="leaf_table does not go with endgame_table"):
        _policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaf_table": "nowhere.pt", "endgame_table": "elsewhere.pt"}, 3, 0)
    with pytest.raises(ValueError, match="fused=True does not take an endgame_table"):
        _policy({"kind": "mlp_puct", "model": z, "sims": 4, "fused": True, "endgame_table": "nowhere.pt"}, 3, 0)
    assert callable(_policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaf_table": None}, 3, 0))
    # the trainer: before the env is looked at
    for kw, text in (({"endgame_table": "elsewhere.pt"}, "leaf_table does not go with endgame_table"),
                     ({"leaves": 4}, "leaf_table does not go with leaves=4"), ({"whole_games": True}, "leaf_table does not go with whole_games=True")):
        with pytest.raises(ValueError, match="PuctSelfPlayTrainer: " + text):
            PuctSelfPlayTrainer(None, sims=4, leaf_table="nowhere.pt", **kw)
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: fused=True does not take an endgame_table"):
        PuctSelfPlayTrainer(None, sims=4, fused=True, endgame_table="nowhere.pt")
    with pytest.raises(ValueError, match="SearchDistillTrainer: fused=True does not take endgame_leaves=True"):
        SearchDistillTrainer(None, search="puct", fused=True, endgame_table="nowhere.pt", endgame_leaves=True)
    # evaluate_model: before the model is looked at
    with pytest.raises(ValueError, match="evaluate_model: puct_table goes with puct and without endgame_table"):
        evaluate_model(None, puct_table="nowhere.pt")
    with pytest.raises(ValueError, match="evaluate_model: puct_table goes with puct and without endgame_table"):
        evaluate_model(None, puct=8, puct_table="nowhere.pt", endgame_table="elsewhere.pt")
    with pytest.raises(ValueError, match="evaluate_model: leaf_table does not go with leaves=4"):
        evaluate_model(None, puct=8, puct_table="nowhere.pt", leaves=4)
    with pytest.raises(ValueError, match="evaluate_model: puct_table must be an EndgameTable or the path of a saved one, got int"):
        evaluate_model(None, puct=8, puct_table=5)


def test_both_command_lines_take_puct_table(monkeypatch, capsys):
    pytest.importorskip("torch")
    from ewn_gym_amd import tournament, train_a2c
    ap = tournament._parser()
    assert ap.parse_args(["--model", "best.pt", "--puct", "64"]).puct_table is None
    a = ap.parse_args(["--model", "best.pt", "--puct", "64", "--puct_table", "t.pt"])
    assert (a.puct, a.puct_table, a.endgame_table, a.playout_table, a.fused, a.leaves) == (64, "t.pt", None, None, False, 1)
    for argv, text in ((["--model", "best.pt", "--puct_table", "t.pt"], "--puct_table goes with --puct and --leaves 1"),
                       (["--model", "best.pt", "--puct", "8", "--leaves", "4", "--puct_table", "t.pt"], "--puct_table goes with --puct and --leaves 1"),
                       (["--model", "best.pt", "--puct", "8", "--endgame_table", "e.pt", "--puct_table", "t.pt"], "without --endgame_table")):
        monkeypatch.setattr(sys, "argv", ["tournament"] + argv)
        with pytest.raises(SystemExit):
            tournament.main()
        assert text in capsys.readouterr().err
    ap = train_a2c._parser()
    assert ap.parse_args(["SELFPLAY"]).puct_table is None
    a = ap.parse_args(["SELFPLAY", "--sims", "16", "--puct_table", "t.pt"])
    assert (a.algorithm, a.sims, a.puct_table, a.endgame_table, a.fused, a.whole_games, a.leaves) == ("SELFPLAY", 16, "t.pt", None, False, False, 1)
