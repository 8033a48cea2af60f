"""Whole self-play games in one launch with exact endgame values at covered leaves, on the host (ewn_puct_selfplay_eg,
selfplay_puct_games_exact, games_table=): the header of its own and the export, the one copy of the table code, what the
entry refuses before anything is launched and the order it looks at it in (ewn_puct_selfplay's, the table among the pointers; then the
table's values, the alignments; noise_eps last and only when noise is given), the binding's ValueErrors and signature, games_table= on
the trainer and on the command line, and the refusals that stay as they were.  No kernel runs here: every pointer is a small fake
address and every call returns before a launch."""
import ctypes as C
import glob
import inspect
import os
import re
import sys

import pytest

from ewn_gym_amd import _lib
from tests.test_puct_games_cpu import EINVAL, ENULL, EUNSUPPORTED, INF, INT_MAX, M_LAST, NAN, OK, ROOT, p

POINTERS = ("params", "boards", "dice", "game", "scratch", "table")


def play(board_size=5, cube_layer=3, M=4, sims=8, max_plies=80, c_puct=1.5, terminal_value=1.0, params=16, noise=16, noise_eps=0.25,
         temp_plies=8, key=0, game_offset=0, tile=0, blocks=0, boards=16, dice=16, game=16, rec=16, scratch=16, max_cubes=2, max_total=4,
         table=16, leaf_counts=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_selfplay_eg(board_size, cube_layer, M, sims, max_plies, c_puct, terminal_value, p(params), p(noise), noise_eps,
                                            temp_plies, key, game_offset, tile, blocks, p(boards), p(dice), p(game), *[p(rec)] * 6, p(scratch),
                                            max_cubes, max_total, p(table), p(leaf_counts), None)


def test_the_entry_point_is_declared_in_its_own_header_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_puct_games_exact.h")).read()
    assert re.search(r"^int ewn_puct_selfplay_eg\(", hdr, re.M) and '#include "ewn_hip.h"' in hdr
    for other in ("ewn_hip.h", "ewn_playout_search.h", "ewn_playout_search_eg.h", "ewn_puct_wide.h", "ewn_puct_exact.h"):
        assert "ewn_puct_selfplay_eg" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert _lib.EXPORTS_PUCT_GAMES_EXACT == ["ewn_puct_selfplay_eg"]
    lists = [_lib.EXPORTS, _lib.EXPORTS_PLAYOUT_SEARCH, _lib.EXPORTS_PUCT_WIDE, _lib.EXPORTS_PLAYOUT_SEARCH_EG, _lib.EXPORTS_PUCT_EXACT,
             _lib.EXPORTS_PUCT_GAMES_EXACT]
    assert sum(len(x) for x in lists) == len(set().union(*lists))                 # pairwise disjoint
    at = lib.ewn_puct_selfplay_eg.argtypes
    assert len(at) == 30 and lib.ewn_puct_selfplay_eg.restype is C.c_int
    assert at[:25] == lib.ewn_puct_selfplay.argtypes[:25]                         # ewn_puct_selfplay's arguments up to the scratch
    assert at[25] is C.c_int and at[26] is C.c_int and all(at[i] is C.c_void_p for i in (27, 28, 29))
    assert [i for i, t in enumerate(at) if t is C.c_float] == [5, 6, 9] and at[11] is C.c_uint64 and at[12] is C.c_int64
    assert lib.ewn_abi_version() == 4                                             # the export is additive
    from ewn_gym_amd import build as b
    assert any(d.endswith("ewn_puct_games_exact.h") for d in b.DEPS)
    assert b.FILE_FLAGS["ewn_puct_games.hip"] == ["-fno-slp-vectorize"]           # no new flag ...
    assert len(b.FILE_FLAGS) == 11 and len(b.SRC) == len(glob.glob(os.path.join(ROOT, "ewn_gym_amd", "csrc", "*.hip")))
    assert not any("exact" in os.path.basename(s) and ("puct" in os.path.basename(s) or "games" in os.path.basename(s)) for s in b.SRC)   # ... no new unit
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_games.hip")).read()
    assert "pol_launch_kernel(k_puct_selfplay<S, NOISE, true>" in src and "template <int S, bool NOISE, bool EG = false>" in src
    assert "<<<" not in src and "getenv" not in src and "hipMalloc" not in src and "hipMemset" not in src and "Synchronize" not in src
    assert "atomic" not in src.split('#include "ewn_puct.hpp"')[1]                # the header's "no atomics" is the only mention
    assert src.count("static_assert(") >= 4 and "POL_LDS_MAX" in src.split("pug_launch_eg")[1].split("pol_launch_kernel")[0]
    assert "PU_LAYOUT 1" in open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct.hpp")).read()


def test_one_copy_of_the_table_code_in_the_tree():
    csrc = os.path.join(ROOT, "ewn_gym_amd", "csrc")
    texts = {f: open(f).read() for f in glob.glob(os.path.join(csrc, "*"))}
    for fn in ("EWN_DEV float eg_move(", "EWN_DEV bool eg_position("):
        assert [os.path.basename(f) for f, t in texts.items() if fn in t] == ["ewn_endgame.hpp"], fn
        assert texts[os.path.join(csrc, "ewn_endgame.hpp")].count(fn) == 1
    src = texts[os.path.join(csrc, "ewn_puct_games.hip")]
    assert "eg_position<S>(" in src and "eg_move<S>(" in src and '#include "ewn_endgame.hpp"' in src
    assert '#include "../../include/ewn_puct_games_exact.h"' in src


@pytest.mark.parametrize("name", POINTERS)
def test_missing_pointer(name):
    assert play(**{name: None}) == ENULL and play(board_size=7, max_total=3, **{name: None}) == ENULL
    for kw in ({"sims": 4097}, {"sims": -1}, {"terminal_value": NAN}, {"c_puct": -1.0}, {"max_plies": 0}, {"temp_plies": -1}, {"tile": 33},
               {"blocks": 257}, {"noise_eps": 2.0}, {"noise_eps": NAN}, {"noise": None}, {"M": M_LAST}, {"max_cubes": 0}, {"max_cubes": 4},
               {"max_total": 1}, {"max_total": 5}, {"leaf_counts": 18}, {"leaf_counts": None}, {"scratch": 18} if name != "scratch" else {},
               {"game": 18} if name != "game" else {}, {"table": 18} if name != "table" else {}):
        assert play(**kw, **{name: None}) == ENULL, kw                       # the pointers come before every value, the table's too
    assert play(board_size=6, **{name: None}) == EUNSUPPORTED              # the geometry comes before the pointers
    assert play(cube_layer=2, **{name: None}) == EUNSUPPORTED
    assert play(M=-1, **{name: None}) == EINVAL                            # ... and M before the geometry
    assert play(M=0, **{name: None}) == OK                                 # ... and so does the empty batch


def test_the_record_pointers_the_noise_and_leaf_counts_may_be_missing():
    assert play(rec=None, noise=None, leaf_counts=None, max_plies=0) == EINVAL           # accepted up to the values
    assert play(rec=None, noise=None, leaf_counts=None, scratch=None) == ENULL
    assert play(leaf_counts=None, max_cubes=0) == EINVAL
    assert play(leaf_counts=18) == EINVAL and play(leaf_counts=17) == EINVAL and play(leaf_counts=19) == EINVAL   # given: 4-byte aligned


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert play(M=0) == OK
    assert play(M=0, params=None, noise=None, boards=None, dice=None, game=None, rec=None, scratch=None, table=None, leaf_counts=None) == OK
    assert play(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, max_plies=0, temp_plies=-1, tile=-1, blocks=999, noise_eps=NAN,
                scratch=18, game=18, max_cubes=9, max_total=-1, table=3, leaf_counts=5) == OK


def test_refusals_and_their_order():
    lib = _lib.load()
    assert play(M=-1) == EINVAL and play(M=-1, board_size=6) == EINVAL           # M comes first
    assert play(M=M_LAST + 1) == EINVAL and play(M=INT_MAX) == EINVAL and play(M=M_LAST + 1, table=None) == EINVAL
    assert play(M=M_LAST, board_size=6) == EUNSUPPORTED                          # in range: the geometry is looked at next
    for S in (6, 8):
        assert play(board_size=S) == EUNSUPPORTED and play(board_size=S, M=0) == EUNSUPPORTED
        assert play(board_size=S, table=None) == EUNSUPPORTED                    # the geometry is looked at before the pointers
        assert play(board_size=S, sims=-1, max_plies=0, tile=99, max_cubes=0, table=18) == EUNSUPPORTED
    for L in (2, 4):
        assert play(cube_layer=L) == EUNSUPPORTED and play(board_size=7, cube_layer=L) == EUNSUPPORTED
    for S in range(3, 12):                                                       # ... exactly where ewn_puct_selfplay is unsupported
        for L in range(1, 5):
            assert (play(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    bad = [("sims", (-1, 4097, INT_MAX, -INT_MAX)), ("scratch", (18, 17, 19)), ("game", (18, 17, 19)), ("terminal_value", (NAN, INF, -INF, 0.0, -1.0)),
           ("c_puct", (NAN, INF, -INF, -0.5)), ("max_plies", (0, -3)), ("temp_plies", (-1,)), ("tile", (-1, 33, INT_MAX)),
           ("blocks", (-1, 257, INT_MAX)), ("max_cubes", (0, -1, 4, INT_MAX)), ("max_total", (1, 0, 5, INT_MAX)), ("table", (18, 17, 19)),
           ("leaf_counts", (18, 17, 19)), ("noise_eps", (NAN, INF, -INF, -0.001, 1.001))]
    for name, values in bad:
        for v in values:
            assert play(**{name: v}) == EINVAL, (name, v)
            assert play(board_size=6, **{name: v}) == EUNSUPPORTED and play(M=0, **{name: v}) == OK, (name, v)
            if name != "noise_eps":
                assert play(noise=None, **{name: v}) == EINVAL, (name, v)        # with and without noise
            if name != "table":
                assert play(table=None, **{name: v}) == ENULL, (name, v)         # a missing table is a missing pointer: before the values
    for eps in (NAN, 2.0, -1.0):                                                 # without noise the weight is not looked at
        assert play(noise_eps=eps, noise=None, scratch=None) == ENULL and play(noise_eps=eps, noise=None, max_cubes=0) == EINVAL
        assert play(noise_eps=eps, noise=None, M=0) == OK
    assert play(max_cubes=3, max_total=7) == EINVAL and play(board_size=7, max_cubes=2, max_total=5) == EINVAL   # eg_params_ok's T <= 2 K
    # every value refusal is EINVAL; what tells their order apart is what the call is refused FOR, which the code alone shows: the
    # entry's body names them in the order of the header
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_games.hip")).read()
    body = src[src.index("int ewn_puct_selfplay_eg("):]
    order = [body.index(s) for s in ("pug_refuse(", "eg_params_ok(", "(uintptr_t)table & 3", "noise && !(noise_eps", "pug_geometry(", "pug_launch_eg<")]
    assert order == sorted(order)
    shared = src[src.index("static int pug_refuse("):src.index("int ewn_puct_selfplay(")]
    order = [shared.index(s) for s in ("pu_refuse(", "M == 0", "!pointers", "sims < 0", "std::isfinite(terminal_value)", "max_plies < 1")]
    assert order == sorted(order)
    # what is accepted at the values' edges, checked up to the pointers
    for kw in ({"sims": 0}, {"sims": 4096}, {"c_puct": 0.0}, {"noise_eps": 0.0}, {"noise_eps": 1.0}, {"tile": 1}, {"tile": 32}, {"blocks": 1},
               {"blocks": 256}, {"max_plies": 1}, {"temp_plies": 0}, {"max_cubes": 1, "max_total": 2}, {"max_cubes": 3, "max_total": 6},
               {"max_cubes": 2, "max_total": 3}, {"terminal_value": 10.0}):
        assert play(scratch=None, **kw) == ENULL, kw


def test_the_entry_reads_no_environment_variable(monkeypatch):
    monkeypatch.setenv("EWN_PUCT_TILE", "33")                                    # ewn_puct_search's alone, and out of its range at that
    assert play(scratch=None) == ENULL and play(tile=33) == EINVAL and play(M=0) == OK


def test_the_binding_checks_its_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd import games, games_exact, search
    from ewn_gym_amd.games_exact import selfplay_puct_games_exact
    assert ewn_gym_amd.selfplay_puct_games_exact is selfplay_puct_games_exact and "selfplay_puct_games_exact" in ewn_gym_amd.__all__
    assert ewn_gym_amd.__all__[0] == "VecEWN" and selfplay_puct_games_exact.__module__ == "ewn_gym_amd.games_exact"
    assert not hasattr(search, "selfplay_puct_games_exact")
    sig = inspect.signature(selfplay_puct_games_exact)
    assert list(sig.parameters) == ["boards", "dice", "params", "leaf_table", "sims", "max_plies", "c_puct", "terminal_value", "noise_eps",
                                    "noise_alpha", "temp_plies", "key", "game_offset", "cube_layer", "tile", "blocks", "return_leaf_counts"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[4:]] == [64, None, 1.5, 1.0, 0.25, 1.0, 8, 0, 0, 3, None, None, False]
    ref = inspect.signature(games.selfplay_puct_games).parameters                 # selfplay_puct_games' defaults where it has the parameter
    for k, v in sig.parameters.items():
        if k in ref:
            assert v.default == ref[k].default, k
    psig = inspect.signature(games.selfplay_puct_games)                           # the pinned signature stays
    assert list(psig.parameters) == ["boards", "dice", "params", "sims", "max_plies", "c_puct", "terminal_value", "noise_eps", "noise_alpha",
                                     "temp_plies", "key", "game_offset", "cube_layer", "tile", "blocks"]
    assert games_exact._games_arguments is games._games_arguments and games_exact._play_games is games._play_games   # shared, not copied
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, params = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    who, t = "selfplay_puct_games_exact", object()                               # the numbers are refused before the table is looked at
    f = lambda **kw: selfplay_puct_games_exact(boards, dice, params, **{"leaf_table": t, **kw})   # noqa: E731
    for sims in (-1, 4097, 2.0, None):
        with pytest.raises(ValueError, match=who + ": sims"):
            f(sims=sims)
    for c in (NAN, -1.0):
        with pytest.raises(ValueError, match=who + ": c_puct"):
            f(c_puct=c)
    for tv in (NAN, 0.0, INF):
        with pytest.raises(ValueError, match=who + ": terminal_value"):
            f(terminal_value=tv)
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match=who + ": noise_eps"):
            f(noise_eps=eps)
    for alpha in (NAN, 0.0, -1.0):
        with pytest.raises(ValueError, match=who + ": noise_alpha"):
            f(noise_alpha=alpha)
    for tp in (-1, 1.5, None):
        with pytest.raises(ValueError, match=who + ": temp_plies"):
            f(temp_plies=tp)
    for tile in (0, -1, 33, 2.0, "4"):
        with pytest.raises(ValueError, match=who + r": tile must be None or an integer in 1\.\.32"):
            f(tile=tile)
    for blocks in (0, -1, 257, 2.0):
        with pytest.raises(ValueError, match=who + r": blocks must be None or an integer in 1\.\.256"):
            f(blocks=blocks)
    with pytest.raises(ValueError, match=who + ": key and game_offset"):
        f(game_offset=2 ** 63)
    with pytest.raises(ValueError, match=who + ": leaf_table must be an EndgameTable, got object"):
        f()
    with pytest.raises(ValueError, match=who + ": leaf_table must be an EndgameTable, got NoneType"):
        f(leaf_table=None)
    with pytest.raises(ValueError):
        selfplay_puct_games_exact(torch.zeros((4, 6, 6), dtype=torch.int8), dice, params, t)
    with pytest.raises(TypeError):                                               # the table is not optional
        selfplay_puct_games_exact(boards, dice, params)
    # the plain binding through the shared helpers: its texts as they were
    with pytest.raises(ValueError, match="selfplay_puct_games: max_plies must be a positive integer or None, got 0"):
        games.selfplay_puct_games(boards, dice, params, max_plies=0)
    with pytest.raises(ValueError, match="selfplay_puct_games: params.*GPU"):
        games.selfplay_puct_games(boards, dice, params, sims=4, tile=4, blocks=2)
    with pytest.raises(TypeError):
        games.selfplay_puct_games(boards, dice, params, leaf_table=t)


def test_games_table_on_the_trainer():
    pytest.importorskip("torch")
    from ewn_gym_amd.distill import PuctSelfPlayTrainer, SearchDistillTrainer
    par = inspect.signature(PuctSelfPlayTrainer.__init__).parameters
    assert par["games_table"].default is None and list(par)[-1] == "leaf_table"   # leaf_table stays the last keyword
    assert "games_table" not in inspect.signature(SearchDistillTrainer.__init__).parameters and "leaf_table" not in inspect.signature(
        SearchDistillTrainer.__init__).parameters
    who = "PuctSelfPlayTrainer: "
    for kw, text in (({"endgame_table": "elsewhere.pt"}, "games_table does not go with endgame_table"),
                     ({"leaf_table": "elsewhere.pt"}, "games_table does not go with leaf_table"),
                     ({"leaves": 4}, "games_table does not go with leaves=4")):
        with pytest.raises(ValueError, match=who + text):                        # before the env is looked at: there is none
            PuctSelfPlayTrainer(None, sims=4, games_table="nowhere.pt", **kw)
        with pytest.raises(ValueError, match=who + text):                        # whole_games is not read
            PuctSelfPlayTrainer(None, sims=4, games_table="nowhere.pt", whole_games=True, **kw)
    with pytest.raises(ValueError, match=who + "sims"):                          # the numbers are still refused first
        PuctSelfPlayTrainer(None, sims=-1, games_table="nowhere.pt", leaves=4)
    with pytest.raises(Exception) as e:                                          # alone it is accepted up to the env, which is missing
        PuctSelfPlayTrainer(None, sims=4, games_table="nowhere.pt", whole_games=True, fused=True)
    assert not isinstance(e.value, ValueError)
    # the refusals that stay, with their texts
    with pytest.raises(ValueError, match=who + "leaf_table does not go with whole_games=True: ewn_puct_selfplay takes no table"):
        PuctSelfPlayTrainer(None, sims=4, leaf_table="nowhere.pt", whole_games=True)
    with pytest.raises(ValueError, match=who + "whole_games=True does not take an endgame_table"):
        PuctSelfPlayTrainer(None, sims=4, whole_games=True, endgame_table=object())
    with pytest.raises(ValueError, match=who + "leaves=4 does not take whole_games=True"):
        PuctSelfPlayTrainer(None, sims=4, whole_games=True, leaves=4)
    with pytest.raises(ValueError, match=who + "leaf_table does not go with endgame_table"):
        PuctSelfPlayTrainer(None, sims=4, leaf_table="nowhere.pt", endgame_table="elsewhere.pt")


def test_the_command_lines(monkeypatch, capsys):
    pytest.importorskip("torch")
    from ewn_gym_amd import tournament, train_a2c
    ap = train_a2c._parser()
    assert ap.parse_args(["SELFPLAY"]).games_table is None
    a = ap.parse_args(["SELFPLAY", "--sims", "16", "--games_table", "t.pt"])
    assert (a.algorithm, a.sims, a.games_table, a.puct_table, a.endgame_table, a.fused, a.whole_games, a.leaves) == (
        "SELFPLAY", 16, "t.pt", None, None, False, False, 1)
    assert not hasattr(tournament._parser().parse_args(["--model", "best.pt"]), "games_table")   # a tournament plays no self-play
    for argv, text in ((["A2C", "--games_table", "t.pt"], "--games_table is read by SELFPLAY only"),
                       (["SELFPLAY", "--games_table", "t.pt", "--endgame_table", "e.pt", "--endgame_leaves"], "--games_table does not go with"),
                       (["SELFPLAY", "--games_table", "t.pt", "--puct_table", "p.pt"], "--games_table does not go with"),
                       (["SELFPLAY", "--games_table", "t.pt", "--leaves", "4"], "--games_table does not go with")):
        monkeypatch.setattr(sys, "argv", ["train_a2c"] + argv)
        with pytest.raises(SystemExit) as e:
            train_a2c.main()
        assert text in str(e.value.code) + capsys.readouterr().err, argv
