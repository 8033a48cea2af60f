"""The arena on the host (ewn_puct_arena, ewn_puct_arena_scratch_bytes, arena_puct, arena_puct_games, tournament.arena, --arena;
DESIGN.md 4y): the header of its own and the exports, what the entry refuses before anything is launched and the order it looks at it
in (ewn_puct_selfplay's, params_b among the pointers; first and the noise may be missing), the scratch rule, the bindings' ValueErrors
and signatures, the command line's refusals.  No kernel runs here: every pointer is a small fake address and every call returns before
a launch."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

from ewn_gym_amd import _lib
from tests.test_puct_games_cpu import EINVAL, ENULL, EUNSUPPORTED, INF, M_LAST, NAN, OK, ROOT, p
from tests.test_puct_games_cpu import play as selfplay

POINTERS = ("params", "params_b", "boards", "dice", "game", "scratch")


def play(board_size=5, cube_layer=3, M=4, sims=8, max_plies=80, c_puct=1.5, terminal_value=1.0, params=16, params_b=16, noise=16,
         noise_eps=0.25, temp_plies=8, key=0, game_offset=0, tile=0, blocks=0, boards=16, dice=16, game=16, first=16, rec=16, scratch=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_arena(board_size, cube_layer, M, sims, max_plies, c_puct, terminal_value, p(params), p(params_b), p(noise),
                                      noise_eps, temp_plies, key, game_offset, tile, blocks, p(boards), p(dice), p(game), p(first),
                                      *[p(rec)] * 6, p(scratch), None)


def test_the_entry_points_are_declared_in_their_own_header_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_puct_arena.h")).read()
    assert re.search(r"^int ewn_puct_arena\(", hdr, re.M) and re.search(r"^int64_t ewn_puct_arena_scratch_bytes\(", hdr, re.M)
    assert '#include "ewn_hip.h"' in hdr
    for other in ("ewn_hip.h", "ewn_playout_search.h", "ewn_playout_search_eg.h", "ewn_puct_wide.h", "ewn_puct_exact.h", "ewn_puct_games_exact.h"):
        assert "ewn_puct_arena" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert _lib.EXPORTS_PUCT_ARENA == ["ewn_puct_arena_scratch_bytes", "ewn_puct_arena"]
    lists = [_lib.EXPORTS, _lib.EXPORTS_PLAYOUT_SEARCH, _lib.EXPORTS_PUCT_WIDE, _lib.EXPORTS_PLAYOUT_SEARCH_EG, _lib.EXPORTS_PUCT_EXACT,
             _lib.EXPORTS_PUCT_GAMES_EXACT, _lib.EXPORTS_PUCT_ARENA]
    assert sum(len(x) for x in lists) == len(set().union(*lists))                 # pairwise disjoint
    at, ref = lib.ewn_puct_arena.argtypes, lib.ewn_puct_selfplay.argtypes
    assert len(at) == 28 and lib.ewn_puct_arena.restype is C.c_int
    # ewn_puct_selfplay's argument list with params_b behind params and first behind game
    assert list(at) == list(ref[:8]) + [C.c_void_p] + list(ref[8:18]) + [C.c_void_p] + list(ref[18:])
    assert lib.ewn_puct_arena_scratch_bytes.argtypes == lib.ewn_puct_selfplay_scratch_bytes.argtypes
    assert lib.ewn_puct_arena_scratch_bytes.restype is C.c_int64
    assert lib.ewn_abi_version() == 4                                             # the exports are additive
    from ewn_gym_amd import build as b
    # the unit is compiled with the matrix units' flag, ewn_puct_games.hip's: the table of its own stands beside FILE_FLAGS
    assert b.unit_flags("ewn_puct_arena.hip") == ["-fno-slp-vectorize"] == b.unit_flags("ewn_puct_games.hip")
    assert b.ARENA_FILE_FLAGS == {"ewn_puct_arena.hip": ["-fno-slp-vectorize"]} and not set(b.ARENA_FILE_FLAGS) & set(b.FILE_FLAGS)
    assert all(b.unit_flags(k) == v for k, v in b.FILE_FLAGS.items()) and b.unit_flags("ewn_endgame.hip") == []
    assert any(s.endswith("ewn_puct_arena.hip") for s in b.SRC)
    assert any(d.endswith("ewn_puct_arena.h") for d in b.DEPS)
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_arena.hip")).read()
    code = src.split('#include "ewn_puct.hpp"')[1]
    assert '#include "../../include/ewn_puct_arena.h"' in code and "pol_launch_kernel(k_puct_arena<S, NOISE>" in code
    assert "<<<" not in code and "getenv" not in code and "hipMalloc" not in code and "hipMemset" not in code and "Synchronize" not in code
    assert "atomic" not in code
    # the tree code, the move and the network code are the shared headers': called here, defined there
    for fn in ("pu_root<S>(", "pu_round<S, NOISE>(", "pu_play<S>(", "mlp3_pack_fwd<S>(", "mlp3_forward<S, "):
        assert fn in code, fn
    for fn in ("void pu_root(", "void pu_round(", "bool pu_play(", "void mlp3_pack_fwd(", "void mlp3_forward("):
        assert fn not in code, fn
    # the instances: S in {5, 7} x NOISE in {false, true}, no table instance
    assert sorted(set(re.findall(r"pua_launch<(\d), (true|false)>", code))) == [("5", "false"), ("5", "true"), ("7", "false"), ("7", "true")]
    assert "ewn_endgame.hpp" not in code and code.count("static_assert(") >= 3 and "POL_LDS_MAX" in code


@pytest.mark.parametrize("name", POINTERS)
def test_missing_pointer(name):
    assert play(**{name: None}) == ENULL and play(board_size=7, **{name: None}) == ENULL
    for kw in ({"sims": 4097}, {"sims": -1}, {"terminal_value": NAN}, {"c_puct": -1.0}, {"max_plies": 0}, {"temp_plies": -1}, {"tile": 33},
               {"blocks": 257}, {"noise_eps": 2.0}, {"noise_eps": NAN}, {"noise": None}, {"first": None}, {"M": M_LAST},
               {"scratch": 18} if name != "scratch" else {}, {"game": 18} if name != "game" else {}):
        assert play(**kw, **{name: None}) == ENULL, kw                       # the pointers come before every value
    assert play(board_size=6, **{name: None}) == EUNSUPPORTED              # the geometry comes before the pointers
    assert play(cube_layer=2, **{name: None}) == EUNSUPPORTED
    assert play(M=-1, **{name: None}) == EINVAL                            # ... and M before the geometry
    assert play(M=0, **{name: None}) == OK                                 # ... and so does the empty batch


def test_first_the_noise_and_the_record_pointers_may_be_missing():
    assert play(first=None, noise=None, rec=None, max_plies=0) == EINVAL   # accepted up to the values
    assert play(first=None, noise=None, rec=None, scratch=None) == ENULL
    assert play(first=17, max_plies=0) == EINVAL                           # bytes: no alignment asked of first
    assert play(M=0, params=None, params_b=None, noise=None, boards=None, dice=None, game=None, first=None, rec=None, scratch=None) == OK


def test_the_order_of_the_refusals_is_ewn_puct_selfplay_s():
    lib = _lib.load()
    assert play(M=-1) == EINVAL and play(M=-1, board_size=6) == EINVAL           # M comes first
    assert play(M=M_LAST + 1) == EINVAL and play(M=M_LAST + 1, board_size=6) == EINVAL and play(M=M_LAST + 1, params_b=None) == EINVAL
    assert play(M=M_LAST, board_size=6) == EUNSUPPORTED
    for S in (6, 8):
        assert play(board_size=S) == EUNSUPPORTED and play(board_size=S, M=0) == EUNSUPPORTED
        assert play(board_size=S, sims=-1, max_plies=0, tile=99, params_b=None) == EUNSUPPORTED
        assert lib.ewn_puct_arena_scratch_bytes(S, 3, 64, 8, 0, 0) == EUNSUPPORTED
    for L in (2, 4):
        assert play(cube_layer=L) == EUNSUPPORTED and play(board_size=7, cube_layer=L) == EUNSUPPORTED
    assert play(M=0) == OK
    assert play(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, max_plies=0, temp_plies=-1, tile=-1, blocks=999, noise_eps=NAN,
                scratch=18) == OK                                                    # the empty batch comes before the values
    # the same call, the same answer as ewn_puct_selfplay's, value by value, with and without noise and under every earlier refusal
    cases = [dict(sims=-1), dict(sims=4097), dict(scratch=18), dict(game=18), dict(terminal_value=NAN), dict(terminal_value=0.0),
             dict(terminal_value=INF), dict(c_puct=NAN), dict(c_puct=-0.5), dict(c_puct=INF), dict(max_plies=0), dict(max_plies=-3),
             dict(temp_plies=-1), dict(tile=-1), dict(tile=33), dict(blocks=-1), dict(blocks=257), dict(noise_eps=NAN), dict(noise_eps=-0.001),
             dict(noise_eps=1.001), dict(tile=1), dict(tile=32), dict(blocks=1), dict(blocks=256), dict(max_plies=1), dict(temp_plies=0),
             dict(sims=0), dict(sims=4096), dict(noise_eps=0.0), dict(noise_eps=1.0)]
    for kw in cases:
        for more in (dict(scratch=None), dict(board_size=6), dict(M=0), dict(M=-1), dict(noise=None, scratch=None), dict(board_size=7, boards=None)):
            assert play(**dict(kw, **more)) == selfplay(**dict(kw, **more)), (kw, more)
    for kw in cases[:20]:
        assert play(**kw) == EINVAL and selfplay(**kw) == EINVAL, kw
        if "noise_eps" not in kw:
            assert play(noise=None, board_size=7, **kw) == EINVAL, kw
        assert play(params_b=None, **kw) == ENULL, kw                                # a missing params_b is a missing pointer: before the values
    for eps in (NAN, 2.0, -1.0):                                                     # without noise the weight is not looked at
        assert play(noise_eps=eps, noise=None, scratch=None) == ENULL and play(noise_eps=eps, noise=None, max_plies=0) == EINVAL
    # every value refusal is EINVAL; what tells their order apart is what the call is refused FOR, which the code alone shows
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_arena.hip")).read()
    body = src[src.index("int ewn_puct_arena("):]
    order = [body.index(s) for s in ("pu_refuse(", "M == 0", "params && params_b && boards && dice && game && scratch", "sims < 0",
                                     "std::isfinite(terminal_value)", "max_plies < 1", "noise && !(noise_eps", "pua_geometry(", "pua_launch<")]
    assert order == sorted(order)


def test_the_entry_reads_no_environment_variable(monkeypatch):
    monkeypatch.setenv("EWN_PUCT_TILE", "33")                                    # ewn_puct_search's alone, and out of its range at that
    assert play(scratch=None) == ENULL and play(tile=33) == EINVAL and play(M=0) == OK


@pytest.mark.parametrize("S,sims", [(5, 8), (7, 64), (5, 0)])
def test_the_scratch_is_blocks_times_tile_trees(S, sims):
    lib = _lib.load()
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    for M, tile, blocks in ((33, 32, 1), (33, 2, 1), (33, 3, 2), (33, 1, 5), (70, 8, 2), (70, 2, 1), (1, 32, 256), (5, 4, 256), (1024, 4, 256),
                            (65536, 32, 256), (65536, 16, 100), (M_LAST, 32, 256)):
        assert lib.ewn_puct_arena_scratch_bytes(S, 3, M, sims, tile, blocks) == nb * min(blocks, -(-M // tile)) * tile, (M, tile, blocks)
    for M in (1, 3, 70, 1024, 16384, 65536):                               # 0: the library's choice, ewn_puct_selfplay's
        for tile, blocks in ((0, 0), (0, 1), (8, 0), (0, 7)):
            n = lib.ewn_puct_arena_scratch_bytes(S, 3, M, sims, tile, blocks)
            assert n > 0 and n == lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, tile, blocks), (M, tile, blocks)
    assert lib.ewn_puct_arena_scratch_bytes(S, 3, 0, sims, 0, 0) == 0
    for bad in (dict(M=-1), dict(sims=-1), dict(sims=4097), dict(tile=33), dict(tile=-1), dict(blocks=257), dict(blocks=-1)):
        kw = dict(dict(M=64, sims=sims, tile=0, blocks=0), **bad)
        assert lib.ewn_puct_arena_scratch_bytes(S, 3, kw["M"], kw["sims"], kw["tile"], kw["blocks"]) == EINVAL, bad


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd import arena, games, search
    from ewn_gym_amd.arena import arena_puct, arena_puct_games
    assert ewn_gym_amd.arena_puct is arena_puct and ewn_gym_amd.arena_puct_games is arena_puct_games
    assert {"arena_puct", "arena_puct_games"} <= set(ewn_gym_amd.__all__) and ewn_gym_amd.__all__[0] == "VecEWN"
    assert arena_puct.__module__ == arena_puct_games.__module__ == "ewn_gym_amd.arena"
    assert arena._games_arguments is games._games_arguments and arena._play_games is games._play_games   # shared, not copied
    sig = inspect.signature(arena_puct)
    assert list(sig.parameters) == ["boards", "dice", "params_a", "params_b", "first", "sims", "max_plies", "c_puct", "terminal_value",
                                    "noise_eps", "noise_alpha", "temp_plies", "key", "game_offset", "chunk", "cube_layer"]
    assert [v.default for v in list(sig.parameters.values())[4:]] == [None, 64, None, 1.5, 1.0, 0.0, 1.0, 0, 0, 0, 1024, 3]
    gsig = inspect.signature(arena_puct_games)
    assert list(gsig.parameters) == ["boards", "dice", "params_a", "params_b", "first", "sims", "max_plies", "c_puct", "terminal_value",
                                     "noise_eps", "noise_alpha", "temp_plies", "key", "game_offset", "cube_layer", "tile", "blocks"]
    for k, v in gsig.parameters.items():                                          # arena_puct's defaults where it has the parameter
        assert v.default == (sig.parameters[k].default if k in sig.parameters else None), k
    ref = inspect.signature(search.selfplay_puct).parameters                     # ... which are selfplay_puct's but for the two an arena sets
    for k in ("sims", "max_plies", "c_puct", "terminal_value", "noise_alpha", "key", "game_offset", "chunk", "cube_layer"):
        assert sig.parameters[k].default == ref[k].default, k
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, params = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    for f in (arena_puct, arena_puct_games):
        who = f.__name__
        g = lambda *a, **kw: f(boards, dice, *(a or (params, params.clone())), **kw)   # noqa: E731
        for sims in (-1, 4097, 2.0, None):
            with pytest.raises(ValueError, match=who + ": sims"):
                g(sims=sims)
        for c in (NAN, -1.0):
            with pytest.raises(ValueError, match=who + ": c_puct"):
                g(c_puct=c)
        for tv in (NAN, 0.0, INF):
            with pytest.raises(ValueError, match=who + ": terminal_value"):
                g(terminal_value=tv)
        for eps in (NAN, INF, -0.1, 1.5):
            with pytest.raises(ValueError, match=who + ": noise_eps"):
                g(noise_eps=eps)
        for alpha in (NAN, 0.0, -1.0):
            with pytest.raises(ValueError, match=who + ": noise_alpha"):
                g(noise_alpha=alpha)
        for tp in (-1, 1.5, None):
            with pytest.raises(ValueError, match=who + ": temp_plies"):
                g(temp_plies=tp)
        for T in (0, -2, 1.5, "8"):
            with pytest.raises(ValueError, match=who + ": max_plies"):
                g(max_plies=T)
        with pytest.raises(ValueError, match=who + ": key and game_offset"):
            g(game_offset=2 ** 63)
        with pytest.raises(ValueError, match=who + ": params must be a contiguous float32 tensor of %d elements" % n):
            g(torch.zeros(n + 1), params)
        with pytest.raises(ValueError, match=who + ": params must be"):
            g(params.double(), params)
        # params_b as params_a: the size, the dtype, the layout
        with pytest.raises(ValueError, match=who + ": params_b must be a contiguous float32 tensor of %d elements" % n):
            g(params, torch.zeros(n + 1))
        with pytest.raises(ValueError, match=who + ": params_b must be a contiguous float32 tensor"):
            g(params, params.double())
        with pytest.raises(ValueError, match=who + ": params_b must be a contiguous float32 tensor"):
            g(params, torch.zeros(2 * n)[::2])
        # first: int8 or bool [M]
        for bad in (torch.zeros(5, dtype=torch.int8), torch.zeros(3, dtype=torch.bool), torch.zeros(4, dtype=torch.int32), torch.zeros(4),
                    torch.zeros(8, dtype=torch.int8)[::2], torch.zeros((4, 2), dtype=torch.int8)):
            with pytest.raises(ValueError, match=who + ": first must be a contiguous int8 tensor of 4 elements"):
                g(first=bad)
        for ok in (None, torch.zeros(4, dtype=torch.int8), torch.ones(4, dtype=torch.bool), [0, 1, 0, 1]):
            with pytest.raises(ValueError, match=who + ": params.*GPU"):           # everything well-formed, but host tensors
                g(first=ok, sims=4)
        with pytest.raises(ValueError):
            f(torch.zeros((4, 6, 6), dtype=torch.int8), dice, params, params)
        with pytest.raises(TypeError):                                            # no table here
            g(endgame_table=object())
    for tile in (0, -1, 33, 2.0, "4"):
        with pytest.raises(ValueError, match=r"arena_puct_games: tile must be None or an integer in 1\.\.32"):
            arena_puct_games(boards, dice, params, params, tile=tile)
    for blocks in (0, -1, 257, 2.0):
        with pytest.raises(ValueError, match=r"arena_puct_games: blocks must be None or an integer in 1\.\.256"):
            arena_puct_games(boards, dice, params, params, blocks=blocks)
    for chunk in (0, -4):
        with pytest.raises(ValueError, match="arena_puct: chunk must be at least 1"):
            arena_puct(boards, dice, params, params, chunk=chunk)
    with pytest.raises(TypeError):
        arena_puct(boards, dice, params, params, tile=4)
    # the plain binding through the shared helper: its texts as they were
    with pytest.raises(ValueError, match="selfplay_puct_games: params.*GPU"):
        games.selfplay_puct_games(boards, dice, params, sims=4, tile=4, blocks=2)


def test_the_tournament_entry_and_the_command_line(monkeypatch, capsys):
    pytest.importorskip("torch")
    from ewn_gym_amd import tournament
    sig = inspect.signature(tournament.arena)
    assert list(sig.parameters) == ["model_a", "model_b", "num", "sims", "board_size", "cube_layer", "seed_offset", "key", "max_plies", "c_puct",
                                    "terminal_value", "whole_games"]
    assert [v.default for v in list(sig.parameters.values())[2:]] == [1024, 64, 5, 3, 0, 12345, None, 1.5, 1.0, True]

    class On7:
        S = 7
    with pytest.raises(ValueError, match="arena: a model plays 7x7 boards, the evaluation is on 5x5"):   # before anything is built
        tournament.arena(On7(), On7())
    ap = tournament._parser()
    assert ap.parse_args(["--model", "a.pt"]).arena is None
    a = ap.parse_args(["--model", "a.pt", "--opponent_model", "b.pt", "--arena", "32"])
    assert (a.model, a.opponent_model, a.arena, a.puct) == ("a.pt", "b.pt", 32, None)
    both = ["--model", "a.pt", "--opponent_model", "b.pt", "--arena", "16"]
    for argv, text in ((["--arena", "16"], "--arena goes with --model and --opponent_model"),
                       (["--model", "a.pt", "--arena", "16"], "--arena goes with --model and --opponent_model"),
                       (["--opponent_model", "b.pt", "--arena", "16"], "--arena goes with --model and --opponent_model"),
                       (both + ["--puct", "8"], "--arena does not go with --puct"),
                       (both + ["--lookahead"], "--arena does not go with"),
                       (both + ["--fused"], "--arena does not go with"),
                       (both + ["--leaves", "4"], "--arena does not go with"),
                       (both + ["--endgame_table", "t.pt"], "--arena does not go with"),
                       (both + ["--puct_table", "t.pt"], "--arena does not go with"),
                       (both + ["--playout_table", "t.pt"], "--arena does not go with"),
                       (both[:4] + ["--arena", "4097"], "--arena takes 0..4096 simulations"),
                       (both[:4] + ["--arena", "-1"], "--arena takes 0..4096 simulations"),
                       # the refusal that stays, with its text
                       (both[:4] + ["--puct", "8"], "--puct goes with --model and the classical opponents of --agents")):
        monkeypatch.setattr(sys, "argv", ["tournament"] + argv)
        with pytest.raises(SystemExit) as e:
            tournament.main()
        assert e.value.code != 0 and text in str(e.value.code) + capsys.readouterr().err, argv
