"""Whole self-play games in one launch on the host (ewn_puct_selfplay, ewn_puct_selfplay_scratch_bytes, selfplay_puct_games; DESIGN.md
4s): the declarations and the exports, what the entry point refuses before anything is launched and the order it looks at it in
(ewn_puct_search's: arguments, geometry, the empty batch, pointers, then the values; then max_plies, temp_plies, tile and blocks;
noise_eps last and only when noise is given), the size function, the binding's ValueErrors, the trainer's and the command line's
whole_games.  No kernel runs here."""
import ctypes as C
import inspect
import os
import re

import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
INT_MAX = 2 ** 31 - 1
M_LAST = INT_MAX // 64
NAN, INF = float("nan"), float("inf")
POINTERS = ("params", "boards", "dice", "game", "scratch")


def p(a):
    return None if a is None else C.c_void_p(a)


def play(board_size=5, cube_layer=3, M=4, sims=8, max_plies=80, c_puct=1.5, terminal_value=1.0, params=16, noise=16, noise_eps=0.25,
         temp_plies=8, key=0, game_offset=0, tile=0, blocks=0, boards=16, dice=16, game=16, rec=16, scratch=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_selfplay(board_size, cube_layer, M, sims, max_plies, c_puct, terminal_value, p(params), p(noise), noise_eps,
                                         temp_plies, key, game_offset, tile, blocks, p(boards), p(dice), p(game), *[p(rec)] * 6, p(scratch), None)


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int ewn_puct_selfplay\(", hdr, re.M) and re.search(r"^int64_t ewn_puct_selfplay_scratch_bytes\(", hdr, re.M)
    for name in ("ewn_puct_selfplay", "ewn_puct_selfplay_scratch_bytes"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    at = lib.ewn_puct_selfplay.argtypes
    assert len(at) == 26
    assert [i for i, t in enumerate(at) if t is C.c_float] == [5, 6, 9]           # c_puct, terminal_value; noise_eps
    assert at[11] is C.c_uint64 and at[12] is C.c_int64                           # key, game_offset
    assert all(at[i] is C.c_int32 for i in (0, 1, 2, 3, 4, 10, 13, 14)) and all(at[i] is C.c_void_p for i in (7, 8) + tuple(range(15, 26)))
    assert len(lib.ewn_puct_selfplay_scratch_bytes.argtypes) == 6 and lib.ewn_puct_selfplay_scratch_bytes.restype is C.c_int64
    assert lib.ewn_abi_version() == 4                                             # the exports are additive
    from ewn_gym_amd import build as b
    assert b.FILE_FLAGS["ewn_puct_games.hip"] == ["-fno-slp-vectorize"] and any(s.endswith("ewn_puct_games.hip") for s in b.SRC)


@pytest.mark.parametrize("name", POINTERS)
def test_missing_pointer(name):
    assert play(**{name: None}) == ENULL and play(board_size=7, **{name: None}) == ENULL
    assert play(sims=4097, **{name: None}) == ENULL                        # the pointers come before the values
    assert play(terminal_value=NAN, **{name: None}) == ENULL and play(c_puct=-1.0, **{name: None}) == ENULL
    assert play(max_plies=0, **{name: None}) == ENULL and play(tile=33, **{name: None}) == ENULL
    assert play(noise_eps=2.0, **{name: None}) == ENULL and play(noise=None, **{name: None}) == ENULL
    assert play(M=M_LAST, **{name: None}) == ENULL
    assert play(board_size=6, **{name: None}) == EUNSUPPORTED              # the geometry comes before the pointers
    assert play(M=0, **{name: None}) == OK                                 # ... and so does the empty batch


def test_the_record_pointers_and_the_noise_may_be_missing():
    assert play(rec=None, noise=None, max_plies=0) == EINVAL               # accepted up to the values


def test_the_order_of_the_refusals():
    lib = _lib.load()
    assert play(M=-1) == EINVAL and play(M=-1, board_size=6) == EINVAL           # M comes first
    assert play(M=M_LAST + 1) == EINVAL and play(M=M_LAST + 1, board_size=6) == EINVAL and play(M=M_LAST + 1, scratch=None) == EINVAL
    assert play(M=M_LAST, board_size=6) == EUNSUPPORTED
    for S in (6, 8):
        assert play(board_size=S) == EUNSUPPORTED and play(board_size=S, M=0) == EUNSUPPORTED
        assert play(board_size=S, sims=-1, max_plies=0, tile=99) == EUNSUPPORTED
        assert lib.ewn_puct_selfplay_scratch_bytes(S, 3, 64, 8, 0, 0) == EUNSUPPORTED
    for L in (2, 4):
        assert play(cube_layer=L) == EUNSUPPORTED and play(board_size=7, cube_layer=L) == EUNSUPPORTED
    assert play(M=0) == OK
    assert play(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, max_plies=0, temp_plies=-1, tile=-1, blocks=999, noise_eps=NAN,
                scratch=18) == OK                                                    # the empty batch comes before the values
    # every value refusal is EINVAL; what tells their order apart is what the call is refused FOR, which the code alone shows.  Each
    # value is refused on its own with everything else in order, with and without noise:
    for kw in (dict(sims=-1), dict(sims=4097), dict(scratch=18), dict(game=18), dict(terminal_value=NAN), dict(terminal_value=0.0),
               dict(terminal_value=INF), dict(c_puct=NAN), dict(c_puct=-0.5), dict(c_puct=INF), dict(max_plies=0), dict(max_plies=-3),
               dict(temp_plies=-1), dict(tile=-1), dict(tile=33), dict(blocks=-1), dict(blocks=257)):
        assert play(**kw) == EINVAL and play(board_size=7, noise=None, **kw) == EINVAL, kw
        assert play(board_size=6, **kw) == EUNSUPPORTED, kw
    for kw in (dict(tile=1), dict(tile=32), dict(blocks=1), dict(blocks=256), dict(max_plies=1), dict(temp_plies=0), dict(sims=0), dict(sims=4096)):
        assert play(scratch=None, **kw) == ENULL, kw                                 # in range: only the missing pointer is refused
    for eps in (NAN, INF, -INF, -0.001, 1.001):
        assert play(noise_eps=eps) == EINVAL and play(board_size=6, noise_eps=eps) == EUNSUPPORTED
        assert play(noise_eps=eps, noise=None, scratch=None) == ENULL                # without noise the weight is not looked at
        assert play(noise_eps=eps, noise=None, M=0) == OK


@pytest.mark.parametrize("S,sims", [(5, 8), (7, 64), (5, 0)])
def test_the_scratch_is_blocks_times_tile_trees(S, sims):
    lib = _lib.load()
    nb = lib.ewn_puct_tree_bytes(S, 3, sims)
    for M, tile, blocks in ((33, 32, 1), (33, 2, 1), (33, 3, 2), (33, 1, 5), (70, 8, 2), (1, 32, 256), (5, 4, 256), (1024, 4, 256),
                            (65536, 32, 256), (65536, 16, 100), (M_LAST, 32, 256)):
        assert lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, tile, blocks) == nb * min(blocks, -(-M // tile)) * tile, (M, tile, blocks)
    for M in (1, 3, 70, 1024, 16384, 65536):                               # 0: the library's choice, within the same ranges
        n = lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, 0, 0)
        assert n > 0 and n % nb == 0 and n // nb <= 32 * 256
        t = lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, 0, 1) // nb   # one block: its columns
        assert 1 <= t <= 32 and n // nb == t * min(256, -(-M // t))
        assert lib.ewn_puct_selfplay_scratch_bytes(S, 3, M, sims, 8, 0) == nb * 8 * min(256, -(-M // 8))
    assert lib.ewn_puct_selfplay_scratch_bytes(S, 3, 0, sims, 0, 0) == 0
    for bad in (dict(M=-1), dict(sims=-1), dict(sims=4097), dict(tile=33), dict(tile=-1), dict(blocks=257), dict(blocks=-1)):
        kw = dict(dict(M=64, sims=sims, tile=0, blocks=0), **bad)
        assert lib.ewn_puct_selfplay_scratch_bytes(S, 3, kw["M"], kw["sims"], kw["tile"], kw["blocks"]) == EINVAL, bad


def test_the_binding_checks_its_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd import games, search
    from ewn_gym_amd.games import selfplay_puct_games
    assert "selfplay_puct_games" in ewn_gym_amd.__all__ and ewn_gym_amd.selfplay_puct_games is selfplay_puct_games
    assert selfplay_puct_games.__module__ == "ewn_gym_amd.games" and not hasattr(search, "selfplay_puct_games")
    sig = inspect.signature(selfplay_puct_games)
    assert list(sig.parameters) == ["boards", "dice", "params", "sims", "max_plies", "c_puct", "terminal_value", "noise_eps", "noise_alpha",
                                    "temp_plies", "key", "game_offset", "cube_layer", "tile", "blocks"]
    ref = inspect.signature(search.selfplay_puct).parameters
    for k, v in sig.parameters.items():                                   # selfplay_puct's defaults where it has the parameter
        assert v.default == (ref[k].default if k in ref else None), k
    assert (games.PUCT_GAMES_TILE, games.PUCT_GAMES_MAX_BLOCKS) == (32, 256)
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, params = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    who = "selfplay_puct_games"
    for sims in (-1, 4097, 2.0, None):
        with pytest.raises(ValueError, match=who + ": sims"):
            selfplay_puct_games(boards, dice, params, sims=sims)
    for c in (NAN, -1.0):
        with pytest.raises(ValueError, match=who + ": c_puct"):
            selfplay_puct_games(boards, dice, params, c_puct=c)
    for tv in (NAN, 0.0, INF):
        with pytest.raises(ValueError, match=who + ": terminal_value"):
            selfplay_puct_games(boards, dice, params, terminal_value=tv)
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match=who + ": noise_eps"):
            selfplay_puct_games(boards, dice, params, noise_eps=eps)
    for alpha in (NAN, 0.0, -1.0):
        with pytest.raises(ValueError, match=who + ": noise_alpha"):
            selfplay_puct_games(boards, dice, params, noise_alpha=alpha)
    for tp in (-1, 1.5, None):
        with pytest.raises(ValueError, match=who + ": temp_plies"):
            selfplay_puct_games(boards, dice, params, temp_plies=tp)
    for T in (0, -2, 1.5, "8"):
        with pytest.raises(ValueError, match=who + ": max_plies"):
            selfplay_puct_games(boards, dice, params, max_plies=T)
    for tile in (0, -1, 33, 2.0, "4"):
        with pytest.raises(ValueError, match=who + ": tile"):
            selfplay_puct_games(boards, dice, params, tile=tile)
    for blocks in (0, -1, 257, 2.0):
        with pytest.raises(ValueError, match=who + ": blocks"):
            selfplay_puct_games(boards, dice, params, blocks=blocks)
    with pytest.raises(ValueError, match=who + ": key and game_offset"):
        selfplay_puct_games(boards, dice, params, game_offset=2 ** 63)
    with pytest.raises(ValueError, match=who + ": params.*GPU"):              # everything well-formed, but host tensors
        selfplay_puct_games(boards, dice, params, sims=4, tile=4, blocks=2)
    with pytest.raises(ValueError, match=who + ": params"):
        selfplay_puct_games(boards, dice, torch.zeros(n + 1))
    with pytest.raises(ValueError):
        selfplay_puct_games(torch.zeros((4, 6, 6), dtype=torch.int8), dice, params)
    with pytest.raises(TypeError):                                        # no table here: the exact leaves are the staged path's
        selfplay_puct_games(boards, dice, params, endgame_table=object())


def test_the_trainer_and_the_command_line_take_whole_games():
    pytest.importorskip("torch")
    from ewn_gym_amd import train_a2c
    from ewn_gym_amd.distill import PuctSelfPlayTrainer
    assert inspect.signature(PuctSelfPlayTrainer.__init__).parameters["whole_games"].default is False
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: whole_games=True does not take an endgame_table"):   # before the env is looked at
        PuctSelfPlayTrainer(None, sims=4, whole_games=True, endgame_table=object())
    ap = train_a2c._parser()
    assert ap.parse_args(["SELFPLAY"]).whole_games is False and ap.parse_args(["SELFPLAY", "--fused"]).whole_games is False
    a = ap.parse_args(["SELFPLAY", "--whole_games", "--sims", "16"])
    assert (a.algorithm, a.whole_games, a.fused, a.sims) == ("SELFPLAY", True, False, 16)
