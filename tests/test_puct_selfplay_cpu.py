"""PUCT self-play on the host: the two entry points' declarations and exports, what ewn_puct_advance_noise and
ewn_puct_play refuse before anything is launched and the order they look at it in (ewn_puct_advance's: arguments, geometry, the empty
batch, pointers, then the values), the bindings' ValueErrors, selfplay_outcomes and the q-free puct_targets on CPU tensors, the
SELFPLAY command line and the trainer's refusals.  No kernel runs here."""
import ctypes as C
import os
import re

import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
INT_MAX = 2 ** 31 - 1
M_LAST = INT_MAX // 64
NAN, INF = float("nan"), float("inf")


def p(a):
    return None if a is None else C.c_void_p(a)


def noise(board_size=5, cube_layer=3, M=4, sims=8, c_puct=1.5, terminal_value=1.0, tree=16, logits=16, value=16, root_noise=16,
          noise_eps=0.25, leaf_boards=16, leaf_dice=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_advance_noise(board_size, cube_layer, M, sims, c_puct, terminal_value, p(tree), p(logits), p(value),
                                              p(root_noise), noise_eps, p(leaf_boards), p(leaf_dice), None)


def play(board_size=5, cube_layer=3, M=4, tree=16, boards=16, dice=16, game=16, temp_plies=8, key=0, game_offset=0, rec=(None,) * 6):
    return _lib.load().ewn_puct_play(board_size, cube_layer, M, p(tree), p(boards), p(dice), p(game), temp_plies, key, game_offset,
                                     *[p(r) for r in rec], None)


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    for name in ("ewn_puct_advance_noise", "ewn_puct_play"):
        assert re.search(r"^int %s\(" % name, hdr, re.M)
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.ewn_puct_advance_noise.argtypes) == 14 and len(lib.ewn_puct_play.argtypes) == 17
    assert lib.ewn_puct_advance_noise.argtypes[10] is C.c_float
    assert lib.ewn_puct_play.argtypes[8] is C.c_uint64 and lib.ewn_puct_play.argtypes[9] is C.c_int64
    assert lib.ewn_abi_version() == 4          # the exports are additive
    assert "2^-30" in hdr                      # the dice draw's bias is stated


@pytest.mark.parametrize("name", ["tree", "logits", "value", "root_noise", "leaf_boards", "leaf_dice"])
def test_noise_missing_pointer(name):
    assert noise(**{name: None}) == ENULL
    assert noise(board_size=7, **{name: None}) == ENULL
    assert noise(sims=4097, **{name: None}) == ENULL                     # the pointers come before the values
    assert noise(terminal_value=NAN, **{name: None}) == ENULL and noise(c_puct=-1.0, **{name: None}) == ENULL
    assert noise(noise_eps=2.0, **{name: None}) == ENULL and noise(noise_eps=NAN, **{name: None}) == ENULL
    assert noise(M=M_LAST, **{name: None}) == ENULL


@pytest.mark.parametrize("name", ["tree", "boards", "dice", "game"])
def test_play_missing_pointer(name):
    assert play(**{name: None}) == ENULL
    assert play(board_size=7, rec=(16,) * 6, **{name: None}) == ENULL
    assert play(temp_plies=-1, **{name: None}) == ENULL                  # the pointers come before the values
    assert play(M=M_LAST, **{name: None}) == ENULL


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert noise(M=0) == OK and play(M=0) == OK
    assert noise(M=0, tree=None, logits=None, value=None, root_noise=None, leaf_boards=None, leaf_dice=None) == OK
    assert play(M=0, tree=None, boards=None, dice=None, game=None) == OK
    assert noise(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, noise_eps=NAN) == OK   # before the values
    assert play(M=0, temp_plies=-5, tree=18) == OK


def test_invalid_and_unsupported_arguments():
    lib = _lib.load()
    for call in (noise, play):
        assert call(M=-1) == EINVAL
        assert call(M=-1, board_size=6) == EINVAL                            # M < 0 comes first
        assert call(M=M_LAST + 1) == EINVAL and call(M=INT_MAX) == EINVAL
        assert call(M=M_LAST + 1, board_size=6) == EINVAL and call(M=M_LAST + 1, tree=None) == EINVAL
        assert call(M=M_LAST, board_size=6) == EUNSUPPORTED                  # in range: the geometry is looked at next
        for S in (6, 8):
            assert call(board_size=S) == EUNSUPPORTED
            assert call(board_size=S, M=0) == EUNSUPPORTED
            assert call(board_size=S, tree=None) == EUNSUPPORTED             # the geometry is looked at before the pointers
        for L in (2, 4):
            assert call(cube_layer=L) == EUNSUPPORTED and call(board_size=7, cube_layer=L) == EUNSUPPORTED
        for S in range(3, 12):                                               # ... exactly where ewn_policy_param_count is unsupported
            for L in range(1, 5):
                assert (call(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
        assert call(tree=18) == EINVAL                                       # a tree that is not 4-byte aligned
    for sims in (-1, 4097, INT_MAX, -INT_MAX):
        assert noise(sims=sims) == EINVAL and noise(board_size=7, sims=sims) == EINVAL
        assert noise(board_size=6, sims=sims) == EUNSUPPORTED
    for tv in (NAN, INF, -INF, 0.0, -1.0):
        assert noise(terminal_value=tv) == EINVAL and noise(board_size=8, terminal_value=tv) == EUNSUPPORTED
    for c in (NAN, INF, -INF, -0.5):
        assert noise(c_puct=c) == EINVAL and noise(board_size=6, c_puct=c) == EUNSUPPORTED
    for eps in (NAN, INF, -INF, -0.001, 1.001, 2.0, -1.0):
        assert noise(noise_eps=eps) == EINVAL and noise(board_size=7, noise_eps=eps) == EINVAL
        assert noise(board_size=6, noise_eps=eps) == EUNSUPPORTED            # the geometry is looked at before the weight
        assert noise(noise_eps=eps, root_noise=None) == ENULL
    for t in (-1, -INT_MAX):
        assert play(temp_plies=t) == EINVAL and play(board_size=7, temp_plies=t) == EINVAL
        assert play(board_size=6, temp_plies=t) == EUNSUPPORTED
    assert play(game=18) == EINVAL and play(game=17) == EINVAL             # game holds int32


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.vec_env import puct_advance, puct_play, selfplay_puct
    for name in ("puct_play", "selfplay_puct", "selfplay_outcomes", "selfplay_noise"):
        assert name in ewn_gym_amd.__all__ and getattr(ewn_gym_amd, name) is getattr(ewn_gym_amd.vec_env, name)
    lib = _lib.load()
    n, nb = lib.ewn_policy_param_count(5, 3), lib.ewn_puct_tree_bytes(5, 3, 8)
    boards, dice = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    tree, logits, value = torch.zeros((4, nb), dtype=torch.uint8), torch.zeros((4, 5)), torch.zeros(4)
    game, eta = torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 6))
    # advance with noise
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match="puct_advance: noise_eps"):
            puct_advance(tree, logits, value, boards, dice, 8, root_noise=eta, noise_eps=eps)
    with pytest.raises(ValueError, match="puct_advance: leaf_boards.*GPU"):      # everything well-formed, but host tensors
        puct_advance(tree, logits, value, boards, dice, 8, root_noise=eta)
    with pytest.raises(ValueError, match="puct_advance: leaf_boards.*GPU"):      # without noise noise_eps is not looked at
        puct_advance(tree, logits, value, boards, dice, 8, noise_eps=NAN)
    # play
    with pytest.raises(ValueError, match="puct_play: tree.*GPU"):
        puct_play(tree, boards, dice, game, 5, 8)
    with pytest.raises(ValueError, match="puct_play: tree"):
        puct_play(tree, boards, dice, game, 5, 9)                                # a tree of another budget
    with pytest.raises(ValueError, match="6x6"):
        puct_play(tree, boards, dice, game, 6, 8)
    with pytest.raises(ValueError, match="puct_play: boards"):
        puct_play(tree, boards.to(torch.int64), dice, game, 5, 8)
    with pytest.raises(ValueError, match="puct_play: dice"):
        puct_play(tree, boards, dice[:3], game, 5, 8)
    with pytest.raises(ValueError, match="puct_play: game"):
        puct_play(tree, boards, dice, game[:, :3], 5, 8)
    with pytest.raises(ValueError, match="puct_play: game"):
        puct_play(tree, boards, dice, game.to(torch.int64), 5, 8)
    for t in (-1, 1.5, None):
        with pytest.raises(ValueError, match="puct_play: temp_plies"):
            puct_play(tree, boards, dice, game, 5, 8, temp_plies=t)
    with pytest.raises(ValueError, match="puct_play: key and game_offset"):
        puct_play(tree, boards, dice, game, 5, 8, game_offset=2 ** 63)
    with pytest.raises(ValueError, match="puct_play: key and game_offset"):
        puct_play(tree, boards, dice, game, 5, 8, key=1.5)
    for out in ([], {"boards": None}):
        with pytest.raises(ValueError, match="puct_play: out must be a dict"):
            puct_play(tree, boards, dice, game, 5, 8, out=out)
    with pytest.raises(ValueError, match="sims"):
        puct_play(tree, boards, dice, game, 5, 4097)
    # the driver
    params = torch.zeros(n)
    for kw, what in (({"sims": -1}, "sims"), ({"sims": 4097}, "sims"), ({"c_puct": NAN}, "c_puct"), ({"terminal_value": 0.0}, "terminal_value"),
                     ({"noise_eps": 1.5}, "noise_eps"), ({"noise_eps": NAN}, "noise_eps"), ({"noise_alpha": 0.0}, "noise_alpha"),
                     ({"noise_alpha": INF}, "noise_alpha"), ({"temp_plies": -1}, "temp_plies"), ({"chunk": 0}, "chunk"),
                     ({"check_every": 0}, "check_every"), ({"max_plies": 0}, "max_plies"), ({"max_plies": 2.5}, "max_plies")):
        with pytest.raises(ValueError, match="selfplay_puct: .*" + what):
            selfplay_puct(boards, dice, params, **kw)
    with pytest.raises(ValueError, match="selfplay_puct: params.*GPU"):          # wrong device
        selfplay_puct(boards, dice, params)
    with pytest.raises(ValueError, match="selfplay_puct: params"):
        selfplay_puct(boards, dice, torch.zeros(n + 1))
    with pytest.raises(ValueError, match="6x6"):
        selfplay_puct(torch.zeros((4, 6, 6), dtype=torch.int8), dice, params)
    from ewn_gym_amd.vec_env import SELFPLAY_MAX_PLIES
    assert SELFPLAY_MAX_PLIES == {5: 80, 7: 128}                                 # above 2 * (40 - 6) + 1 = 69 and 2 * (64 - 6) + 1 = 117


def test_selfplay_outcomes_on_the_host():
    torch = pytest.importorskip("torch")
    from ewn_gym_amd.vec_env import selfplay_outcomes
    winner = torch.tensor([1, -1, 0, 1], dtype=torch.int32)         # three finished games of 3, 2 and 4 plies, one unfinished
    live = torch.tensor([[1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 0]], dtype=torch.bool)
    z, w = selfplay_outcomes(winner, live)
    assert z.dtype == w.dtype == torch.float32 and z.shape == w.shape == (5, 4)
    assert z.t().tolist() == [[1, -1, 1, 0, 0], [-1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, -1, 1, -1, 0]]
    assert w.t().tolist() == [[1, 1, 1, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 0]]
    assert not torch.signbit(z[w == 0]).any()                       # zeros, not negative zeros: the records compare by bytes
    z8, w8 = selfplay_outcomes(winner, live.to(torch.int8))         # the kernel's live column as it is
    assert torch.equal(z8, z) and torch.equal(w8, w)


def test_targets_without_q_on_the_host():
    torch = pytest.importorskip("torch")
    from ewn_gym_amd.distill import both_flags_one_cube, puct_targets
    b = torch.zeros((5, 5, 5), dtype=torch.int8)
    for m, cubes in enumerate(({3: (0, 0), 5: (1, 1)}, {3: (0, 0), 5: (1, 1)}, {3: (0, 0), 5: (1, 1)}, {2: (2, 2)}, {1: (0, 0), 6: (4, 0)})):
        for k, (x, y) in cubes.items():
            b[m, x, y] = k
        b[m, 4, 4] = -4
    d = torch.tensor([4, 3, 6, 9, 0], dtype=torch.int8)             # between two cubes; on a cube; above both; one cube; clamped to 1
    one = both_flags_one_cube(b, d)
    assert one.tolist() == [False, True, True, True, True]
    visits = torch.tensor([[[3, 1, 0], [2, 2, 0]], [[5, 0, 3], [0, 0, 0]], [[0, 0, 0], [0, 0, 0]], [[1, 0, 0], [0, 0, 0]],
                           [[0, 4, 0], [0, 0, 0]]], dtype=torch.int32)
    ninf = -INF
    q = torch.tensor([[[0.0] * 3] * 2, [[0.0] * 3, [ninf] * 3], [[0.0] * 3, [ninf] * 3], [[0.0] * 3, [ninf] * 3], [[0.0] * 3, [ninf] * 3]])
    value = torch.tensor([0.25, 0.5, 0.0, -1.0, 0.125])
    got = puct_targets(visits, None, value, 2.0, one_cube=one)
    want = puct_targets(visits, q, value, 2.0)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert got[0][1].tolist() == [0.5, 0.5, 5.0 / 8.0, 0.0, 3.0 / 8.0] and got[2].tolist() == [1.0, 1.0, 0.0, 1.0, 1.0]


def test_the_selfplay_command_line_parses():
    from ewn_gym_amd import train_a2c
    ap = train_a2c._parser()
    a = ap.parse_args(["SELFPLAY"])
    assert (a.algorithm, a.sims, a.c_puct, a.terminal_value, a.noise_eps, a.noise_alpha, a.temp_plies, a.max_plies) == (
        "SELFPLAY", 64, 1.5, 1.0, 0.25, 1.0, 8, None)
    assert a.endgame_table is None and a.endgame_leaves is False
    a = ap.parse_args(["SELFPLAY", "--sims", "16", "--c_puct", "2.5", "--noise_eps", "0.1", "--noise_alpha", "0.3", "--temp_plies", "4",
                       "--max_plies", "96", "--terminal_value", "10", "--endgame_table", "t.pt", "--endgame_leaves"])
    assert (a.sims, a.c_puct, a.noise_eps, a.noise_alpha, a.temp_plies, a.max_plies, a.terminal_value, a.endgame_table, a.endgame_leaves) == (
        16, 2.5, 0.1, 0.3, 4, 96, 10.0, "t.pt", True)
    for bad in (["SELFPLAY", "--temp_plies", "1.5"], ["SELFPLAY", "--max_plies", "many"], ["SELF"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    assert ap.parse_args([]).algorithm == "A2C" and ap.parse_args(["SEARCH"]).noise_eps == 0.25   # the others are as they were


def test_the_trainer_refuses_bad_numbers_before_it_looks_at_the_env():
    pytest.importorskip("torch")
    from ewn_gym_amd.distill import PuctSelfPlayTrainer

    class Env:                             # never reached
        pass

    for kw in ({"sims": -1}, {"sims": 4097}, {"c_puct": NAN}, {"terminal_value": 0.0}, {"noise_eps": 1.5}, {"noise_eps": NAN},
               {"noise_alpha": 0.0}, {"temp_plies": -1}, {"max_plies": 0}, {"pi_coef": -1.0}, {"vf_coef": INF}):
        with pytest.raises(ValueError, match="PuctSelfPlayTrainer: " + next(iter(kw))):
            PuctSelfPlayTrainer(Env(), **kw)
    assert PuctSelfPlayTrainer.algorithm == "SELFPLAY"


def test_the_trainer_refuses_a_table_of_another_board_size():
    torch = pytest.importorskip("torch")
    from ewn_gym_amd.distill import PuctSelfPlayTrainer
    from ewn_gym_amd.endgame import EndgameTable

    class Env:                             # only its board size is looked at
        S = 5

    t = EndgameTable(7, 1, 2, torch.zeros(EndgameTable.table_bytes(7, 1, 2) // 4))   # wraps a buffer: nothing is built or launched
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: the endgame table is for 7x7 boards, the env plays 5x5"):
        PuctSelfPlayTrainer(Env(), endgame_table=t)
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: sims"):     # the numbers are still looked at first
        PuctSelfPlayTrainer(Env(), sims=-1, endgame_table=t)


def test_targets_without_q_need_the_mask():
    torch = pytest.importorskip("torch")
    from ewn_gym_amd.distill import puct_targets
    with pytest.raises(ValueError, match="puct_targets: without q, one_cube"):
        puct_targets(torch.zeros((2, 2, 3), dtype=torch.int32), None, torch.zeros(2))


@pytest.mark.parametrize("flags", [["--n_steps", "7"], ["--opponent_update_every", "5"], ["--goal_reward", "1"], ["--reference_quirks"],
                                   ["--opponent_policy", "self"], ["--batch_size", "64"], ["--endgame_table", "t.pt"], ["--endgame_leaves"]])
def test_selfplay_refuses_the_flags_it_does_not_read(monkeypatch, flags):
    """before an env is made: SELFPLAY reads no rollout length, opponent or reward, and a table only at the leaves"""
    import sys
    from ewn_gym_amd import train_a2c
    monkeypatch.setattr(sys, "argv", ["train_a2c", "SELFPLAY"] + flags)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="SELFPLAY"):
        train_a2c.main()
