"""The PUCT search in one launch on the host (ewn_puct_search): the declaration and the export, what the entry point
refuses before anything is launched and the order it looks at it in (ewn_puct_advance_noise's: arguments, geometry, the empty batch,
pointers, then the values -- noise_eps only when root noise is given), the bindings' ValueErrors, the fused= keyword's refusal of an
endgame table at every level, and the two command lines.  No kernel runs here."""
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


def p(a):
    return None if a is None else C.c_void_p(a)


def search(board_size=5, cube_layer=3, M=4, sims=8, rounds=-1, c_puct=1.5, terminal_value=1.0, boards=16, dice=16, params=16,
           root_noise=16, noise_eps=0.25, tree=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_search(board_size, cube_layer, M, sims, rounds, c_puct, terminal_value, p(boards), p(dice), p(params),
                                       p(root_noise), noise_eps, p(tree), None)


def test_the_entry_point_is_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int ewn_puct_search\(", hdr, re.M)
    assert "ewn_puct_search" in _lib.EXPORTS and lib.ewn_puct_search.argtypes is not None
    at = lib.ewn_puct_search.argtypes
    assert len(at) == 14
    assert [i for i, t in enumerate(at) if t is C.c_float] == [5, 6, 11]          # c_puct, terminal_value; noise_eps
    assert all(at[i] is C.c_int32 for i in range(5))                              # ... rounds is the fifth integer
    assert all(at[i] is C.c_void_p for i in (7, 8, 9, 10, 12, 13))
    assert lib.ewn_abi_version() == 4                                             # the export is additive
    from ewn_gym_amd import build as b
    assert b.FILE_FLAGS["ewn_puct_fused.hip"] == ["-fno-slp-vectorize"] and any(s.endswith("ewn_puct_fused.hip") for s in b.SRC)


@pytest.mark.parametrize("name", ["boards", "dice", "params", "tree"])
def test_missing_pointer(name):
    assert search(**{name: None}) == ENULL
    assert search(board_size=7, **{name: None}) == ENULL
    assert search(sims=4097, **{name: None}) == ENULL                    # the pointers come before the values
    assert search(terminal_value=NAN, **{name: None}) == ENULL and search(c_puct=-1.0, **{name: None}) == ENULL
    assert search(noise_eps=2.0, **{name: None}) == ENULL and search(noise_eps=NAN, **{name: None}) == ENULL
    assert search(M=M_LAST, **{name: None}) == ENULL
    assert search(root_noise=None, **{name: None}) == ENULL


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert search(M=0) == OK
    assert search(M=0, boards=None, dice=None, params=None, root_noise=None, tree=None) == OK
    assert search(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, noise_eps=NAN, tree=18) == OK   # before the values


def test_invalid_and_unsupported_arguments():
    lib = _lib.load()
    assert search(M=-1) == EINVAL
    assert search(M=-1, board_size=6) == EINVAL                              # M < 0 comes first
    assert search(M=M_LAST + 1) == EINVAL and search(M=INT_MAX) == EINVAL
    assert search(M=M_LAST + 1, board_size=6) == EINVAL and search(M=M_LAST + 1, tree=None) == EINVAL
    assert search(M=M_LAST, board_size=6) == EUNSUPPORTED                    # in range: the geometry is looked at next
    for S in (6, 8):
        assert search(board_size=S) == EUNSUPPORTED
        assert search(board_size=S, M=0) == EUNSUPPORTED
        assert search(board_size=S, tree=None) == EUNSUPPORTED               # the geometry is looked at before the pointers
    for L in (2, 4):
        assert search(cube_layer=L) == EUNSUPPORTED and search(board_size=7, cube_layer=L) == EUNSUPPORTED
    for S in range(3, 12):                                                   # ... exactly where ewn_policy_param_count is unsupported
        for L in range(1, 5):
            assert (search(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    assert search(tree=18) == EINVAL and search(tree=18, root_noise=None) == EINVAL       # a tree that is not 4-byte aligned
    for sims in (-1, 4097, INT_MAX, -INT_MAX):
        assert search(sims=sims) == EINVAL and search(board_size=7, sims=sims) == EINVAL
        assert search(board_size=6, sims=sims) == EUNSUPPORTED
        assert search(sims=sims, rounds=0) == EINVAL                         # whatever the rounds
    for tv in (NAN, INF, -INF, 0.0, -1.0):
        assert search(terminal_value=tv) == EINVAL and search(board_size=8, terminal_value=tv) == EUNSUPPORTED
        assert search(terminal_value=tv, root_noise=None) == EINVAL
    for c in (NAN, INF, -INF, -0.5):
        assert search(c_puct=c) == EINVAL and search(board_size=6, c_puct=c) == EUNSUPPORTED
    for eps in (NAN, INF, -INF, -0.001, 1.001, 2.0, -1.0):
        assert search(noise_eps=eps) == EINVAL and search(board_size=7, noise_eps=eps) == EINVAL
        assert search(board_size=6, noise_eps=eps) == EUNSUPPORTED           # the geometry is looked at before the weight
        # without root noise the weight is not looked at: the call is accepted up to the pointer checks and the other values
        assert search(noise_eps=eps, root_noise=None, tree=None) == ENULL
        assert search(noise_eps=eps, root_noise=None, tree=18) == EINVAL and search(noise_eps=eps, root_noise=None, sims=-1) == EINVAL
        assert search(noise_eps=eps, root_noise=None, M=0) == OK


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.vec_env import predict_puct, puct_search, selfplay_puct
    assert "puct_search" in ewn_gym_amd.__all__ and ewn_gym_amd.puct_search is puct_search
    sig = inspect.signature(puct_search)
    assert list(sig.parameters) == ["boards", "dice", "params", "sims", "c_puct", "terminal_value", "root_noise", "noise_eps", "rounds",
                                    "cube_layer", "out"]
    assert [sig.parameters[k].default for k in ("c_puct", "terminal_value", "root_noise", "noise_eps", "rounds", "cube_layer", "out")] == [
        1.5, 1.0, None, 0.25, None, 3, None]
    for f in (predict_puct, selfplay_puct):
        assert inspect.signature(f).parameters["fused"].default is False     # no existing call changes a launch
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, eta = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.ones((4, 6))
    for sims in (-1, 4097, 2.0, None):
        with pytest.raises(ValueError, match="puct_search: sims"):
            puct_search(boards, dice, torch.zeros(n), sims)
    for c in (NAN, -1.0):
        with pytest.raises(ValueError, match="puct_search: c_puct"):
            puct_search(boards, dice, torch.zeros(n), 8, c_puct=c)
    for tv in (NAN, 0.0, INF):
        with pytest.raises(ValueError, match="puct_search: terminal_value"):
            puct_search(boards, dice, torch.zeros(n), 8, terminal_value=tv)
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match="puct_search: noise_eps"):
            puct_search(boards, dice, torch.zeros(n), 8, root_noise=eta, noise_eps=eps)
    for rounds in (-1, 1.5, "2"):
        with pytest.raises(ValueError, match="puct_search: rounds"):
            puct_search(boards, dice, torch.zeros(n), 8, rounds=rounds)
    with pytest.raises(ValueError, match="puct_search: params.*GPU"):            # everything well-formed, but host tensors
        puct_search(boards, dice, torch.zeros(n), 8)
    with pytest.raises(ValueError, match="puct_search: params.*GPU"):            # without noise noise_eps is not looked at
        puct_search(boards, dice, torch.zeros(n), 8, noise_eps=NAN)
    with pytest.raises(ValueError, match="puct_search: params"):
        puct_search(boards, dice, torch.zeros(n + 1), 8)
    with pytest.raises(ValueError):
        puct_search(torch.zeros((4, 6, 6), dtype=torch.int8), dice, torch.zeros(n), 8)
    # fused= and a table: refused before the table, the tensors or the GPU are looked at
    for f, who in ((predict_puct, "predict_puct"), (selfplay_puct, "selfplay_puct")):
        with pytest.raises(ValueError, match="%s: fused=True does not take an endgame_table" % who):
            f(boards, dice, torch.zeros(n), sims=4, fused=True, endgame_table=object())
        with pytest.raises(ValueError, match="%s: params.*GPU" % who):           # fused alone goes on to the usual checks
            f(boards, dice, torch.zeros(n), sims=4, fused=True)


def test_agent_spec_and_trainers_take_fused(monkeypatch):
    torch = pytest.importorskip("torch")
    from classical_policies.model import PuctAgent
    from ewn_gym_amd.distill import PuctSelfPlayTrainer, SearchDistillTrainer
    from ewn_gym_amd.tournament import evaluate_model
    n = _lib.load().ewn_policy_param_count(5, 3)
    assert inspect.signature(PuctAgent.__init__).parameters["fused"].default is False
    with pytest.raises(ValueError, match="PuctAgent: fused=True does not take an endgame_table"):    # before the model is looked at
        PuctAgent(torch.zeros(n), sims=4, fused=True, endgame_table="nowhere.pt")
    real = torch.Tensor.to                 # the constructor on a host without a device: its parameters stay where they are
    monkeypatch.setattr(torch.Tensor, "to", lambda t, *a, **k: t if a[:1] == ("cuda",) else real(t, *a, **k))
    assert PuctAgent(torch.zeros(n), sims=4).fused is False and PuctAgent(torch.zeros(n), sims=4, fused=True).fused is True
    from ewn_gym_amd.tournament import _policy
    assert callable(_policy({"kind": "mlp_puct", "model": torch.zeros(n), "sims": 4, "fused": True}, 3, 0))
    with pytest.raises(ValueError, match="fused=True does not take an endgame_table"):
        _policy({"kind": "mlp_puct", "model": torch.zeros(n), "sims": 4, "fused": True, "endgame_table": "nowhere.pt"}, 3, 0)
    for f in (SearchDistillTrainer.__init__, PuctSelfPlayTrainer.__init__, evaluate_model):
        assert inspect.signature(f).parameters["fused"].default is False


def test_both_command_lines_accept_fused():
    pytest.importorskip("torch")
    from ewn_gym_amd import tournament, train_a2c
    ap = tournament._parser()
    assert ap.parse_args(["--model", "best.pt", "--puct", "64"]).fused is False
    assert ap.parse_args(["--model", "best.pt", "--puct", "64", "--fused"]).fused is True
    ap = train_a2c._parser()
    assert ap.parse_args(["SELFPLAY"]).fused is False and ap.parse_args(["SEARCH", "--search", "puct"]).fused is False
    assert ap.parse_args(["SELFPLAY", "--fused"]).fused is True
    a = ap.parse_args(["SEARCH", "--search", "puct", "--sims", "16", "--fused"])
    assert (a.algorithm, a.search, a.sims, a.fused) == ("SEARCH", "puct", 16, True)
