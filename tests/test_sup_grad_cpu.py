"""ewn_sup_grad / ewn_sup_scratch_bytes / ewn_lookahead_targets on the host: declarations and exports, the arguments the entry points
refuse before anything is launched and the order they refuse them in, the checks of the Python bindings sup_grad and lookahead_targets
(no kernel runs here), the trainer's import and the SEARCH sub-command's argument parser."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
SUP_POINTERS = ["boards", "dice", "target_pi", "target_value", "params", "grad", "scratch"]


def p(a):
    """a small fake address where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return None if a is None else C.c_void_p(a)


def sup(board_size=5, cube_layer=3, M=4, boards=16, dice=16, target_pi=16, target_value=16, weight=None, params=16, pi_coef=1.0, vf_coef=0.5,
        grad=16, scratch=16):
    return _lib.load().ewn_sup_grad(board_size, cube_layer, M, p(boards), p(dice), p(target_pi), p(target_value), p(weight), p(params),
                                    pi_coef, vf_coef, p(grad), p(scratch), None)


def targets(M=4, q=16, temperature=0.0, target_pi=16, target_value=16, weight=16):
    return _lib.load().ewn_lookahead_targets(M, p(q), temperature, p(target_pi), p(target_value), p(weight), None)


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int64_t ewn_sup_scratch_bytes\(int board_size, int cube_layer, int M\);", hdr, re.M)
    assert re.search(r"^int ewn_sup_grad\(", hdr, re.M) and re.search(r"^int ewn_lookahead_targets\(", hdr, re.M)
    for name in ("ewn_sup_scratch_bytes", "ewn_sup_grad", "ewn_lookahead_targets"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.ewn_abi_version() == 4          # the exports are additive
    assert re.search(r"#define EWN_ABI_VERSION 4\b", hdr)


def test_scratch_bytes():
    lib = _lib.load()
    for S in (5, 7):
        P = lib.ewn_policy_param_count(S, 3)
        stride = (S * S + 6 + 15) & ~15
        for M in (1, 33, 327680):
            n = lib.ewn_sup_scratch_bytes(S, 3, M)
            assert n >= 256 * (P + 8) * 4 + M * stride and n <= 256 * (P + 8) * 4 + M * stride + 64, (S, M, n)
    assert lib.ewn_sup_scratch_bytes(5, 3, 0) == EINVAL and lib.ewn_sup_scratch_bytes(5, 3, -3) == EINVAL
    assert lib.ewn_sup_scratch_bytes(6, 3, 0) == EINVAL                         # M comes first
    for S, L in ((6, 3), (8, 3), (5, 2), (7, 4), (4, 3)):
        assert lib.ewn_sup_scratch_bytes(S, L, 4) == EUNSUPPORTED, (S, L)
    for S in range(3, 12):
        for L in range(1, 5):
            assert (lib.ewn_sup_scratch_bytes(S, L, 4) > 0) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)


def test_sup_grad_refusals_and_their_order():
    assert sup(M=0) == EINVAL and sup(M=-1) == EINVAL
    assert sup(M=0, board_size=6) == EINVAL                                    # 1. M
    assert sup(M=0, boards=None, vf_coef=-1.0) == EINVAL
    for S in (6, 8):
        assert sup(board_size=S) == EUNSUPPORTED                               # 2. geometry
        assert sup(board_size=S, boards=None) == EUNSUPPORTED
        assert sup(board_size=S, vf_coef=-1.0) == EUNSUPPORTED
    for L in (2, 4):
        assert sup(cube_layer=L) == EUNSUPPORTED and sup(board_size=7, cube_layer=L) == EUNSUPPORTED
    for name in SUP_POINTERS:                                                  # 3. pointers
        assert sup(**{name: None}) == ENULL, name
        assert sup(board_size=7, **{name: None}) == ENULL, name
        assert sup(vf_coef=-1.0, **{name: None}) == ENULL, name                # ... before the coefficients
        assert sup(pi_coef=float("nan"), **{name: None}) == ENULL, name
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):              # 4. coefficients
        assert sup(vf_coef=bad) == EINVAL, bad
        assert sup(pi_coef=bad) == EINVAL, bad
        assert sup(board_size=7, weight=16, vf_coef=bad) == EINVAL, bad
    # M whose tile count would overflow an int; a scratch that cannot hold floats (looked at last)
    big = 2 ** 31 - 1
    assert sup(M=big) == EINVAL and sup(M=big, board_size=6) == EINVAL and sup(M=big - 32896, boards=None) == ENULL   # the largest M served
    assert _lib.load().ewn_sup_scratch_bytes(5, 3, big) == EINVAL and _lib.load().ewn_sup_scratch_bytes(5, 3, big - 32896) > 0
    for off in (1, 2, 3):
        assert sup(scratch=16 + off) == EINVAL, off
        assert sup(scratch=16 + off, boards=None) == ENULL and sup(scratch=16 + off, board_size=6) == EUNSUPPORTED


def test_lookahead_targets_refusals():
    assert targets(M=-1) == EINVAL
    assert targets(M=-1, q=None) == EINVAL
    assert targets(M=0) == OK
    assert targets(M=0, q=None, target_pi=None, target_value=None, weight=None) == OK
    for name in ("q", "target_pi", "target_value", "weight"):
        assert targets(**{name: None}) == ENULL, name
        assert targets(temperature=float("nan"), **{name: None}) == ENULL, name
    for bad in (float("nan"), float("inf"), float("-inf"), -0.5):
        assert targets(temperature=bad) == EINVAL, bad


def test_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.vec_env import lookahead_targets, sup_grad
    assert ewn_gym_amd.sup_grad is sup_grad and ewn_gym_amd.lookahead_targets is lookahead_targets
    assert "sup_grad" in ewn_gym_amd.__all__ and "lookahead_targets" in ewn_gym_amd.__all__
    n = _lib.load().ewn_policy_param_count(5, 3)
    M = 4
    boards, dice = torch.zeros((M, 5, 5), dtype=torch.int8), torch.ones(M, dtype=torch.int8)
    tp, tv, params = torch.zeros((M, 5)), torch.zeros(M), torch.zeros(n)
    with pytest.raises(ValueError, match="params"):            # a 7x7 vector for 5x5 boards
        sup_grad(boards, dice, tp, tv, torch.zeros(_lib.load().ewn_policy_param_count(7, 3)))
    with pytest.raises(ValueError, match="params"):
        sup_grad(boards, dice, tp, tv, params.double())
    with pytest.raises(ValueError, match="GPU"):               # everything well-formed, but host tensors
        sup_grad(boards, dice, tp, tv, params)
    with pytest.raises(ValueError, match="GPU"):
        sup_grad(np.zeros((5, 5), np.int8), [3], np.zeros((1, 5), np.float32), [0.0], params)
    with pytest.raises(ValueError, match="sup_grad: boards.*not contiguous"):
        sup_grad(torch.zeros((M, 5, 8), dtype=torch.int8)[:, :, :5], dice, tp, tv, params)
    with pytest.raises(ValueError, match="boards"):            # int64 boards are not converted behind the caller's back
        sup_grad(boards.to(torch.int64), dice, tp, tv, params)
    with pytest.raises(ValueError, match="dice"):
        sup_grad(boards, torch.ones(3, dtype=torch.int8), tp, tv, params)
    with pytest.raises(ValueError, match="target_pi"):
        sup_grad(boards, dice, torch.zeros((M, 6)), tv, params)
    with pytest.raises(ValueError, match="target_pi"):
        sup_grad(boards, dice, tp.double(), tv, params)
    with pytest.raises(ValueError, match="target_value"):
        sup_grad(boards, dice, tp, torch.zeros(M + 1), params)
    with pytest.raises(ValueError, match="weight"):
        sup_grad(boards, dice, tp, tv, params, weight=torch.zeros(M, dtype=torch.float64))
    with pytest.raises(ValueError, match="out"):
        sup_grad(boards, dice, tp, tv, params, out=torch.zeros(n))
    with pytest.raises(ValueError, match="scratch"):
        sup_grad(boards, dice, tp, tv, params, scratch=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="4-byte aligned.*1 past"):
        sup_grad(boards, dice, tp, tv, params, scratch=torch.zeros(2 ** 24 + 64, dtype=torch.uint8)[1:])
    with pytest.raises(ValueError, match="vf_coef"):
        sup_grad(boards, dice, tp, tv, params, vf_coef=-1.0)
    with pytest.raises(ValueError, match="pi_coef"):
        sup_grad(boards, dice, tp, tv, params, pi_coef=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        sup_grad(torch.zeros((M, 5, 6), dtype=torch.int8), dice, tp, tv, params)
    with pytest.raises(ValueError, match="6x6"):
        sup_grad(torch.zeros((M, 6, 6), dtype=torch.int8), dice, tp, tv, params)
    with pytest.raises(ValueError, match="at least one"):
        sup_grad(torch.zeros((0, 5, 5), dtype=torch.int8), dice[:0], tp[:0], tv[:0], params)
    # lookahead_targets
    with pytest.raises(ValueError, match="shape"):
        lookahead_targets(torch.zeros((M, 5)))
    with pytest.raises(ValueError, match="shape"):
        lookahead_targets(torch.zeros((M, 3, 2)))
    with pytest.raises(ValueError, match="temperature"):
        lookahead_targets(torch.zeros((M, 2, 3)), temperature=float("nan"))
    with pytest.raises(ValueError, match="temperature"):
        lookahead_targets(torch.zeros((M, 6)), temperature=-1.0)
    with pytest.raises(ValueError, match="q must"):
        lookahead_targets(torch.zeros((M, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="GPU"):
        lookahead_targets(torch.zeros((M, 2, 3)))


def test_trainer_is_importable_and_the_sub_command_parses():
    pytest.importorskip("torch")
    from ewn_gym_amd.distill import SearchDistillTrainer
    assert SearchDistillTrainer.algorithm == "SEARCH"
    for name in ("collect_and_update", "learn", "stats_dict", "policy_fn", "save", "load"):
        assert callable(getattr(SearchDistillTrainer, name))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SEARCH", "--plies", "2", "--temperature", "0.5", "--terminal_value", "1",
                        "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--plies", "--temperature", "--terminal_value", "SEARCH"):
        assert flag in r.stdout


def test_search_refuses_flags_that_do_not_apply():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for extra in (["--trainer", "torch"], ["--batch_size", "64"]):
        r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SEARCH"] + extra, cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode != 0 and "SearchDistillTrainer" in r.stderr, (extra, r.stderr[-500:])


def test_the_placeholder_points_at_the_trainer():
    import classical_policies as cp
    with pytest.raises(NotImplementedError, match="SearchDistillTrainer"):
        cp.AlphaZeroAgent(cube_layer=3, board_size=5)
