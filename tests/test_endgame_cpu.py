"""The endgame table on the host: declarations and exports, ewn_endgame_table_bytes against the formula, every refusal of
ewn_endgame_build / ewn_endgame_lookup and their order on small fake addresses (each call returns before a launch), the bindings'
ValueErrors, and what EndgameAgent, the tournament kind and the train_a2c flag do without a GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest

from ewn_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL = 0, -2, -1


def formula(S, K, T):
    n = lambda k: math.comb(6, k) * (S * S) ** k   # noqa: E731
    return 4 * sum(n(a) * n(o) for a in range(1, K + 1) for o in range(1, K + 1) if a + o <= T)


def p(a):
    return None if a is None else C.c_void_p(a)


def build(S=5, K=2, T=4, table=16, table_bytes=None):
    nb = formula(S, K, T) if table_bytes is None else table_bytes
    return _lib.load().ewn_endgame_build(S, K, T, p(table), nb, None)


def lookup(S=5, K=2, T=4, table=16, M=4, boards=16, dice=16, actions=16, q=None, value=None, covered=None):
    return _lib.load().ewn_endgame_lookup(S, K, T, p(table), M, p(boards), p(dice), p(actions), p(q), p(value), p(covered), None)


def test_declared_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert re.search(r"^int64_t ewn_endgame_table_bytes\(", hdr, re.M)
    for name in ("ewn_endgame_build", "ewn_endgame_lookup"):
        assert re.search(r"^int %s\(" % name, hdr, re.M)
    for name in ("ewn_endgame_table_bytes", "ewn_endgame_build", "ewn_endgame_lookup"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.ewn_abi_version() == 4 and re.search(r"^#define EWN_ABI_VERSION 4\b", hdr, re.M)     # additive
    assert os.path.exists(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_endgame.hip"))
    from ewn_gym_amd import build as b
    assert "ewn_endgame.hip" not in b.FILE_FLAGS and any(s.endswith("ewn_endgame.hip") for s in b.SRC)   # picked up by itself, no per-file flag


def test_table_bytes():
    tb = _lib.load().ewn_endgame_table_bytes
    assert tb(3, 2, 4) == 4 * 1610361 and tb(3, 3, 4) == 4 * 3185001 and tb(4, 2, 4) == 4 * 15492096
    assert tb(5, 2, 4) == 362902500 and tb(5, 3, 5) == 24175402500
    assert tb(7, 2, 4) > 2 ** 32 and tb(7, 2, 4) == formula(7, 2, 4)
    assert tb(5, 1, 2) == formula(5, 1, 2) == 4 * 150 * 150 and tb(11, 1, 2) == formula(11, 1, 2)
    for S in range(3, 12):
        for K in (1, 2, 3):
            for T in range(2, 2 * K + 1):
                assert tb(S, K, T) == formula(S, K, T), (S, K, T)
    for bad in ((2, 2, 4), (12, 2, 4), (5, 0, 2), (5, 0, 0), (5, 4, 4), (5, 2, 1), (5, 2, 5), (5, 1, 3), (5, 3, 7), (-1, 2, 4)):
        assert tb(*bad) == EINVAL, bad


def test_build_refusals_and_their_order():
    assert build(S=2) == EINVAL and build(K=4) == EINVAL and build(T=1) == EINVAL and build(T=5) == EINVAL
    assert build(S=12, table=None) == EINVAL                       # the parameters come before the pointer
    assert build(table=None) == ENULL
    assert build(table=None, table_bytes=8) == ENULL               # ... and the pointer before the size
    assert build(table_bytes=formula(5, 2, 4) - 4) == EINVAL and build(table_bytes=0) == EINVAL and build(table_bytes=formula(5, 2, 3)) == EINVAL
    for addr in (17, 18, 19):
        assert build(table=addr) == EINVAL                         # not 4-byte aligned


def test_build_refuses_a_level_of_more_than_2_31_workgroups():
    """three cubes a side and six in all from 6x6 on: block (3, 3) alone has 20 * 36^3 = 933 120 side indices a side and 3 645
    workgroups per agent side, 3.40 x 10^9 at one level.  The refusal comes before anything touches the table (16 is no address),
    and after the checks of the pointer and the size.  (No shape that passes is built here: it would go on to the device.)"""
    EUNSUPPORTED = -4
    assert _lib.load().ewn_strerror(EUNSUPPORTED) != _lib.load().ewn_strerror(EINVAL)
    assert -(-(20 * 36 ** 3) // 256) * (20 * 36 ** 3) == 3645 * 933120 > 2 ** 31 - 1
    for S in (6, 7, 11):
        assert build(S=S, K=3, T=6) == EUNSUPPORTED, S
    assert build(S=6, K=3, T=6, table_bytes=formula(6, 3, 6) - 4) == EINVAL and build(S=6, K=3, T=6, table_bytes=formula(6, 3, 5)) == EINVAL
    assert build(S=6, K=3, T=6, table=18) == EINVAL
    assert build(S=6, K=3, T=6, table=None) == ENULL and build(S=6, K=3, T=6, table=None, table_bytes=8) == ENULL


def test_lookup_refusals_and_their_order():
    assert lookup(M=-1) == EINVAL and lookup(M=-1, table=None) == EINVAL
    assert lookup(S=2, M=0) == EINVAL and lookup(K=0, M=0) == EINVAL and lookup(T=5, M=0) == EINVAL   # the parameters before the empty batch
    assert lookup(M=0) == OK
    assert lookup(M=0, table=None, boards=None, dice=None, actions=None) == OK
    assert lookup(M=0, table=18) == OK                             # nothing is looked at for an empty batch
    for name in ("table", "boards", "dice", "actions"):
        assert lookup(**{name: None}) == ENULL
        assert lookup(S=7, K=3, T=5, **{name: None}) == ENULL
    assert lookup(table=18, boards=None) == ENULL                  # the pointers before the alignment
    for addr in (17, 18, 19):
        assert lookup(table=addr) == EINVAL
        assert lookup(table=addr, q=16, value=16, covered=16) == EINVAL


def test_the_bindings_check_their_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.endgame import EndgameTable
    assert ewn_gym_amd.EndgameTable is EndgameTable and "EndgameTable" in ewn_gym_amd.__all__
    assert EndgameTable.table_bytes(5, 2) == 362902500 and EndgameTable.table_bytes(5, 3, 5) == 24175402500
    for bad in ((2, 2, None), (5, 4, None), (5, 2, 5), (5, 2, 1)):
        with pytest.raises(ValueError, match="board_size 3..11"):
            EndgameTable.build(*bad)
        with pytest.raises(ValueError, match="board_size 3..11"):
            EndgameTable(*bad, torch.zeros(4))
    n = EndgameTable.table_bytes(3, 1) // 4
    with pytest.raises(ValueError, match="float32 tensor of %d elements" % n):
        EndgameTable(3, 1, 2, torch.zeros(n + 1))
    with pytest.raises(ValueError, match="float32 tensor"):
        EndgameTable(3, 1, 2, torch.zeros(n, dtype=torch.float64))
    with pytest.raises(ValueError, match="GPU"):
        EndgameTable.build(3, 1, out=torch.zeros(n))
    t = EndgameTable(3, 1, None, torch.zeros(n))                   # a host table: enough to construct, not to look up
    assert (t.board_size, t.max_cubes, t.max_total, t.levels) == (3, 1, 2, 8) and t.table.numel() == n
    boards, dice = torch.zeros((4, 3, 3), dtype=torch.int8), torch.ones(4, dtype=torch.int8)
    with pytest.raises(ValueError, match="GPU"):
        t.lookup(boards, dice)
    with pytest.raises(ValueError, match="shape"):
        t.lookup(torch.zeros((4, 3, 4), dtype=torch.int8), dice)
    with pytest.raises(ValueError, match="the table is for 3x3"):
        t.lookup(torch.zeros((4, 5, 5), dtype=torch.int8), dice)
    with pytest.raises(ValueError, match="EndgameTable.lookup: boards.*not contiguous"):
        t.lookup(torch.zeros((4, 3, 8), dtype=torch.int8)[:, :, :3], dice)
    with pytest.raises(ValueError, match="boards"):                # int64 boards are not converted behind the caller's back
        t.lookup(boards.to(torch.int64), dice)
    with pytest.raises(ValueError, match="dice"):
        t.lookup(boards, torch.ones(3, dtype=torch.int8))


def test_the_agent_and_the_tournament_kind_construct():
    torch = pytest.importorskip("torch")
    import classical_policies as cp
    from classical_policies.model import EndgameAgent
    from ewn_gym_amd.endgame import EndgameTable
    from ewn_gym_amd.tournament import _parser, _policy
    assert cp.EndgameAgent is EndgameAgent and "EndgameAgent" in cp.__all__ and issubclass(EndgameAgent, cp.PolicyBase)
    t = EndgameTable(3, 1, 2, torch.zeros(EndgameTable.table_bytes(3, 1) // 4))

    class Fallback:
        board_size = 3

        def predict_batch(self, boards, dice):
            raise AssertionError("not reached on the host")

    agent = EndgameAgent(t, Fallback())
    assert agent.table is t and agent.board_size == 3 and callable(agent.policy_fn())
    with pytest.raises(ValueError, match="predict_batch"):
        EndgameAgent(t, object())
    with pytest.raises(ValueError, match="EndgameTable"):
        EndgameAgent(torch.zeros(3), Fallback())
    Fallback.board_size = 5
    with pytest.raises(ValueError, match="3x3"):
        EndgameAgent(t, Fallback())
    assert callable(_policy({"kind": "endgame", "table": t, "fallback": {"kind": "random"}}, 3, 1))
    with pytest.raises(ValueError, match="fallback"):
        _policy({"kind": "endgame", "table": t}, 3, 1)
    with pytest.raises(ValueError, match="unknown agent kind"):
        _policy({"kind": "endgame", "table": t, "fallback": {"kind": "nope"}}, 3, 1)
    assert _parser().parse_args(["--model", "m.pt", "--endgame_table", "t.pt"]).endgame_table == "t.pt"
    assert _parser().parse_args([]).endgame_table is None


def test_the_trainer_takes_the_keyword_and_train_a2c_lists_the_flag():
    pytest.importorskip("torch")
    import inspect
    from ewn_gym_amd.distill import SearchDistillTrainer
    assert inspect.signature(SearchDistillTrainer.__init__).parameters["endgame_table"].default is None
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ewn_gym_amd.train_a2c", "SEARCH", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--endgame_table" in r.stdout
