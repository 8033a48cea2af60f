"""The PUCT search with several leaves per tree and round on the host (ewn_puct_search_wide): the header of its own and
the export list, what the entry point refuses before anything is launched and the order it looks at it in (ewn_puct_search's, then
leaves, tile and blocks, noise_eps last and only with root noise), the size function, the bindings' ValueErrors, the leaves= keyword
at every level -- and the definition itself as a numpy model, WideModel: tests/test_gpu_puct.py's Model with the marks, the wide walk
and the round of two halves, driven here by a fake deterministic network.  tests/test_gpu_puct_wide.py compares the kernel's trees
with that model field by field.  No kernel runs here."""
import ctypes as C
import inspect
import os
import re
import zlib

import numpy as np
import pytest

from ewn_gym_amd import _lib

pytest.importorskip("torch")

from tests.test_gpu_puct import F, FIELDS, Model, edges, flip, prior64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENULL, EINVAL, EUNSUPPORTED = 0, -2, -1, -4
INT_MAX = 2 ** 31 - 1
M_LAST = INT_MAX // 64
NAN, INF = float("nan"), float("inf")
BEGUN, LEAF, COLLISION = 0, 1, 2


# ---------------------------------------------------------------- the model of the definition

class WideModel(Model):
    """Model with the marks vn, vcn and a round of two halves.  pend: the pending nodes, ascending.  It counts its rounds, those that
    collected at least two leaves (wide_rounds), the most leaves a round collected and the walks that ended on a collision"""

    def __init__(self, board, dice, sims, leaves):
        super().__init__(board, dice, sims)
        N = sims + 1
        self.L = leaves
        self.vn, self.vcn = np.zeros((N, 6), np.int32), np.zeros((N, 6, 6), np.int32)
        self.pend = [] if self.degenerate else [0]
        self.rounds = self.wide_rounds = self.collisions = self.most = 0

    def busy(self):
        return not self.degenerate and (bool(self.pend) or self.done < self.sims)

    def rows(self):
        """the pending nodes' observations, column by column"""
        return [(self.t["board"][j], int(self.t["dice"][j])) for j in self.pend]

    def unmark(self, j):
        t = self.t
        while t["parent"][j, 0] >= 0:
            p, a, d = (int(x) for x in t["parent"][j, :3])
            self.vn[p, a] -= 1
            self.vcn[p, a, d - 1] -= 1
            j = p

    def round(self, outputs, c, inv_tv, gpu_p):
        """one round: outputs = [(logits, V)] for the pending nodes in order; gpu_p [nodes, 6]: the priors to adopt -> [(node, the
        float64 prior)] of the nodes evaluated"""
        t, out = self.t, []
        assert len(outputs) == len(self.pend) <= self.L
        for j, (logits, V) in zip(self.pend, outputs):             # (A) evaluate, in ascending order
            self.unmark(j)
            kind, _, one = edges(t["board"][j], int(t["dice"][j]))
            t["kind"][j], t["p"][j] = kind, gpu_p[j]
            out.append((j, prior64(logits, kind, one)))
            v = F(F(V) * inv_tv)
            v = v if v > F(-1) else F(-1)
            v = v if v < F(1) else F(1)
            self.backup(j, v)
        self.pend, count0 = [], self.count
        while len(self.pend) < self.L and self.done < self.sims:   # (B) walk
            r = self.walk(c, count0)
            if r == COLLISION:
                self.collisions += 1
                break
            self.done += 1
            if r == LEAF:
                self.pend.append(self.count - 1)
        self.pending = -1                                          # the header's word once the search is over
        self.rounds += 1
        self.wide_rounds += len(self.pend) >= 2
        self.most = max(self.most, len(self.pend))
        return out

    def walk(self, c, count0):
        """Model.simulate on n + vn, w - (float)vn and cn + vcn"""
        t, j = self.t, 0
        while True:
            kind, b1, _ = edges(t["board"][j], int(t["dice"][j]))
            vn = self.vn[j]
            n, w, p = t["n"][j] + vn, (t["w"][j] - vn.astype(F)).astype(F), t["p"][j]
            rs = np.sqrt(F(int(n.sum()) + 1))                      # correctly rounded
            best, sb = -1, F(0)
            for a in range(6):
                if kind[a] == 0:
                    continue
                q = F(w[a] / F(n[a])) if n[a] > 0 else F(0)
                s = F(q + F(F(F(c * p[a]) * rs) / F(1 + int(n[a]))))
                if best < 0 or s > sb:
                    best, sb = a, s
            a = best
            if kind[a] == 1:                                       # 1. the edge wins
                self.unmark(j)
                t["w"][j, a] = F(t["w"][j, a] + F(1))
                t["n"][j, a] += 1
                self.backup(j, F(1))
                return BEGUN
            d = int(np.argmin(t["cn"][j, a].astype(np.int32) + self.vcn[j, a])) + 1      # the first minimum
            ch = int(t["child"][j, a, d - 1])
            if ch >= count0:                                       # 2. created in this round: a collision
                self.unmark(j)
                return COLLISION
            self.vn[j, a] += 1                                     # 3. marked, and down
            self.vcn[j, a, d - 1] += 1
            if ch >= 0:
                j = ch
                continue
            idx = self.count
            self.count += 1
            t["child"][j, a, d - 1], t["board"][idx], t["dice"][idx], t["parent"][idx] = idx, flip(b1[a]), d, (j, a, d, 0)
            return LEAF


def fake_network(board, dice):
    """five logits and a value that depend on the observation alone"""
    rs = np.random.RandomState(zlib.crc32(np.ascontiguousarray(board).tobytes() + bytes([int(dice)])))
    return rs.normal(size=5).astype(F), F(rs.uniform(-1.2, 1.2))


def fake_prior(board, dice, logits):
    kind, _, one = edges(board, dice)
    return prior64(logits, kind, one).astype(F)


def opening(S=5):
    b = np.zeros((S, S), np.int8)
    for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0))):
        b[r, c], b[S - 1 - r, S - 1 - c] = (3, 1, 6, 2, 5, 4)[k], -(4, 6, 2, 1, 3, 5)[k]
    return b


def run_wide(board, dice, sims, leaves, c=F(1.5), inv_tv=F(1)):
    m = WideModel(board, dice, sims, leaves)
    gp = np.zeros((sims + 1, 6), F)
    while m.busy():
        assert m.rounds <= sims, "more than sims + 1 rounds"
        outs = [fake_network(b, d) for b, d in m.rows()]
        for j, (b, d), (lg, _) in zip(m.pend, m.rows(), outs):
            gp[j] = fake_prior(b, d, lg)
        m.round(outs, c, inv_tv, gp)
    return m


def run_plain(board, dice, sims, c=F(1.5), inv_tv=F(1)):
    m = Model(board, dice, sims)
    gp = np.zeros((sims + 1, 6), F)
    for _ in range(sims + 1):
        b, d = m.leaf()
        lg, V = fake_network(b, d)
        if m.pending >= 0:
            gp[m.pending] = fake_prior(b, d, lg)
        m.advance(lg, V, c, inv_tv, gp)
    return m


@pytest.mark.parametrize("dice", [1, 4])
@pytest.mark.parametrize("sims", [6, 17, 64])
def test_one_leaf_is_the_plain_model(dice, sims):
    wide, plain = run_wide(opening(), dice, sims, 1), run_plain(opening(), dice, sims)
    assert (wide.count, wide.done, wide.pending, wide.rounds) == (plain.count, plain.done, plain.pending, sims + 1)
    for name in FIELDS:
        assert np.array_equal(wide.t[name], plain.t[name]), name
    for name in ("w", "p"):
        assert np.array_equal(wide.t[name].view(np.int32), plain.t[name].view(np.int32)), name
    assert wide.collisions == 0 and wide.wide_rounds == 0 and not wide.vn.any() and not wide.vcn.any()


@pytest.mark.parametrize("dice", [1, 4])
@pytest.mark.parametrize("sims", [5, 64])
@pytest.mark.parametrize("leaves", [2, 4, 8, 32])
def test_a_wide_search_ends_with_its_budget_begun_and_no_mark_left(dice, sims, leaves):
    m = run_wide(opening(), dice, sims, leaves)
    assert m.done == sims and m.count == sims + 1 and int(m.t["n"][0].sum()) == sims and not m.pend
    assert not m.vn.any() and not m.vcn.any()
    assert -(-sims // leaves) + 1 <= m.rounds <= sims + 1 and m.most <= leaves
    if sims == 64:
        assert m.rounds < 65 and m.wide_rounds > 0
        print("L = %d, dice %d: %d rounds for 64 simulations, at most %d leaves a round, %d collisions" % (
            leaves, dice, m.rounds, m.most, m.collisions))


def test_the_collision_rule_fires():
    assert sum(run_wide(opening(), d, 64, 32).collisions for d in (1, 4)) > 0


# ---------------------------------------------------------------- the C ABI

def p(a):
    return None if a is None else C.c_void_p(a)


def search(board_size=5, cube_layer=3, M=4, sims=8, leaves=4, c_puct=1.5, terminal_value=1.0, boards=16, dice=16, params=16,
           root_noise=16, noise_eps=0.25, tile=0, blocks=0, tree=16, scratch=16):
    """small fake addresses where a pointer is needed: never dereferenced, every call here returns before a launch"""
    return _lib.load().ewn_puct_search_wide(board_size, cube_layer, M, sims, leaves, c_puct, terminal_value, p(boards), p(dice), p(params),
                                            p(root_noise), noise_eps, tile, blocks, p(tree), p(scratch), None)


def test_the_entries_are_declared_in_a_header_of_their_own_and_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ewn_puct_wide.h")).read()
    assert re.search(r"^int ewn_puct_search_wide\(", hdr, re.M) and re.search(r"^int64_t ewn_puct_search_wide_scratch_bytes\(", hdr, re.M)
    assert '#include "ewn_hip.h"' in hdr and "ewn_puct_search_wide" not in open(os.path.join(ROOT, "include", "ewn_hip.h")).read()
    assert _lib.EXPORTS_PUCT_WIDE == ["ewn_puct_search_wide_scratch_bytes", "ewn_puct_search_wide"]
    assert not set(_lib.EXPORTS_PUCT_WIDE) & set(_lib.EXPORTS)
    at = lib.ewn_puct_search_wide.argtypes
    assert len(at) == 17 and lib.ewn_puct_search_wide.restype is C.c_int
    assert [i for i, t in enumerate(at) if t is C.c_float] == [5, 6, 11]          # c_puct, terminal_value; noise_eps
    assert all(at[i] is C.c_int for i in (0, 1, 2, 3, 4, 12, 13))                 # ... leaves the fifth integer; tile, blocks
    assert all(at[i] is C.c_void_p for i in (7, 8, 9, 10, 14, 15, 16))
    assert lib.ewn_puct_search_wide_scratch_bytes.restype is C.c_int64 and lib.ewn_puct_search_wide_scratch_bytes.argtypes == [C.c_int] * 4
    assert lib.ewn_abi_version() == 4                                             # the exports are additive
    from ewn_gym_amd import build as b
    assert b.FILE_FLAGS["ewn_puct_wide.hip"] == ["-fno-slp-vectorize"] and any(s.endswith("ewn_puct_wide.hip") for s in b.SRC)
    assert any(d.endswith("ewn_puct_wide.h") for d in b.DEPS)
    src = open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_wide.hip")).read()
    assert "pol_launch_kernel(k_puct_search_wide<S, NOISE>" in src and "getenv" not in src and "atomic" not in src.replace("No atomics", "")
    assert '#include "ewn_puct.hpp"' in open(os.path.join(ROOT, "ewn_gym_amd", "csrc", "ewn_puct_wide.hpp")).read()


def test_the_size_function():
    f = _lib.load().ewn_puct_search_wide_scratch_bytes
    assert f(5, 3, 0, 64) == 0 and f(7, 3, 0, 0) == 0
    for S in (5, 7):
        for M, sims in ((1, 0), (9, 12), (1024, 64), (16384, 256), (M_LAST, 4096)):
            n = f(S, 3, M, sims)
            assert n > 0 and n % 4 == 0 and n % M == 0 and n == M * f(S, 3, 1, sims)           # a tree's marks, back to back
            assert n >= M * (sims + 1) * (6 + 36)                                             # room for vn and vcn of every node
    assert f(5, 3, -1, 8) == EINVAL and f(5, 3, M_LAST + 1, 8) == EINVAL and f(6, 3, -1, 8) == EINVAL
    assert f(6, 3, 4, 8) == EUNSUPPORTED and f(5, 2, 4, 8) == EUNSUPPORTED and f(6, 3, 4, -1) == EUNSUPPORTED
    assert f(5, 3, 4, -1) == EINVAL and f(5, 3, 4, 4097) == EINVAL and f(7, 3, 0, 4097) == EINVAL


@pytest.mark.parametrize("name", ["boards", "dice", "params", "tree", "scratch"])
def test_missing_pointer(name):
    assert search(**{name: None}) == ENULL
    assert search(board_size=7, **{name: None}) == ENULL
    assert search(sims=4097, **{name: None}) == ENULL                    # the pointers come before the values
    assert search(terminal_value=NAN, **{name: None}) == ENULL and search(c_puct=-1.0, **{name: None}) == ENULL
    assert search(leaves=0, **{name: None}) == ENULL and search(tile=33, **{name: None}) == ENULL and search(blocks=-1, **{name: None}) == ENULL
    assert search(noise_eps=2.0, **{name: None}) == ENULL and search(noise_eps=NAN, **{name: None}) == ENULL
    assert search(M=M_LAST, **{name: None}) == ENULL
    assert search(root_noise=None, **{name: None}) == ENULL


def test_the_empty_batch_is_ok_with_nothing_touched():
    assert search(M=0) == OK
    assert search(M=0, boards=None, dice=None, params=None, root_noise=None, tree=None, scratch=None) == OK
    assert search(M=0, board_size=7, sims=4097, terminal_value=0.0, c_puct=NAN, noise_eps=NAN, tree=18, leaves=0, tile=-1, blocks=999) == OK


def test_invalid_and_unsupported_arguments_in_their_order():
    lib = _lib.load()
    assert search(M=-1) == EINVAL and search(M=-1, board_size=6) == EINVAL   # M < 0 comes first
    assert search(M=M_LAST + 1) == EINVAL and search(M=M_LAST + 1, board_size=6) == EINVAL and search(M=M_LAST + 1, tree=None) == EINVAL
    assert search(M=M_LAST, board_size=6) == EUNSUPPORTED                    # in range: the geometry is looked at next
    for S in (6, 8):
        assert search(board_size=S) == EUNSUPPORTED and search(board_size=S, M=0) == EUNSUPPORTED
        assert search(board_size=S, tree=None) == EUNSUPPORTED               # the geometry is looked at before the pointers
        assert search(board_size=S, leaves=0) == EUNSUPPORTED and search(board_size=S, tile=99) == EUNSUPPORTED
    for L in (2, 4):
        assert search(cube_layer=L) == EUNSUPPORTED and search(board_size=7, cube_layer=L) == EUNSUPPORTED
    for S in range(3, 12):                                                   # ... exactly where ewn_policy_param_count is unsupported
        for L in range(1, 5):
            assert (search(board_size=S, cube_layer=L, M=0) == OK) == (lib.ewn_policy_param_count(S, L) > 0), (S, L)
    assert search(tree=18) == EINVAL and search(scratch=18) == EINVAL and search(scratch=17, root_noise=None) == EINVAL
    for sims in (-1, 4097, INT_MAX, -INT_MAX):
        assert search(sims=sims) == EINVAL and search(board_size=7, sims=sims) == EINVAL and search(board_size=6, sims=sims) == EUNSUPPORTED
    for tv in (NAN, INF, -INF, 0.0, -1.0):
        assert search(terminal_value=tv) == EINVAL and search(board_size=8, terminal_value=tv) == EUNSUPPORTED
        assert search(terminal_value=tv, root_noise=None) == EINVAL
    for c in (NAN, INF, -INF, -0.5):
        assert search(c_puct=c) == EINVAL and search(board_size=6, c_puct=c) == EUNSUPPORTED
    for leaves in (0, -1, 33, INT_MAX):
        assert search(leaves=leaves) == EINVAL and search(leaves=leaves, root_noise=None) == EINVAL
        assert search(leaves=leaves, tree=None) == ENULL
    for leaves, most in ((1, 32), (2, 16), (3, 10), (4, 8), (5, 6), (8, 4), (11, 2), (16, 2), (17, 1), (32, 1)):
        for tile in (-1, most + 1, 33, INT_MAX):
            assert search(leaves=leaves, tile=tile) == EINVAL, (leaves, tile)
        assert search(leaves=leaves, tile=most, blocks=257) == EINVAL          # ... tile in range: the grid is looked at
    for blocks in (-1, 257, INT_MAX):
        assert search(blocks=blocks) == EINVAL and search(blocks=blocks, root_noise=None) == EINVAL
    for eps in (NAN, INF, -INF, -0.001, 1.001, 2.0, -1.0):
        assert search(noise_eps=eps) == EINVAL and search(board_size=7, noise_eps=eps) == EINVAL
        assert search(board_size=6, noise_eps=eps) == EUNSUPPORTED           # the geometry is looked at before the weight
        # without root noise the weight is not looked at: the call is accepted up to the pointer checks and the other values
        assert search(noise_eps=eps, root_noise=None, tree=None) == ENULL
        assert search(noise_eps=eps, root_noise=None, leaves=0) == EINVAL and search(noise_eps=eps, root_noise=None, tile=9) == EINVAL
        assert search(noise_eps=eps, root_noise=None, M=0) == OK


# ---------------------------------------------------------------- the bindings

def test_the_binding_checks_its_arguments_before_any_launch():
    torch = pytest.importorskip("torch")
    import ewn_gym_amd
    from ewn_gym_amd.wide import puct_search_wide
    assert "puct_search_wide" in ewn_gym_amd.__all__ and ewn_gym_amd.puct_search_wide is puct_search_wide and ewn_gym_amd.__all__[0] == "VecEWN"
    sig = inspect.signature(puct_search_wide)
    assert list(sig.parameters) == ["boards", "dice", "params", "sims", "leaves", "c_puct", "terminal_value", "root_noise", "noise_eps", "tile",
                                    "blocks", "cube_layer", "out"]
    assert [sig.parameters[k].default for k in ("c_puct", "terminal_value", "root_noise", "noise_eps", "tile", "blocks", "cube_layer", "out")] == [
        1.5, 1.0, None, 0.25, None, None, 3, None]
    assert sig.parameters["leaves"].default is inspect.Parameter.empty
    psig = inspect.signature(ewn_gym_amd.puct_search)                               # the pinned signature stays
    assert list(psig.parameters) == ["boards", "dice", "params", "sims", "c_puct", "terminal_value", "root_noise", "noise_eps", "rounds",
                                     "cube_layer", "out"]
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, eta = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.ones((4, 6))
    z = torch.zeros(n)
    for sims in (-1, 4097, 2.0, None):
        with pytest.raises(ValueError, match="puct_search_wide: sims"):
            puct_search_wide(boards, dice, z, sims, 4)
    for c in (NAN, -1.0):
        with pytest.raises(ValueError, match="puct_search_wide: c_puct"):
            puct_search_wide(boards, dice, z, 8, 4, c_puct=c)
    for tv in (NAN, 0.0, INF):
        with pytest.raises(ValueError, match="puct_search_wide: terminal_value"):
            puct_search_wide(boards, dice, z, 8, 4, terminal_value=tv)
    for leaves in (0, -1, 33, 2.0, None, "4", True):
        with pytest.raises(ValueError, match="puct_search_wide: leaves"):
            puct_search_wide(boards, dice, z, 8, leaves)
    for eps in (NAN, INF, -0.1, 1.5):
        with pytest.raises(ValueError, match="puct_search_wide: noise_eps"):
            puct_search_wide(boards, dice, z, 8, 4, root_noise=eta, noise_eps=eps)
    for leaves, tile in ((4, 0), (4, 9), (4, -1), (4, 1.0), (32, 2), (3, 11)):
        with pytest.raises(ValueError, match="puct_search_wide: tile"):
            puct_search_wide(boards, dice, z, 8, leaves, tile=tile)
    for blocks in (0, -1, 257, 1.5):
        with pytest.raises(ValueError, match="puct_search_wide: blocks"):
            puct_search_wide(boards, dice, z, 8, 4, blocks=blocks)
    with pytest.raises(ValueError, match="puct_search_wide: params.*GPU"):           # everything well-formed, but host tensors
        puct_search_wide(boards, dice, z, 8, 4, tile=8, blocks=256)
    with pytest.raises(ValueError, match="puct_search_wide: params.*GPU"):           # without noise noise_eps is not looked at
        puct_search_wide(boards, dice, z, 8, 4, noise_eps=NAN)
    with pytest.raises(ValueError, match="puct_search_wide: params"):
        puct_search_wide(boards, dice, torch.zeros(n + 1), 8, 4)
    with pytest.raises(ValueError):
        puct_search_wide(torch.zeros((4, 6, 6), dtype=torch.int8), dice, z, 8, 4)


def test_leaves_defaults_to_one_everywhere_and_is_checked_before_any_launch(monkeypatch):
    torch = pytest.importorskip("torch")
    from classical_policies.model import PuctAgent
    from ewn_gym_amd import predict_puct, selfplay_puct
    from ewn_gym_amd.distill import PuctSelfPlayTrainer, SearchDistillTrainer
    from ewn_gym_amd.tournament import _policy, evaluate_model
    for f in (predict_puct, selfplay_puct, PuctAgent.__init__, SearchDistillTrainer.__init__, PuctSelfPlayTrainer.__init__, evaluate_model):
        assert inspect.signature(f).parameters["leaves"].default == 1, f
    n = _lib.load().ewn_policy_param_count(5, 3)
    boards, dice, z = torch.zeros((4, 5, 5), dtype=torch.int8), torch.ones(4, dtype=torch.int8), torch.zeros(n)
    for f, who in ((predict_puct, "predict_puct"), (selfplay_puct, "selfplay_puct")):
        for leaves in (0, 33, 2.5, None):
            with pytest.raises(ValueError, match="%s: leaves must be an integer in 1..32" % who):
                f(boards, dice, z, sims=4, leaves=leaves)
        with pytest.raises(ValueError, match="%s: leaves=4 does not take endgame_table" % who):     # before the table is looked at
            f(boards, dice, z, sims=4, leaves=4, endgame_table=object())
        with pytest.raises(ValueError, match="%s: params.*GPU" % who):                              # leaves alone goes on to the usual checks
            f(boards, dice, z, sims=4, leaves=4)
        with pytest.raises(ValueError, match="%s: params.*GPU" % who):                              # ... whatever fused says
            f(boards, dice, z, sims=4, leaves=4, fused=True)
    with pytest.raises(ValueError, match="PuctAgent: leaves=8 does not take endgame_table"):        # before the model is looked at
        PuctAgent(z, sims=4, leaves=8, endgame_table="nowhere.pt")
    with pytest.raises(ValueError, match="PuctAgent: leaves"):
        PuctAgent(z, sims=4, leaves=0)
    for kw, word in (({"search": "lookahead"}, "search='lookahead'"), ({"search": "puct", "endgame_leaves": True, "endgame_table": "nowhere.pt"},
                                                                       "endgame_leaves=True")):
        with pytest.raises(ValueError, match="SearchDistillTrainer: leaves=4 does not take %s" % word):   # before the env is looked at
            SearchDistillTrainer(None, leaves=4, **kw)
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: leaves=4 does not take endgame_table"):
        PuctSelfPlayTrainer(None, sims=4, leaves=4, endgame_table="nowhere.pt")
    with pytest.raises(ValueError, match="PuctSelfPlayTrainer: leaves=4 does not take whole_games=True"):
        PuctSelfPlayTrainer(None, sims=4, leaves=4, whole_games=True)
    real = torch.Tensor.to                 # the constructor on a host without a device: its parameters stay where they are
    monkeypatch.setattr(torch.Tensor, "to", lambda t, *a, **k: t if a[:1] == ("cuda",) else real(t, *a, **k))
    assert PuctAgent(z, sims=4).leaves == 1 and PuctAgent(z, sims=4, leaves=4, fused=True).leaves == 4
    assert callable(_policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaves": 4}, 3, 0))
    with pytest.raises(ValueError, match="leaves=4 does not take endgame_table"):
        _policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaves": 4, "endgame_table": "nowhere.pt"}, 3, 0)
    with pytest.raises(ValueError, match="PuctAgent: leaves"):
        _policy({"kind": "mlp_puct", "model": z, "sims": 4, "leaves": 40}, 3, 0)


def test_both_command_lines_accept_leaves():
    pytest.importorskip("torch")
    from ewn_gym_amd import tournament, train_a2c
    ap = tournament._parser()
    assert ap.parse_args(["--model", "best.pt", "--puct", "64"]).leaves == 1
    assert ap.parse_args(["--model", "best.pt", "--puct", "64", "--leaves", "8"]).leaves == 8
    ap = train_a2c._parser()
    assert ap.parse_args(["SELFPLAY"]).leaves == 1 and ap.parse_args(["SEARCH", "--search", "puct"]).leaves == 1
    assert ap.parse_args(["SELFPLAY", "--leaves", "4"]).leaves == 4
    a = ap.parse_args(["SEARCH", "--search", "puct", "--sims", "16", "--leaves", "8"])
    assert (a.algorithm, a.search, a.sims, a.leaves) == ("SEARCH", "puct", 16, 8)
