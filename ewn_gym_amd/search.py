"""The calls on a trained actor-critic, stateless and batched: predict_policy, the lookahead on its critic and the lookahead's stages,
the supervised gradient, the PUCT search in stages and in one launch, and the search's self-play.

Host side is plumbing only, as in vec_env.py: torch owns the buffers and the stream, libewn_hip.so does the work.  Every call
checks what it is given before it launches; the checks that all bindings share are _args.py's.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import (_at_least_one, _describe, _finite, _is_buffer, _lookahead_shape, _not_negative, _policy_input, _policy_params,
                    _positive, _ptr, _same_gpu, _stream)
from .endgame import _accept_table

LA_TUPLES = 108        # (agent move, reply) tuples per observation of the lookahead tree (csrc/ewn_lookahead.hpp)
LA_ROWS = 648          # its leaf rows: a tuple under each of the six d2
PUCT_LAYOUT = 1        # the version of a PUCT tree's layout (csrc/ewn_puct.hip); begin writes it into every header
PUCT_MAX_SIMS = 4096
PUCT_FUSED_TILE = 32          # the most trees a block of ewn_puct_search holds at a time (csrc/ewn_puct_fused.hip) ...
PUCT_FUSED_MAX_BLOCKS = 256   # ... and its grid's cap: more tiles are walked grid-stride
SELFPLAY_MAX_PLIES = {5: 80, 7: 128}   # above the rules' bound on a game's length: 69 / 117 plies
_PLAY_ROWS = (("board", torch.int8, lambda S: (S, S)), ("dice", torch.int8, lambda S: ()), ("visits", torch.int32, lambda S: (2, 3)),
              ("value", torch.float32, lambda S: ()), ("action", torch.int8, lambda S: (2,)), ("live", torch.int8, lambda S: ()))


def _network_inputs(who, boards, dice, params, cube_layer, more=(), optional=(), table=None, table_name="endgame_table"):
    """The opening of a call on the network, up to the device check, which is the caller's _same_gpu(who, dev, "params", t.items()):
    boards [S, S] or [M, S, S], dice [M], params as predict_policy takes them; more and optional = [(name, x, dtype, shape of (M, P))],
    further inputs in the order they are checked, an optional one may be None; table: an EndgameTable for the boards' size or None
    (EndgameTable.lookup's texts), the caller's keyword table_name
    -> (M, S, cube_layer, the device of params, {name: checked tensor or None}: params, boards, dice, more, optional, "the table")"""
    M, S, P = _lookahead_shape(who, boards, cube_layer)
    if table is not None:
        _accept_table(who, table, S, "boards of shape %s, the table is for %%dx%%d" % [M, S, S], name=table_name)
    dev = _policy_params(who, params, P, S)
    t = {"params": params}
    for name, x, dtype, shape in (("boards", boards, torch.int8, lambda M, P: (M, S, S)), ("dice", dice, torch.int8, lambda M, P: (M,))) + more:
        t[name] = _policy_input(name, x, dtype, shape(M, P), dev, who=who)
    for name, x, dtype, shape in optional:
        t[name] = None if x is None else _policy_input(name, x, dtype, shape(M, P), dev, who=who)
    t["the table"] = None if table is None else table.table
    return M, S, int(cube_layer), dev, t


def _outputs(first, *asked):
    """what a call with optional outputs returns: `first` alone, or the tuple of it and those of `asked` that are not None"""
    out = (first,) + tuple(t for t in asked if t is not None)
    return out[0] if len(out) == 1 else out


def _device_of(x):
    """the device of a call without params: x's if it is a tensor, else the current GPU -- the host where there is none"""
    if isinstance(x, torch.Tensor):
        return x.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def predict_policy(boards, dice, params, deterministic=True, key=0, obs_id=None, uniforms=None, return_logits=False, return_value=False,
                   cube_layer=3):
    """The trained actor-critic's predict on M observations (ewn_predict_policy; model.predict(obs, deterministic=True) upstream):
    boards [S, S] or [M, S, S], dice [M], params the flat fp32 device vector of a2c.ActorCritic.flat_parameters() -> actions int8
    [M, 2], or the tuple (actions, logits float32 [M, 5] if return_logits, value float32 [M] if return_value).  The network is the
    rollout kernel's: a rollout_policy step replayed on its observation with its recorded noise row as `uniforms` returns the recorded
    logits, value and action bit for bit.  deterministic=False samples (Gumbel-max): from `uniforms` (float32 [M, 5] in (0, 1)) when
    given, else from a hash of (key, obs_id[m]) -- obs_id None: m.  Tensors are read in place and must be contiguous device tensors of
    the kernel's dtype (int8 observations, float32 params / uniforms, int32 or uint32 obs_id); host arrays are copied over.  Anything
    else raises ValueError before a launch."""
    who = "predict_policy"
    lib = _lib.load()
    if isinstance(obs_id, torch.Tensor) and obs_id.dtype == torch.uint32:    # read in place: unlike the older queries' host obs_id
        obs_id = obs_id.view(torch.int32)
    if obs_id is not None and not isinstance(obs_id, torch.Tensor):
        obs_id = np.asarray(obs_id).astype(np.uint32).view(np.int32)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, optional=(
        ("uniforms", uniforms, torch.float32, lambda M, P: (M, 5)), ("obs_id", obs_id, torch.int32, lambda M, P: (M,))))
    _same_gpu(who, dev, "params", t.items())
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    logits = torch.zeros((M, 5), dtype=torch.float32, device=dev) if return_logits else None
    value = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    with torch.cuda.device(dev):
        check(lib.ewn_predict_policy(S, L, M, _ptr(t["boards"]), _ptr(t["dice"]), _ptr(params), int(bool(deterministic)),
                                     C.c_uint64(int(key) & 0xFFFFFFFFFFFFFFFF), _ptr(t["obs_id"]), _ptr(t["uniforms"]), _ptr(acts),
                                     _ptr(logits), _ptr(value), _stream()), "ewn_predict_policy")
    return _outputs(acts, logits, value)


def _stage_inputs(who, named, cube_layer):
    """the inputs of a lookahead stage, checked as predict_lookahead checks its own: named = [(name, x, dtype, shape of (M, S))], boards
    first.  The device is the first tensor's (host arrays are copied there), and it must be a GPU."""
    M, S, _ = _lookahead_shape(who, named[0][1], cube_layer)
    if M * LA_ROWS > 2 ** 31 - 1:
        raise ValueError("%s: %d observations are %d leaf rows, more than 2^31 - 1: call in chunks" % (who, M, M * LA_ROWS))
    dev = _device_of(next((x for _, x, _, _ in named if isinstance(x, torch.Tensor)), None))
    out = [_policy_input(name, x, dtype, shape(M, S), dev, who=who) for name, x, dtype, shape in named]
    _same_gpu(who, dev, named[0][0], [(name, t) for (name, _, _, _), t in zip(named, out)])
    return M, S, dev, out


def lookahead_expand(boards, dice, cube_layer=3):
    """The leaves of predict_lookahead's tree as observations (ewn_lookahead_expand): boards [S, S] or [M, S, S], dice [M]
    -> (leaf_boards int8 [M, 648, S, S], leaf_dice int8 [M, 648], kind int8 [M, 108]).  Tuple t = 18 (3 f + r) + 3 (cube - 1) + direction
    is the agent's move (f, r) followed by the reply of the opponent's cube in that direction; kind[m, t] is 0 where there is no such
    reply (or the root leaves the board, wins, or repeats roots 0..2), 1 where the reply wins for the opponent, 2 for a leaf.  Row
    6 t + d2 - 1 holds the board after both moves and the dice d2 where kind is 2, a zero board and d2 elsewhere.  predict_lookahead's
    argument checks."""
    M, S, dev, (b, d) = _stage_inputs("lookahead_expand", [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                                           ("dice", dice, torch.int8, lambda M, S: (M,))], cube_layer)
    lb = torch.empty((M, LA_ROWS, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty((M, LA_ROWS), dtype=torch.int8, device=dev)
    kind = torch.empty((M, LA_TUPLES), dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_expand(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(lb), _ptr(ld), _ptr(kind), _stream()),
              "ewn_lookahead_expand")
    return lb, ld, kind


def lookahead_reduce(boards, dice, kind, leaf, terminal_value=1.0, return_q=False, cube_layer=3):
    """Leaf values folded back into Q and the action (ewn_lookahead_reduce): boards, dice as lookahead_expand took them,
    kind as it returned it, leaf float32 [M, 648] (a value per leaf row) or [M, 648, 6] (a q row per leaf row: its maximum is the
    row's value) -> actions int8 [M, 2], with return_q the float32 [M, 2, 3] Q as well.  The arithmetic is predict_lookahead's: with
    leaf = predict_policy(leaf rows, return_value=True)'s values the result is predict_lookahead's, bit for bit."""
    who = "lookahead_reduce"
    _finite(who, "terminal_value", terminal_value)
    shp = tuple(leaf.shape) if isinstance(leaf, torch.Tensor) else np.asarray(leaf).shape
    if not (len(shp) in (2, 3) and shp[1] == LA_ROWS and (len(shp) == 2 or shp[2] == 6)):
        raise ValueError("%s: leaf must have shape [M, 648] or [M, 648, 6], got %s" % (who, list(shp)))
    width = 6 if len(shp) == 3 else 1
    M, S, dev, (b, d, k, lf) = _stage_inputs(who, [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                                  ("dice", dice, torch.int8, lambda M, S: (M,)),
                                                  ("kind", kind, torch.int8, lambda M, S: (M, LA_TUPLES)),
                                                  ("leaf", leaf, torch.float32, lambda M, S: (M, LA_ROWS, width))], cube_layer)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_reduce(S, int(cube_layer), M, _ptr(b), _ptr(d), _ptr(k), _ptr(lf), width,
                                               C.c_float(float(terminal_value)), _ptr(acts), _ptr(q), _stream()), "ewn_lookahead_reduce")
    return _outputs(acts, q)


def predict_lookahead(boards, dice, params, terminal_value=1.0, return_q=False, cube_layer=3, plies=1, chunk=1024, endgame_table=None,
                      return_leaf_counts=False):
    """What the trained actor-critic plays when it looks one move ahead with its own value net (ewn_predict_lookahead):
    per observation and env action (f, r), Q = -inf for a move that leaves the board, +terminal_value for one that wins, otherwise the
    mean over the opponent's dice of its best (minimal) reply, a reply being worth -terminal_value if it wins for the opponent and
    else the mean over the agent's next dice of the value net there.  Plain expectiminimax, no pruning.  boards [S, S] or [M, S, S],
    dice [M] (outside 1..6: clamped), params as predict_policy takes them -> actions int8 [M, 2] (the first maximum of Q), and with
    return_q the float32 [M, 2, 3] Q as well.  A row that is already over, or has no agent cube, gets (0, 0) and six -inf.  The same
    argument checks as predict_policy: anything the kernel cannot read in place raises ValueError before a launch.
    plies=2 looks two moves ahead: the same tree with each leaf V(b2, d2) replaced by the maximum of the one-move Q at
    (b2, d2) -- lookahead_expand, ewn_predict_lookahead on the 648 leaf rows per observation, lookahead_reduce -- `chunk` observations
    at a time on scratch allocated once per call (about 49 KB per observation of the chunk at 7x7).
    endgame_table (an EndgameTable of the boards' size on the same GPU): a leaf b2 that the table covers is worth
    terminal_value * E(b2), exactly, instead of the critic's mean there (ewn_predict_lookahead_eg); with plies=2 the table goes to the
    inner call on the 648 leaf rows.  return_leaf_counts (plies=1 with a table): the int16 [M, 2] counts of leaf tuples valued by the
    table and by the critic are returned last."""
    lib = _lib.load()
    if plies not in (1, 2):
        raise ValueError("predict_lookahead: plies must be 1 or 2, got %r" % (plies,))
    who = "predict_lookahead"
    _at_least_one(who, "chunk", chunk)
    if return_leaf_counts and plies != 1:
        raise ValueError("predict_lookahead: return_leaf_counts is the one-move call's (plies=1), got plies=%r" % (plies,))
    if return_leaf_counts and endgame_table is None:
        raise ValueError("predict_lookahead: return_leaf_counts needs an endgame_table")
    tv = _finite(who, "terminal_value", terminal_value)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, table=endgame_table)
    _same_gpu(who, dev, "params", t.items())
    b, d, table = t["boards"], t["dice"], endgame_table
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    if plies == 2:
        return _predict_lookahead2(lib, S, L, M, b, d, params, tv, acts, q, int(chunk), table)
    if table is None:
        with torch.cuda.device(dev):
            check(lib.ewn_predict_lookahead(S, L, M, _ptr(b), _ptr(d), _ptr(params), C.c_float(tv), _ptr(acts), _ptr(q), _stream()),
                  "ewn_predict_lookahead")
        return _outputs(acts, q)
    counts = torch.zeros((M, 2), dtype=torch.int16, device=dev) if return_leaf_counts else None
    with torch.cuda.device(dev):
        check(lib.ewn_predict_lookahead_eg(S, L, M, _ptr(b), _ptr(d), _ptr(params), C.c_float(tv), table.max_cubes, table.max_total,
                                           _ptr(table.table), _ptr(acts), _ptr(q), _ptr(counts), _stream()), "ewn_predict_lookahead_eg")
    return _outputs(acts, q, counts)


def _predict_lookahead2(lib, S, L, M, b, d, params, tv, acts, q, chunk, table=None):
    """predict_lookahead(plies=2) on checked inputs: per chunk of c observations expand -> ewn_predict_lookahead with q on the 648 c
    leaf rows (ewn_predict_lookahead_eg where there is a table) -> reduce at leaf_width 6; the scratch is one allocation per call,
    every row of it rewritten per chunk"""
    dev = params.device
    c = max(1, min(chunk, M, (2 ** 31 - 1) // LA_ROWS))  # a chunk's 648 c leaf rows are counted in an int
    lb = torch.empty((c * LA_ROWS, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty(c * LA_ROWS, dtype=torch.int8, device=dev)
    kind = torch.empty((c, LA_TUPLES), dtype=torch.int8, device=dev)
    la = torch.empty((c * LA_ROWS, 2), dtype=torch.int8, device=dev)
    lq = torch.empty((c * LA_ROWS, 6), dtype=torch.float32, device=dev)
    tvf = C.c_float(tv)
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            bi, di, ai, qi = b[i:i + n], d[i:i + n], acts[i:i + n], None if q is None else q[i:i + n]
            check(lib.ewn_lookahead_expand(S, L, n, _ptr(bi), _ptr(di), _ptr(lb), _ptr(ld), _ptr(kind), st), "ewn_lookahead_expand")
            if table is None:
                check(lib.ewn_predict_lookahead(S, L, LA_ROWS * n, _ptr(lb), _ptr(ld), _ptr(params), tvf, _ptr(la), _ptr(lq), st), "ewn_predict_lookahead")
            else:
                check(lib.ewn_predict_lookahead_eg(S, L, LA_ROWS * n, _ptr(lb), _ptr(ld), _ptr(params), tvf, table.max_cubes, table.max_total,
                                                   _ptr(table.table), _ptr(la), _ptr(lq), None, st), "ewn_predict_lookahead_eg")
            check(lib.ewn_lookahead_reduce(S, L, n, _ptr(bi), _ptr(di), _ptr(kind), _ptr(lq), 6, tvf, _ptr(ai), _ptr(qi), st),
                  "ewn_lookahead_reduce")
    return _outputs(acts, q)


def lookahead_targets(q, temperature=0.0):
    """predict_lookahead's Q as training targets (ewn_lookahead_targets): q float32 [M, 2, 3] or [M, 6] on the GPU ->
    (target_pi float32 [M, 5], target_value float32 [M], weight float32 [M]).  A row of six -inf (a finished observation) gets zeros
    and weight 0; any other row weight 1 and its maximum as the value.  temperature 0: the search's action one-hot on both heads
    ((0.5, 0.5) on the flag head when both flags move the same cube); temperature > 0: the softmax of q / temperature over the
    moves that stay on the board, summed per head."""
    who = "lookahead_targets"
    t = _not_negative(who, "temperature", temperature)
    shp = tuple(q.shape) if isinstance(q, torch.Tensor) else np.asarray(q).shape
    if not (len(shp) in (2, 3) and math.prod(shp[1:]) == 6 and (len(shp) == 2 or shp[1:] == (2, 3))):
        raise ValueError("%s: q must have shape [M, 2, 3] or [M, 6], got %s" % (who, list(shp)))
    M = int(shp[0])
    dev = _device_of(q)
    qq = _policy_input("q", q, torch.float32, (M, 6), dev, who=who)
    if not qq.is_cuda:
        raise ValueError("%s: q must live on the GPU, got %s" % (who, _describe(qq)))
    pi = torch.zeros((M, 5), dtype=torch.float32, device=dev)
    val = torch.zeros(M, dtype=torch.float32, device=dev)
    w = torch.zeros(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_lookahead_targets(M, _ptr(qq), C.c_float(t), _ptr(pi), _ptr(val), _ptr(w), _stream()), "ewn_lookahead_targets")
    return pi, val, w


def sup_grad(boards, dice, target_pi, target_value, params, weight=None, pi_coef=1.0, vf_coef=0.5, cube_layer=3, out=None, scratch=None):
    """The gradient of a supervised loss on M given observations (ewn_sup_grad):
        loss = mean_m w_m (pi_coef * CE(target_pi[m], policy heads) + vf_coef * (V - target_value[m])^2)
    boards [S, S] or [M, S, S], dice [M], target_pi float32 [M, 5] (entries 0-1 the flag head, 2-4 the direction head; a head whose
    entries are all zero is masked), target_value [M], weight [M] or None (ones), params as predict_policy takes them -> float32
    [P + 8]: the gradient in the params layout, then the sums over the samples with weight > 0 of {w CE, w entropy, agreement
    count, w, w (V - v*)^2, 0, 0, 0}.  A row whose weight is 0 is skipped altogether (its targets may be NaN or infinite).  out: a
    float32 [P + 8] device tensor to write into; scratch: a 4-byte aligned uint8 device tensor of at least ewn_sup_scratch_bytes.  predict_policy's
    argument checks: anything the kernels cannot read in place raises ValueError before a launch.  The step is ewn_a2c_apply."""
    who = "sup_grad"
    lib = _lib.load()
    pi_coef, vf_coef = _not_negative(who, "pi_coef", pi_coef), _not_negative(who, "vf_coef", vf_coef)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, (
        ("target_pi", target_pi, torch.float32, lambda M, P: (M, 5)), ("target_value", target_value, torch.float32, lambda M, P: (M,))), (
        ("weight", weight, torch.float32, lambda M, P: (M,)), ("out", out, torch.float32, lambda M, P: (P + 8,))))
    if M < 1:
        raise ValueError("%s: needs at least one observation (a mean over nothing is undefined)" % who)
    nscr = int(lib.ewn_sup_scratch_bytes(S, L, M))
    if scratch is not None and not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.uint8 and scratch.is_contiguous()
                                    and scratch.numel() >= nscr and scratch.data_ptr() % 4 == 0):
        raise ValueError("%s: scratch must be a contiguous, 4-byte aligned uint8 tensor of at least %d elements, got %s%s" % (
            who, nscr, _describe(scratch), " at an address that is %d past a multiple of 4" % (scratch.data_ptr() % 4)
            if isinstance(scratch, torch.Tensor) and scratch.data_ptr() % 4 else ""))
    _same_gpu(who, dev, "params", list(t.items()) + [("scratch", scratch)])
    grad = out if out is not None else torch.zeros(params.numel() + 8, dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.zeros(nscr, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.ewn_sup_grad(S, L, M, _ptr(t["boards"]), _ptr(t["dice"]), _ptr(t["target_pi"]), _ptr(t["target_value"]), _ptr(t["weight"]),
                               _ptr(params), C.c_float(pi_coef), C.c_float(vf_coef), _ptr(grad), _ptr(scratch), _stream()), "ewn_sup_grad")
    return grad


def _puct_sections(S, sims):
    """a PUCT tree's sections: ({name: (byte offset, dtype, shape per tree)}, bytes of one tree)"""
    N = sims + 1
    secs, o = {}, 0
    for name, dt, shape in (("hdr", torch.int32, (8,)), ("n", torch.int32, (N, 6)), ("w", torch.float32, (N, 6)),
                            ("p", torch.float32, (N, 6)), ("child", torch.int16, (N, 6, 6)), ("cn", torch.int16, (N, 6, 6)),
                            ("parent", torch.int16, (N, 4)), ("kind", torch.int8, (N, 6)), ("dice", torch.int8, (N,)),
                            ("board", torch.int8, (N, S, S))):
        secs[name] = (o, dt, shape)
        o += (math.prod(shape) * dt.itemsize + 3) // 4 * 4
    return secs, o


def _puct_numbers(who, sims, c_puct=0.0, terminal_value=1.0):
    if not (isinstance(sims, (int, np.integer)) and 0 <= int(sims) <= PUCT_MAX_SIMS):
        raise ValueError("%s: sims must be an integer in 0..%d, got %r" % (who, PUCT_MAX_SIMS, sims))
    _not_negative(who, "c_puct", c_puct)
    _positive(who, "terminal_value", terminal_value)
    return int(sims)


def _tree_rows(who, tree, nb, S, sims, laid_out, layout):
    """M of a tree buffer, a uint8 tensor [M, nb] that laid_out() accepts: the kernels read a contiguous, aligned one, the views any
    whose rows are; `layout`: the error's words for it"""
    if not (isinstance(tree, torch.Tensor) and tree.dtype == torch.uint8 and tree.dim() == 2 and tree.shape[1] == nb and laid_out(tree)):
        raise ValueError("%s: tree must be a %suint8 tensor [M, %d] (puct_begin's, for sims=%d on %dx%d), got %s" % (
            who, layout, nb, sims, S, S, _describe(tree)))
    return int(tree.shape[0])


def _puct_tree(who, tree, S, sims, cube_layer=3):
    """the checked tree buffer: a contiguous uint8 device tensor [M, tree_bytes] at a 4-byte aligned address -> (M, tree_bytes)"""
    nb = int(_lib.load().ewn_puct_tree_bytes(int(S), int(cube_layer), sims))
    if nb < 0:
        raise ValueError("%s: no policy network for %dx%d boards with cube_layer %d (served: cube_layer 3 on 5x5 and 7x7)" % (
            who, S, S, cube_layer))
    return _tree_rows(who, tree, nb, S, sims, lambda t: t.is_contiguous() and t.data_ptr() % 4 == 0, "contiguous, 4-byte aligned "), nb


def _holds_trees(who, name, tree, Mt, M, dev):
    if Mt != M or not (tree.is_cuda and tree.device == dev):
        raise ValueError("%s: %s must hold %d trees on %s, got %s" % (who, name, M, dev, _describe(tree)))


def _tree_device(who, tree):
    if not tree.is_cuda:
        raise ValueError("%s: tree must live on the GPU, got %s" % (who, _describe(tree)))
    return tree.device


def puct_tree_views(tree, board_size, sims):
    """Tensor views onto the sections of puct_begin's trees (uint8 [M, tree_bytes]; layout PUCT_LAYOUT), nothing is
    copied: count, done, pending, degenerate int32 [M]; n int32, w, p float32 [M, sims + 1, 6] per node and edge a = 3 f + r;
    child, cn int16 [M, sims + 1, 6, 6] per node, edge and dice d' - 1; parent int16 [M, sims + 1, 4] (node, edge, dice, 0; the
    root: -1, 0, 0, 0); kind int8 [M, sims + 1, 6]; dice int8 [M, sims + 1]; board int8 [M, sims + 1, S, S].  Rows of nodes
    count .. sims are as puct_begin left them: zeros, child -1."""
    sims = _puct_numbers("puct_tree_views", sims)
    S = int(board_size)
    secs, nb = _puct_sections(S, sims)
    _tree_rows("puct_tree_views", tree, nb, S, sims,
               lambda t: t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.storage_offset() % 4 == 0, "")
    out = {}
    for name, (o, dt, shape) in secs.items():
        out[name] = tree[:, o:o + math.prod(shape) * dt.itemsize].view(dt).unflatten(1, shape)
    hdr = out.pop("hdr")
    out.update(count=hdr[:, 0], done=hdr[:, 1], pending=hdr[:, 2], degenerate=hdr[:, 3])
    return out


def puct_begin(boards, dice, sims, cube_layer=3):
    """The trees of a PUCT search on M observations (ewn_puct_begin): boards [S, S] or [M, S, S], dice [M] (outside
    1..6: clamped) -> (tree uint8 [M, tree_bytes], leaf_boards int8 [M, S, S], leaf_dice int8 [M]).  Every byte of the trees is
    written; the root is the pending leaf and the leaf row its observation, except where the observation is already over or a side
    has no cube: that tree is degenerate and its leaf row a zero board with dice 1.  predict_lookahead's argument checks."""
    who = "puct_begin"
    sims = _puct_numbers(who, sims)
    M, S, dev, (b, d) = _stage_inputs(who, [("boards", boards, torch.int8, lambda M, S: (M, S, S)),
                                            ("dice", dice, torch.int8, lambda M, S: (M,))], cube_layer)
    lib = _lib.load()
    nb = int(lib.ewn_puct_tree_bytes(S, int(cube_layer), sims))
    tree = torch.empty((M, nb), dtype=torch.uint8, device=dev)
    lb = torch.empty((M, S, S), dtype=torch.int8, device=dev)
    ld = torch.empty(M, dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(lib.ewn_puct_begin(S, int(cube_layer), M, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), _stream()), "ewn_puct_begin")
    return tree, lb, ld


def _noise_eps(who, noise_eps):
    if not (math.isfinite(float(noise_eps)) and 0.0 <= float(noise_eps) <= 1.0):
        raise ValueError("%s: noise_eps must be a finite number in [0, 1], got %r" % (who, noise_eps))
    return float(noise_eps)


def puct_advance(tree, logits, value, leaf_boards, leaf_dice, sims, c_puct=1.5, terminal_value=1.0, board_size=None, cube_layer=3,
                 root_noise=None, noise_eps=0.25):
    """One round of the search (ewn_puct_advance): logits float32 [M, 5] and value float32 [M] are predict_policy's on
    the leaf rows.  Per tree the pending leaf is evaluated (priors from the logits, v = value / terminal_value clamped to [-1, 1])
    and backed up; then, while fewer than `sims` simulations have begun, one more walks down to a new leaf, or ends at once on a
    winning move.  tree, leaf_boards and leaf_dice are updated in place (a tree without a pending leaf: a zero board with dice 1) and
    returned.  board_size: taken from leaf_boards [M, S, S] when None.  sims + 1 rounds after puct_begin complete the search.
    root_noise (float32 [M, 2, 3] or [M, 6], un-normalised weights, e.g. Gamma variates): ewn_puct_advance_noise
    instead -- where the leaf evaluated is the root, its priors become (1 - noise_eps) P + noise_eps eta / sum(eta) over the legal
    edges with a finite positive weight.  None: exactly the plain call, noise_eps is not looked at."""
    who = "puct_advance"
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = None if root_noise is None else _noise_eps(who, noise_eps)
    for name, t in (("tree", tree), ("leaf_boards", leaf_boards), ("leaf_dice", leaf_dice)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s is updated in place and must be a tensor, got %s" % (who, name, _describe(t)))
    if board_size is not None and not (leaf_boards.dim() == 3 and leaf_boards.shape[1] == int(board_size)):
        raise ValueError("%s: leaf_boards must have shape [M, %d, %d], got %s" % (who, int(board_size), int(board_size), list(leaf_boards.shape)))
    M, S, dev, (lb, lg, v, ld) = _stage_inputs(who, [("leaf_boards", leaf_boards, torch.int8, lambda M, S: (M, S, S)),
                                                    ("logits", logits, torch.float32, lambda M, S: (M, 5)),
                                                    ("value", value, torch.float32, lambda M, S: (M,)),
                                                    ("leaf_dice", leaf_dice, torch.int8, lambda M, S: (M,))], cube_layer)
    _holds_trees(who, "tree", tree, _puct_tree(who, tree, S, sims, cube_layer)[0], M, dev)
    lib = _lib.load()
    fn, noise, name = lib.ewn_puct_advance, (), "ewn_puct_advance"
    if root_noise is not None:                                 # the noise instance: the same call with two more arguments
        rn = _policy_input("root_noise", root_noise, torch.float32, (M, 6), dev, who=who)
        _same_gpu(who, dev, "leaf_boards", (("root_noise", rn),))
        fn, noise, name = lib.ewn_puct_advance_noise, (_ptr(rn), C.c_float(eps)), "ewn_puct_advance_noise"
    with torch.cuda.device(dev):
        check(fn(S, int(cube_layer), M, sims, C.c_float(float(c_puct)), C.c_float(float(terminal_value)), _ptr(tree), _ptr(lg), _ptr(v),
                 *noise, _ptr(lb), _ptr(ld), _stream()), name)
    return tree, leaf_boards, leaf_dice


def puct_result(tree, board_size, sims, return_visits=False, return_q=False, return_value=False, cube_layer=3):
    """What the search found at the roots (ewn_puct_result) -> actions int8 [M, 2], or the tuple (actions, visits int32
    [M, 2, 3] if return_visits, q float32 [M, 2, 3] if return_q, value float32 [M] if return_value).  The action is the first root
    move that wins if there is one, else the first maximum of the visits over the searched moves; q is -inf where (f, r) is no
    action, +1 where it wins, else W / N (0 unvisited), value sum W / sum N, both in units of the terminal value.  A degenerate row:
    (0, 0), zero visits, six -inf, 0."""
    who = "puct_result"
    sims = _puct_numbers(who, sims)
    S = int(board_size)
    M, _ = _puct_tree(who, tree, S, sims, cube_layer)
    dev = _tree_device(who, tree)
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    with torch.cuda.device(dev):
        check(_lib.load().ewn_puct_result(S, int(cube_layer), M, _ptr(tree), _ptr(acts), _ptr(visits), _ptr(q), _ptr(val), _stream()),
              "ewn_puct_result")
    return _outputs(acts, visits, q, val)


def _fused_table(who, fused, endgame_table):
    if fused and endgame_table is not None:
        raise ValueError("%s: fused=True does not take an endgame_table: the exact-leaf substitution is the staged path's (fused=False)" % who)


def _leaf_table_alone(who, leaf_table, endgame_table=None, leaves=1, whole_games=False):
    """the users' keyword: leaf_table is the one launch of ewn_puct_search_eg, which is neither the staged path's
    substitution, nor the wide launch, nor whole games -> whether there is one"""
    if leaf_table is None:
        return False
    if endgame_table is not None:
        raise ValueError("%s: leaf_table does not go with endgame_table: both put exact values at the covered leaves, leaf_table in one "
                         "launch (ewn_puct_search_eg), endgame_table on the staged path" % who)
    if leaves > 1:
        raise ValueError("%s: leaf_table does not go with leaves=%d: ewn_puct_search_wide takes no table (leaves=1)" % (who, leaves))
    if whole_games:
        raise ValueError("%s: leaf_table does not go with whole_games=True: ewn_puct_selfplay takes no table" % who)
    return True


def _puct_scratch(c, nb, S, dev, fused):
    """a search's scratch for c observations: (tree, leaf boards, leaf dice, leaf actions, logits, value); fused: the tree alone"""
    tree = torch.empty((c, nb), dtype=torch.uint8, device=dev)
    if fused:
        return (tree, None, None, None, None, None)
    return (tree, torch.empty((c, S, S), dtype=torch.int8, device=dev), torch.empty(c, dtype=torch.int8, device=dev),
            torch.empty((c, 2), dtype=torch.int8, device=dev), torch.empty((c, 5), dtype=torch.float32, device=dev),
            torch.empty(c, dtype=torch.float32, device=dev))


def _search_setup(lib, S, L, M, sims, chunk, c_puct, terminal_value, dev, fused, leaves=1):
    """what predict_puct and selfplay_puct search M observations on: (the observations of a chunk, its _puct_scratch, allocated once per
    call, c_puct and terminal_value as the kernels take them).  leaves > 1 (the wide launch): the tree alone, and the
    launch's marks behind it"""
    c = max(1, min(int(chunk), M))
    nb = int(lib.ewn_puct_tree_bytes(S, L, sims))
    scratch = _puct_scratch(c, nb, S, dev, fused or leaves > 1)
    if leaves > 1:
        from .wide import _wide_scratch
        scratch += (_wide_scratch(lib, S, L, c, sims, dev),)
    return c, scratch, C.c_float(float(c_puct)), C.c_float(float(terminal_value))


def puct_search(boards, dice, params, sims, c_puct=1.5, terminal_value=1.0, root_noise=None, noise_eps=0.25, rounds=None, cube_layer=3,
                out=None):
    """The whole PUCT search of M observations in one launch (ewn_puct_search) -> tree uint8 [M, tree_bytes]: byte for
    byte what puct_begin and then `rounds` rounds of predict_policy on the leaf rows and puct_advance leave (the first round with
    root_noise and noise_eps when root_noise is given: float32 [M, 2, 3] or [M, 6], puct_advance's).  rounds None: all sims + 1;
    an integer: min(rounds, sims + 1), 0 is puct_begin alone.  puct_result, puct_play and puct_tree_views read the tree.  out: a
    contiguous, 4-byte aligned uint8 tensor [M, tree_bytes] to write into (what it held does not matter).  predict_puct's argument
    checks."""
    who = "puct_search"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    eps = 0.0 if root_noise is None else _noise_eps(who, noise_eps)
    rounds = _rounds(who, rounds, sims)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, optional=(
        ("root_noise", root_noise, torch.float32, lambda M, P: (M, 6)),))
    _same_gpu(who, dev, "params", t.items())
    out = _search_out(who, lib, out, M, S, L, sims, dev)
    with torch.cuda.device(dev):
        check(lib.ewn_puct_search(S, L, M, sims, rounds, C.c_float(float(c_puct)),
                                  C.c_float(float(terminal_value)), _ptr(t["boards"]), _ptr(t["dice"]), _ptr(params), _ptr(t["root_noise"]),
                                  C.c_float(eps), _ptr(out), _stream()), "ewn_puct_search")
    return out


def _rounds(who, rounds, sims):
    """rounds= of a whole search as the entries take it: -1 for all sims + 1"""
    if rounds is not None and not (isinstance(rounds, (int, np.integer)) and int(rounds) >= 0):
        raise ValueError("%s: rounds must be None or an integer that is not negative, got %r" % (who, rounds))
    return -1 if rounds is None else min(int(rounds), sims + 1)


def _search_out(who, lib, out, M, S, L, sims, dev):
    """out= of a whole search: None -> new trees; else the checked contiguous, 4-byte aligned uint8 tensor [M, tree_bytes] on dev"""
    if out is None:
        return torch.empty((M, int(lib.ewn_puct_tree_bytes(S, L, sims))), dtype=torch.uint8, device=dev)
    _holds_trees(who, "out", out, _puct_tree(who, out, S, sims, L)[0], M, dev)
    return out


def _puct_search(lib, S, L, n, sims, b, d, params, cp, tv, table, scratch, st, noise=None, eps=0.0, fused=False, leaves=1, exact=False):
    """predict_puct's and selfplay_puct's search of n observations on the caller's scratch: begin, then sims + 1 rounds of
    ewn_predict_policy and advance.  noise (float32 [n, 6]): the first round, which evaluates the roots, is the noise instance's.
    fused: the one launch of ewn_puct_search instead -- the same bytes in the tree; of the scratch only the tree is used.
    leaves > 1: the one launch of ewn_puct_search_wide, whatever fused says -- another tree, in fewer rounds.
    exact: `table` goes to the one launch of ewn_puct_search_eg, whatever fused says -- the staged search with the
    table, but for the sign of a zero"""
    tree, lb, ld, la, lg, lv = scratch[:6]
    if exact:
        from .puct_exact import _launch
        _launch(lib, S, L, n, sims, -1, cp, tv, b, d, params, noise, eps, 0, 0, table, tree, None, st)
        return
    if leaves > 1:
        from .wide import _launch
        _launch(lib, S, L, n, sims, leaves, cp, tv, b, d, params, noise, eps, 0, 0, tree, scratch[6], st)
        return
    if fused:
        check(lib.ewn_puct_search(S, L, n, sims, -1, cp, tv, _ptr(b), _ptr(d), _ptr(params), _ptr(noise), C.c_float(eps), _ptr(tree), st),
              "ewn_puct_search")
        return
    check(lib.ewn_puct_begin(S, L, n, sims, _ptr(b), _ptr(d), _ptr(tree), _ptr(lb), _ptr(ld), st), "ewn_puct_begin")
    for rnd in range(sims + 1):
        check(lib.ewn_predict_policy(S, L, n, _ptr(lb), _ptr(ld), _ptr(params), 1, C.c_uint64(0), None, None, _ptr(la), _ptr(lg),
                                     _ptr(lv), st), "ewn_predict_policy")
        if table is not None:                                  # a tree without a pending leaf shows a zero board: not covered
            _, covered, q_exact = table.lookup(lb[:n], ld[:n], return_q=True)
            lv[:n] = torch.where(covered, tv.value * q_exact.reshape(n, 6).max(1).values, lv[:n])
        if rnd == 0 and noise is not None:
            check(lib.ewn_puct_advance_noise(S, L, n, sims, cp, tv, _ptr(tree), _ptr(lg), _ptr(lv), _ptr(noise), C.c_float(eps), _ptr(lb),
                                             _ptr(ld), st), "ewn_puct_advance_noise")
        else:
            check(lib.ewn_puct_advance(S, L, n, sims, cp, tv, _ptr(tree), _ptr(lg), _ptr(lv), _ptr(lb), _ptr(ld), st), "ewn_puct_advance")


def predict_puct(boards, dice, params, sims=64, c_puct=1.5, terminal_value=1.0, return_visits=False, return_q=False, return_value=False,
                 cube_layer=3, chunk=1024, endgame_table=None, fused=False, leaves=1, leaf_table=None):
    """What the trained actor-critic plays after a PUCT search of `sims` simulations on its own two heads: the policy
    head says where to look, the value head what a leaf is worth, a move that wins on the board is worth +1 and is played; the
    opponent's and the agent's later dice are chance nodes sampled in a fixed stratified order, so the search is deterministic.
    boards [S, S] or [M, S, S], dice [M] (outside 1..6: clamped), params as predict_policy takes them -> actions int8 [M, 2], or the
    tuple (actions, visits int32 [M, 2, 3], q float32 [M, 2, 3], value float32 [M]) of what was asked for, as puct_result returns
    them.  sims=0: no search, zero visits, the first legal move unless one wins.  The stages are puct_begin, then sims + 1 rounds of
    ewn_predict_policy on the leaf rows and puct_advance, then puct_result, `chunk` observations at a time on scratch allocated once
    per call (a tree is 256 bytes per simulation at 5x5, 280 at 7x7).  predict_lookahead's argument checks.
    endgame_table (an EndgameTable of the boards' size on the same GPU): a pending leaf that the table covers is worth
    terminal_value * max_a q_exact(leaf board, leaf dice) instead of the value head's output; the logits are the policy head's.
    fused=True: each chunk's search is the one launch of ewn_puct_search -- the same trees byte for byte, so the same
    results bit for bit, and no leaf-row scratch; not together with endgame_table (the exact leaves stay on the staged path).
    leaves: 1 is all of the above; 2..32: each chunk's search is the one launch of ewn_puct_search_wide, which collects
    up to that many leaves per tree and round under a virtual loss -- about sims / leaves rounds, another tree and so other
    results than leaves=1, whatever fused says; not together with endgame_table.
    leaf_table (an EndgameTable of the boards' size on the same GPU): endgame_table's exact leaves with each chunk's
    search in the one launch of ewn_puct_search_eg and no leaf-row scratch -- the staged search's results in every value (a zero may
    differ in its sign); fused is not read; not together with endgame_table or leaves > 1."""
    who = "predict_puct"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    _fused_table(who, fused, endgame_table)
    from .wide import _NO_TABLE, _leaves_alone
    leaves = _leaves_alone(who, leaves, endgame_table=(endgame_table is not None, _NO_TABLE))
    exact = _leaf_table_alone(who, leaf_table, endgame_table, leaves)
    _at_least_one(who, "chunk", chunk)
    M, S, L, dev, t = _network_inputs(who, boards, dice, params, cube_layer, table=leaf_table if exact else endgame_table,
                                      table_name="leaf_table" if exact else "endgame_table")
    _same_gpu(who, dev, "params", t.items())
    b, d = t["boards"], t["dice"]
    acts = torch.zeros((M, 2), dtype=torch.int8, device=dev)
    visits = torch.zeros((M, 2, 3), dtype=torch.int32, device=dev) if return_visits else None
    q = torch.zeros((M, 2, 3), dtype=torch.float32, device=dev) if return_q else None
    val = torch.zeros(M, dtype=torch.float32, device=dev) if return_value else None
    c, scratch, cp, tv = _search_setup(lib, S, L, M, sims, chunk, c_puct, terminal_value, dev, fused or exact, leaves)
    tree = scratch[0]
    with torch.cuda.device(dev):
        st = _stream()
        for i in range(0, M, c):
            n = min(c, M - i)
            sl = slice(i, i + n)
            _puct_search(lib, S, L, n, sims, b[sl], d[sl], params, cp, tv, leaf_table if exact else endgame_table, scratch, st, fused=fused,
                         leaves=leaves, exact=exact)
            check(lib.ewn_puct_result(S, L, n, _ptr(tree), _ptr(acts[sl]), _ptr(None if visits is None else visits[sl]),
                                      _ptr(None if q is None else q[sl]), _ptr(None if val is None else val[sl]), st), "ewn_puct_result")
    return _outputs(acts, visits, q, val)


def _play_numbers(who, temp_plies, key, game_offset):
    if not (isinstance(temp_plies, (int, np.integer)) and 0 <= int(temp_plies) <= 2 ** 31 - 1):
        raise ValueError("%s: temp_plies must be an integer that is not negative, got %r" % (who, temp_plies))
    if not (isinstance(key, (int, np.integer)) and isinstance(game_offset, (int, np.integer)) and -2 ** 63 <= int(game_offset) < 2 ** 63):
        raise ValueError("%s: key and game_offset must be integers, game_offset within 64 bits, got %r and %r" % (who, key, game_offset))
    return int(temp_plies), int(key) & 0xFFFFFFFFFFFFFFFF, int(game_offset)


def puct_play(tree, boards, dice, game, board_size, sims, temp_plies=0, key=0, game_offset=0, out=None, cube_layer=3):
    """One ply of M self-play games off their searched trees (ewn_puct_play; puct_result's checks of the tree).  boards
    int8 [M, S, S], dice int8 [M] and game int32 [M, 4] = (ply, over, winner, 0) are updated in place: the move is the first root
    move that wins, else drawn in proportion to the root's visits while ply < temp_plies (a Philox word of key, game_offset + m and
    ply), else the first maximum of the visits; the next dice is a second word of the same block.  The position played and recorded
    is the tree's root.  A game that is over, or whose tree is degenerate, is left as it is (the latter is then over, without a
    winner).  out: None -> a new record row {board int8 [M, S, S], dice int8 [M], visits int32 [M, 2, 3], value float32 [M], action
    int8 [M, 2], live int8 [M]} is returned; a dict -> the tensors it holds under those names are written (a missing name or None:
    not written) and it is returned."""
    who = "puct_play"
    sims = _puct_numbers(who, sims)
    temp_plies, key, game_offset = _play_numbers(who, temp_plies, key, game_offset)
    S = int(board_size)
    M, _ = _puct_tree(who, tree, S, sims, cube_layer)
    for name, t, dtype, shape in (("boards", boards, torch.int8, (M, S, S)), ("dice", dice, torch.int8, (M,)), ("game", game, torch.int32, (M, 4))):
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("%s: %s is updated in place and must be a contiguous %s tensor of shape %s, got %s" % (
                who, name, str(dtype).replace("torch.", ""), list(shape), _describe(t)))
    if out is not None and (not isinstance(out, dict) or set(out) - {name for name, _, _ in _PLAY_ROWS}):
        raise ValueError("%s: out must be a dict with keys among board, dice, visits, value, action, live, got %r" % (
            who, sorted(out) if isinstance(out, dict) else type(out).__name__))
    dev = _tree_device(who, tree)
    _same_gpu(who, dev, "tree", (("boards", boards), ("dice", dice), ("game", game)))
    if out is None:
        out = {name: torch.zeros((M,) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}
    rows = []
    for name, dt, shape in _PLAY_ROWS:
        t = out.get(name)
        if t is not None:
            if isinstance(t, torch.Tensor) and t.dtype == torch.bool and dt == torch.int8:
                t = t.view(torch.int8)
            if not (_is_buffer(t, dt) and t.numel() == M * math.prod(shape(S))):
                raise ValueError("%s: out[%r] must be a contiguous %s device tensor of %s elements, got %s" % (
                    who, name, str(dt).replace("torch.", ""), " x ".join(map(str, (M,) + shape(S))), _describe(t)))
            _same_gpu(who, dev, "tree", ((("out[%r]" % name), t),))
        rows.append(t)
    with torch.cuda.device(dev):
        check(_lib.load().ewn_puct_play(S, int(cube_layer), M, _ptr(tree), _ptr(boards), _ptr(dice), _ptr(game), temp_plies, C.c_uint64(key),
                                        C.c_int64(game_offset), *[_ptr(t) for t in rows], _stream()), "ewn_puct_play")
    return out


def selfplay_outcomes(winner, live):
    """The value targets of self-play records whose games all start at ply 0 in row 0 (plain torch): winner [M] (0 none, +1 the side
    that moves at even plies, -1 the other), live bool [T, M] -> (z float32 [T, M], weight float32 [T, M]).  z[t, m] is the result
    seen from the side to move in row t: winner[m] at even t, -winner[m] at odd t, on live rows; weight is 1 on the live rows of
    finished games.  Everything else is 0."""
    live = live.to(torch.bool)
    w = winner.to(torch.float32)[None, :]
    sign = 1.0 - 2.0 * (torch.arange(live.shape[0], device=live.device) % 2).to(torch.float32)
    counts = live & (w != 0)
    z = torch.where(counts, w * sign[:, None], torch.zeros((), device=live.device))
    return z.contiguous(), counts.to(torch.float32).contiguous()


def _game_column(game, i):
    """column i of game [M, 4] as a dense tensor of its own: stride 1 at M == 1 too, where .contiguous() hands the strided view back"""
    return torch.empty(game.shape[0], dtype=game.dtype, device=game.device).copy_(game[:, i])


NOISE_BLOCK = 16384     # selfplay_noise draws whole blocks of this many consecutive global games


def selfplay_noise(M, noise_alpha, key, game_offset, ply, device="cuda"):
    """selfplay_puct's root noise of one ply: float32 [M, 6] Gamma(noise_alpha) variates (torch._standard_gamma), row m for the global
    game g = game_offset + m.  A row depends on key, the ply and g alone: the games are cut into blocks of NOISE_BLOCK consecutive
    global ids, block j is one [NOISE_BLOCK, 6] draw on a generator seeded from key, j and the ply, and the call returns its rows of
    the blocks it touches -- so the shards of a run (game_offset + the shard's first lane) get the rows the whole run gets.
    Normalised over the legal edges by the kernel they are Dirichlet(noise_alpha) noise."""
    M, first = int(M), int(game_offset)
    rows = []
    for j in range(first // NOISE_BLOCK, (first + max(M, 1) - 1) // NOISE_BLOCK + 1):
        gen = torch.Generator(device=device)
        gen.manual_seed((int(key) * 0x9E3779B97F4A7C15 + j * 0xD1B54A32D192ED03 + int(ply) * 0x2545F4914F6CDD1D) & (2 ** 63 - 1))
        block = torch._standard_gamma(torch.full((NOISE_BLOCK, 6), float(noise_alpha), dtype=torch.float32, device=device), generator=gen)
        lo, hi = max(first, j * NOISE_BLOCK), min(first + M, (j + 1) * NOISE_BLOCK)
        rows.append(block[lo - j * NOISE_BLOCK:hi - j * NOISE_BLOCK])
    return rows[0].contiguous() if len(rows) == 1 else torch.cat(rows)


def selfplay_puct(boards, dice, params, sims=64, max_plies=None, c_puct=1.5, terminal_value=1.0, noise_eps=0.25, noise_alpha=1.0,
                  temp_plies=8, key=0, game_offset=0, chunk=1024, check_every=8, endgame_table=None, cube_layer=3, fused=False,
                  leaves=1, leaf_table=None):
    """M games of the PUCT search against itself, from the given positions to the end: per ply puct_begin, sims + 1
    rounds of ewn_predict_policy and advance -- the first with Dirichlet(noise_alpha) noise of weight noise_eps on the root's priors
    (ewn_puct_advance_noise) -- then ewn_puct_play into row t: the move is drawn in proportion to the visits for the first
    temp_plies plies of a game and is the most visited one after that.  boards [S, S] or [M, S, S], dice [M], params as
    predict_policy takes them; they are not changed.  `chunk` games are played at a time, each chunk to its end; every check_every
    plies one host read ends a chunk whose games are all over.  max_plies None: 80 on 5x5, 128 on 7x7 -- a move lowers the mover's
    summed distance to its corner by at least one, so a game lasts at most 69 / 117 plies.  noise_alpha = 1.0 is a choice (about 10
    over the number of moves, AlphaZero's rule of thumb), not a measurement.  endgame_table: predict_puct's, at the leaves.
    fused=True: a ply's search is the one launch of ewn_puct_search, the records are the same bit for bit; not
    together with endgame_table.  leaves: 1 is all of the above; 2..32: a ply's search is the one launch of
    ewn_puct_search_wide with that ply's noise rows -- other trees, so other games; not together with endgame_table.
    leaf_table: predict_puct's -- endgame_table's exact leaves with a ply's search in the one launch of
    ewn_puct_search_eg; fused is not read; not together with endgame_table or leaves > 1.
    The noise is selfplay_noise: torch._standard_gamma keyed by key, the ply and the global game game_offset + m, drawn once per ply
    for all M games and read by each chunk's rows: a call repeats itself bit for bit, whatever the chunk, and the calls on the shards
    of M games (game_offset moved to each shard's first game) give the rows of the one call on all of them.  Returns a dict: board int8 [T, M, S, S], dice int8
    [T, M], visits int32 [T, M, 2, 3], value float32 [T, M], action int8 [T, M, 2], live bool [T, M] (T = max_plies; rows past a
    game's end are zero), z and weight float32 [T, M] (selfplay_outcomes), winner int32 [M], plies int32 [M]."""
    who = "selfplay_puct"
    lib = _lib.load()
    sims = _puct_numbers(who, sims, c_puct, terminal_value)
    _fused_table(who, fused, endgame_table)
    from .wide import _NO_TABLE, _leaves_alone
    leaves = _leaves_alone(who, leaves, endgame_table=(endgame_table is not None, _NO_TABLE))
    exact = _leaf_table_alone(who, leaf_table, endgame_table, leaves)
    eps = _noise_eps(who, noise_eps)
    temp_plies, key, game_offset = _play_numbers(who, temp_plies, key, game_offset)
    _positive(who, "noise_alpha", noise_alpha)
    if int(chunk) < 1 or int(check_every) < 1:
        raise ValueError("%s: chunk and check_every must be at least 1, got %r and %r" % (who, chunk, check_every))
    M, S, L, dev, inputs = _network_inputs(who, boards, dice, params, cube_layer, table=leaf_table if exact else endgame_table,
                                           table_name="leaf_table" if exact else "endgame_table")
    T = SELFPLAY_MAX_PLIES[S] if max_plies is None else max_plies
    if not (isinstance(T, (int, np.integer)) and int(T) >= 1):
        raise ValueError("%s: max_plies must be a positive integer or None, got %r" % (who, max_plies))
    T = int(T)
    _same_gpu(who, dev, "params", inputs.items())
    b, d, table = inputs["boards"], inputs["dice"], leaf_table if exact else endgame_table
    rec = {name: torch.zeros((T, M) + shape(S), dtype=dt, device=dev) for name, dt, shape in _PLAY_ROWS}
    game = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    c, scratch, cp, tv = _search_setup(lib, S, L, M, sims, chunk, c_puct, terminal_value, dev, fused or exact, leaves)
    with torch.cuda.device(dev):
        st = _stream()
        drawn = []
        for i in range(0, M, c):
            n = min(c, M - i)
            cb, cd, cg = b[i:i + n].clone(), d[i:i + n].clone(), game[i:i + n]
            for t in range(T):
                noise = None
                if eps > 0.0:
                    if t == len(drawn):                        # a ply's noise is drawn once, for all M games: later chunks read their rows
                        drawn.append(selfplay_noise(M, noise_alpha, key, game_offset, t, dev))
                    noise = drawn[t][i:i + n]
                _puct_search(lib, S, L, n, sims, cb, cd, params, cp, tv, table, scratch, st, noise, eps, fused, leaves, exact)
                check(lib.ewn_puct_play(S, L, n, _ptr(scratch[0]), _ptr(cb), _ptr(cd), _ptr(cg), temp_plies, C.c_uint64(key),
                                        C.c_int64(game_offset + i), *[_ptr(rec[name][t, i:i + n]) for name, _, _ in _PLAY_ROWS], st),
                      "ewn_puct_play")
                if (t + 1) % int(check_every) == 0 and bool(cg[:, 1].all()):
                    break
    rec["live"] = rec["live"].view(torch.bool)
    rec["winner"], rec["plies"] = _game_column(game, 2), _game_column(game, 0)
    rec["z"], rec["weight"] = selfplay_outcomes(rec["winner"], rec["live"])
    return rec
