/*
 * include/ewn_playout_search.h -- C ABI of libewn_hip.so, continued: the PUCT tree search that needs no network.
 *
 * A header of its own beside ewn_hip.h, whose codes and conventions it takes (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can be captured into
 * a hipGraph).  It reads no environment variable: its one tuning knob, `blocks`, is an argument.  ewn_abi_version() is unchanged.
 *
 * ---- uniform priors, random playouts at the leaves, one launch ----
 * A tree is ewn_puct_begin's (ewn_puct_tree_bytes(S, L, sims) bytes, 4-byte aligned, trees back to back).  When
 * ewn_playout_search finishes, every byte of `tree` equals what this sequence leaves there:
 *   ewn_puct_begin(boards, dice); then for round r = 0 .. R - 1
 *     w     = ewn_playout_wins(the leaf rows, first_player = 1, n_sims = playouts, key_r), tree m's leaf row standing at row index
 *             obs_id0 + m of that call (the index keys the playouts: playout x of the row starts from
 *             seed(philox word of (obs_id0 + m, 0x53494D55, key_r), x), x = 0 .. playouts - 1);
 *     value = fl(float(2 w - playouts) / float(playouts)): the share of playouts the side to move at the leaf won, on [-1, 1];
 *     ewn_puct_advance(logits = 0, value, terminal_value = 1).
 * key_r = key + r * 0x9E3779B97F4A7C15 (mod 2^64).  R = sims + 1 when rounds < 0, min(rounds, sims + 1) otherwise; rounds == 0 is
 * ewn_puct_begin alone.  Zero logits make the priors uniform over a node's legal edges.  A leaf row is the node's board seen from
 * its side to move, which is ewn_playout_wins' TOP_LEFT and moves first; a leaf is never a finished position (a winning move is
 * backed up without a node).  A tree without a pending leaf in a round -- a degenerate root, a simulation that ended on a winning
 * edge, a used-up budget -- gets no playouts in it, and no value is read for it.  What `tree` held before the call does not
 * matter; ewn_puct_result and ewn_puct_play read the finished tree as they read any other.  obs_id0 + m wraps at 2^32.
 *
 * blocks: 0 is the library's choice; 1 .. EWN_PLAYOUT_SEARCH_MAX_BLOCKS pins the grid (four trees per block and trip, further
 * trees grid-stride).  It changes no byte of the result.
 *
 * Refusals in this order, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by geometry (served:
 * cube_layer 3 on 5x5 and 7x7, as ewn_policy_param_count()); EWN_OK without a launch for M == 0; EWN_ENULL for a missing boards,
 * dice or tree; then EWN_EINVAL for sims outside 0 .. 4096, for a tree that is not 4-byte aligned, for playouts outside
 * 1 .. EWN_PLAYOUT_SEARCH_MAX_PLAYOUTS, for a c_puct that is not finite and non-negative, and for blocks outside
 * 0 .. EWN_PLAYOUT_SEARCH_MAX_BLOCKS.
 * One kernel launch on `stream`; it writes exactly the M trees, with vector stores only and no atomics on global memory; byte
 * offsets into `tree` are 64-bit.  The same inputs give the same bits.
 */
#ifndef EWN_PLAYOUT_SEARCH_H
#define EWN_PLAYOUT_SEARCH_H

#include "ewn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EWN_PLAYOUT_SEARCH_MAX_PLAYOUTS 4096
#define EWN_PLAYOUT_SEARCH_MAX_BLOCKS 4096

int ewn_playout_search(int board_size, int cube_layer, int M, int sims, int rounds, int playouts, float c_puct,
                       uint64_t key, uint32_t obs_id0, int blocks,
                       const int8_t *boards, const int8_t *dice, void *tree, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PLAYOUT_SEARCH_H */
