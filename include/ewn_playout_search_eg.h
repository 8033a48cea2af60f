/*
 * include/ewn_playout_search_eg.h -- C ABI of libewn_hip.so, continued: the playout tree search of ewn_playout_search.h with exact
 * endgame values at the leaves that an endgame table covers.
 *
 * A header of its own beside ewn_playout_search.h, whose entry, constants and conventions it takes (device pointers owned by the
 * caller, `stream` a hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can
 * be captured into a hipGraph; no environment variable is read).  ewn_abi_version() is unchanged.
 *
 * ---- the definition ----
 * `table` is the table that ewn_endgame_build(board_size, max_cubes, max_total) wrote (layout version 1, 4-byte aligned,
 * ewn_endgame_table_bytes() bytes).  It is only read, and it must be complete before this call in stream order: built on the same
 * stream, or the building stream synchronised first.  When ewn_playout_search_eg finishes, every byte of `tree` equals what
 * ewn_playout_search's sequence leaves there with one change.  In round r, for every tree with a pending leaf:
 *     ewn_endgame_lookup(table, the leaf rows, the leaf dice) -> actions, q, covered;
 *     where covered: value = q at the action the lookup returns, which is the first maximum of the six q in action order under a
 *                    strict > (that also fixes the sign of a zero); no playout runs for that leaf;
 *     elsewhere:     value = fl(float(2 w - playouts) / float(playouts)) of ewn_playout_wins, as in ewn_playout_search: the same
 *                    key_r = key + r * 0x9E3779B97F4A7C15 and the same row index obs_id0 + m.  The playouts are keyed by round and
 *                    row, not by a running counter, so a covered leaf in one round moves no playout of another.
 *     ewn_puct_advance(logits = 0, value, terminal_value = 1).
 * A tree without a pending leaf is not looked up.  The leaf row is the node's board seen from its side to move, which is the view
 * the table is indexed by.  The coverage test is ewn_endgame_lookup's on every board, malformed ones included: cell values within
 * -6 .. 6, no cube number twice on a side, no agent cube on the last cell, no opposing cube on cell 0, 1 .. max_cubes cubes a side
 * and at most max_total in all.  rounds, blocks, obs_id0: as in ewn_playout_search.
 *
 * leaf_counts: NULL, or int32 [M][2], 4-byte aligned: per tree {the rounds whose pending leaf the table valued, the rounds whose
 * pending leaf playouts valued}, over the rounds run; their sum is the number of rounds in which the tree had a pending leaf.
 * Every element is written; what it held does not matter.
 *
 * Refusals in ewn_playout_search's order, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by
 * geometry; EWN_OK without a launch for M == 0, before anything else is looked at; EWN_ENULL for a missing table, boards, dice or
 * tree; EWN_EINVAL for sims, the tree's alignment, playouts, c_puct and blocks as there; then the table's: EWN_EINVAL for
 * (board_size, max_cubes, max_total) that ewn_endgame_table_bytes() refuses, and for a table or leaf_counts that is not 4-byte
 * aligned.
 * One kernel launch on `stream`; it writes exactly the M trees and leaf_counts, with vector stores only and no atomics on global
 * memory; every index into the table lies inside it.  The same inputs give the same bits.
 */
#ifndef EWN_PLAYOUT_SEARCH_EG_H
#define EWN_PLAYOUT_SEARCH_EG_H

#include "ewn_playout_search.h"

#ifdef __cplusplus
extern "C" {
#endif

int ewn_playout_search_eg(int board_size, int cube_layer, int M, int sims, int rounds, int playouts, float c_puct, uint64_t key,
                          uint32_t obs_id0, int blocks, int max_cubes, int max_total, const float *table,
                          const int8_t *boards, const int8_t *dice, void *tree, int32_t *leaf_counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PLAYOUT_SEARCH_EG_H */
