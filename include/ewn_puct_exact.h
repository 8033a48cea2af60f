/*
 * include/ewn_puct_exact.h -- C ABI of libewn_hip.so, continued: the one-launch PUCT search of ewn_puct_search (ewn_hip.h) with
 * exact endgame values at the leaves that an endgame table covers.
 *
 * A header of its own beside ewn_hip.h, whose codes and conventions it takes (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can be captured into
 * a hipGraph).  It reads no environment variable: `tile` and `blocks` are arguments.  ewn_abi_version() is unchanged, and so is
 * the trees' layout.
 *
 * ---- the definition ----
 * `table` is the table that ewn_endgame_build(board_size, max_cubes, max_total) wrote (layout version 1, 4-byte aligned,
 * ewn_endgame_table_bytes() bytes).  It is only read, and it must be complete before this call in stream order: built on the same
 * stream, or the building stream synchronised first.  When ewn_puct_search_eg finishes, every byte of `tree` equals what this
 * sequence leaves there: ewn_puct_begin, then in round r = 0 .. R - 1, on the leaf rows and leaf dice,
 *     ewn_predict_policy(deterministic = 1)              -> logits, value;
 *     ewn_endgame_lookup(table, leaf rows, leaf dice)    -> actions, q, covered;
 *     where covered: value = fl(terminal_value * q at the action the lookup returns), which is the first maximum of the six q in
 *                    action order under a strict > (that also fixes the sign of a zero); the logits stay the policy head's;
 *     ewn_puct_advance(logits, value) -- in round 0 ewn_puct_advance_noise(root_noise, noise_eps) when root_noise is given.
 * The backup therefore sees fl(fl(terminal_value * q) * fl(1 / terminal_value)), clamped to [-1, 1] as every leaf value is.  A
 * tree without a pending leaf shows a zero board as its leaf row and is not covered.  The coverage test is ewn_endgame_lookup's on
 * every board, malformed ones included: cell values within -6 .. 6, no cube number twice on a side, no agent cube on the last cell,
 * no opposing cube on cell 0, 1 .. max_cubes cubes a side and at most max_total in all.  R and `rounds`: as in ewn_puct_search
 * (rounds < 0 or > sims + 1: all sims + 1).
 *
 * leaf_counts: NULL, or int32 [M][2], 4-byte aligned: per tree {the rounds whose pending leaf the table valued, the rounds whose
 * pending leaf the value head valued}, over the rounds run; their sum is the number of rounds in which the tree had a pending
 * leaf.  Every element is written; what it held does not matter.
 *
 * tile: the trees a block holds at a time.  0 is the library's choice: ceil(M / 256), at most 32; otherwise 1 .. 32.  blocks: 0 is
 * the library's choice: 256, never more than ceil(M / tile); otherwise 1 .. EWN_PUCT_EXACT_MAX_BLOCKS (never more than
 * ceil(M / tile) are launched); further tiles are walked grid-stride.  No byte of the result depends on either.
 *
 * Refusals in ewn_puct_search's order and codes, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64;
 * EWN_EUNSUPPORTED by geometry (served: cube_layer 3 on 5x5 and 7x7); EWN_OK without a launch for M == 0, before anything else is
 * looked at; EWN_ENULL for a missing boards, dice, params, tree or table; then EWN_EINVAL for sims outside 0 .. 4096, for a tree
 * that is not 4-byte aligned, for a terminal_value that is not finite and positive, for a c_puct that is not finite and
 * non-negative and, only when root_noise is given, for a noise_eps outside [0, 1]; then EWN_EINVAL for tile or blocks outside their
 * ranges, for (board_size, max_cubes, max_total) that ewn_endgame_table_bytes() refuses, and for a table or leaf_counts that is not
 * 4-byte aligned.
 * One kernel launch on `stream`; it writes exactly the M trees and leaf_counts, with vector stores only and no atomics; every
 * index into the table lies inside it; byte offsets into `tree` are 64-bit.  The same inputs give the same bits.
 */
#ifndef EWN_PUCT_EXACT_H
#define EWN_PUCT_EXACT_H

#include "ewn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EWN_PUCT_EXACT_MAX_TILE 32
#define EWN_PUCT_EXACT_MAX_BLOCKS 256

int ewn_puct_search_eg(int board_size, int cube_layer, int M, int sims, int rounds, float c_puct, float terminal_value,
        const int8_t *boards, const int8_t *dice, const float *params, const float *root_noise, float noise_eps,
        int tile, int blocks, int max_cubes, int max_total, const float *table, void *tree, int32_t *leaf_counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PUCT_EXACT_H */
