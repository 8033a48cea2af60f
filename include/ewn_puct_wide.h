/*
 * include/ewn_puct_wide.h -- C ABI of libewn_hip.so, continued: the PUCT search in one launch with several leaves per tree and
 * round.
 *
 * A header of its own beside ewn_hip.h, whose codes and conventions it takes (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can be captured into
 * a hipGraph).  It reads no environment variable: `tile` and `blocks` are arguments.  ewn_abi_version() is unchanged.
 *
 * ---- what the search is ----
 * ewn_puct_search (ewn_hip.h) evaluates one leaf per tree per round, and a round costs the two network passes over a 32-column
 * tile whatever the tile holds.  Here a tree collects up to `leaves` = L leaves per round under a virtual loss and has them
 * evaluated together.  The tree is ewn_puct_begin's (ewn_puct_tree_bytes(S, L, sims) bytes, 4-byte aligned, trees back to back,
 * layout 1); ewn_puct_result and ewn_puct_play read it as they read any other.
 *
 * Beside each tree the search keeps integer marks vn[node][6] and vcn[node][6][6], all zero outside a round's span: a mark on
 * (p, a, d) says that a leaf collected in this round and not yet evaluated lies below edge a of node p under dice d.
 * A round of one tree:
 *   (A) evaluate: every pending node in ascending index order.  Its marks are removed along its parent chain -- for each
 *       (p, a, d) up to the root vn[p][a] -= 1, vcn[p][a][d - 1] -= 1 -- then it is evaluated exactly as ewn_puct_advance evaluates
 *       its pending node on that leaf's five logits and value (ewn_puct_advance_noise for the root, when root_noise is given).
 *   (B) walk: count0 = the node count.  While fewer than L leaves are collected and fewer than `sims` simulations have begun, one
 *       walk: ewn_puct_advance's simulation with n + vn for an edge's visits, w - (float)vn for its value sum (one fp32
 *       subtraction of an exactly converted integer) and cn + vcn for its chance counts, nothing else changed.  At the
 *       selected (node j, edge, dice), in this order:
 *         1. the edge wins: the walk's marks (the chain from j) are removed, +1 is backed up from j; the simulation has begun.
 *         2. the child exists and its index is >= count0 -- created in this round, not evaluated yet, a collision: the walk's
 *            marks are removed, the simulation has NOT begun, and the round collects no further leaf.
 *         3. otherwise (j, edge, dice) is marked and the walk descends; where there is no child, node count++ is created as
 *            ewn_puct_advance creates it, the simulation has begun, and the node is pending.
 *       A walk that ewn_puct_advance would break off for its other reasons counts as begun and removes its marks.
 * The first walk of a round cannot collide, so every round begins a simulation; rounds repeat until no node is pending and `sims`
 * simulations have begun, at most sims + 1 of them.  Then hdr[2] = -1, hdr[1] = sims and all marks are zero; a degenerate root is
 * left as ewn_puct_begin leaves it.  With leaves == 1 no mark is ever seen by a walk: every byte of every tree equals
 * ewn_puct_search's with the same arguments (rounds < 0).  The result depends on the observation, params, sims, leaves, c_puct,
 * terminal_value and the noise row alone -- never on tile, blocks or where a tree was held.
 *
 * scratch holds the marks: ewn_puct_search_wide_scratch_bytes(S, L, M, sims) bytes (negative: the EWN_E* code of a call with these
 * arguments; 0 for M == 0), 4-byte aligned.  Its layout is the library's own, and what it held does not matter.
 *
 * tile: the trees a block holds at a time, each with `leaves` of the 32 columns.  0 is the library's choice: ceil(M / 256), at
 * most floor(32 / leaves), at least 1; otherwise 1 .. floor(32 / leaves).  blocks: 0 is the library's choice: 256, never more
 * than ceil(M / tile); otherwise 1 .. EWN_PUCT_WIDE_MAX_BLOCKS (more than ceil(M / tile) launches that many); further tiles are
 * walked grid-stride.
 *
 * Refusals in ewn_puct_search's order and codes, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64;
 * EWN_EUNSUPPORTED by geometry (served: cube_layer 3 on 5x5 and 7x7); EWN_OK without a launch for M == 0; EWN_ENULL for a missing
 * boards, dice, params, tree or scratch; then EWN_EINVAL for sims outside 0 .. 4096, for a tree or scratch that is not 4-byte
 * aligned, for a terminal_value that is not finite and positive, for a c_puct that is not finite and non-negative, for leaves
 * outside 1 .. EWN_PUCT_WIDE_MAX_LEAVES, for tile or blocks outside their ranges and, last and only when root_noise is given, for
 * a noise_eps outside [0, 1].
 * One kernel launch on `stream`; it writes the M trees and the scratch, with vector stores only and no atomics; byte offsets
 * into `tree` and `scratch` are 64-bit.  The same inputs give the same bits.
 */
#ifndef EWN_PUCT_WIDE_H
#define EWN_PUCT_WIDE_H

#include "ewn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EWN_PUCT_WIDE_MAX_LEAVES 32
#define EWN_PUCT_WIDE_MAX_BLOCKS 256

int64_t ewn_puct_search_wide_scratch_bytes(int board_size, int cube_layer, int M, int sims);

int ewn_puct_search_wide(int board_size, int cube_layer, int M, int sims, int leaves,
        float c_puct, float terminal_value,
        const int8_t *boards, const int8_t *dice, const float *params,
        const float *root_noise, float noise_eps,
        int tile, int blocks, void *tree, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PUCT_WIDE_H */
