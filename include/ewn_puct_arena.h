/*
 * include/ewn_puct_arena.h -- C ABI of libewn_hip.so, continued: the arena, whole games between the PUCT searches of two networks in
 * one launch.
 *
 * A header of its own beside ewn_hip.h, whose codes and conventions it takes (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can be captured into
 * a hipGraph).  It reads no environment variable.  ewn_abi_version() is unchanged, and so is the trees' layout.
 *
 * ---- the definition ----
 * ewn_puct_selfplay's games, records and in-place updates (ewn_hip.h), with one change: the network that searches a ply is the
 * ply's mover's.  The mover of ply t of game m is network A (`params`) when (t + first[m]) is even, network B (`params_b`)
 * otherwise; only bit 0 of first[m] is read, and first == NULL is all zeros: A moves at the even plies of every game.  Per ply of
 * game m: ewn_puct_search on its position with the mover's parameters and all sims + 1 rounds (round 0 with row (ply * M + m) of
 * `noise` when noise != NULL), then ewn_puct_play with key and game_offset + m into row `ply` of the record buffers.  The records,
 * boards, dice and game equal what that ply-by-ply sequence leaves, byte for byte; what scratch or the record buffers held before
 * the call does not matter.  game[m] = {ply, over, winner, 0} is ewn_puct_play's: winner is +1 for the side that moves at even
 * plies, which is A where first[m] is even and B where it is odd.  A game that enters at ply p > 0 is played from there, and its
 * mover is (p + first[m]) & 1 as at any other ply.
 *
 * tile, blocks and scratch: ewn_puct_selfplay's; ewn_puct_arena_scratch_bytes is ewn_puct_selfplay_scratch_bytes' rule, blocks x
 * tile trees of ewn_puct_tree_bytes() for the effective values.  A block holds the weights of one network at a time and plays, in
 * turns, the columns that wait for it.  No byte of the result depends on tile or blocks.
 *
 * Refusals, ewn_puct_selfplay's in its order, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by
 * geometry (served: cube_layer 3 on 5x5 and 7x7); EWN_OK without a launch for M == 0, before anything else is looked at; EWN_ENULL
 * for a missing params, params_b, boards, dice, game or scratch; then EWN_EINVAL for sims outside 0 .. 4096, a scratch or game that
 * is not 4-byte aligned, a terminal_value that is not finite and positive, a c_puct that is not finite and non-negative; for
 * max_plies < 1, temp_plies < 0, tile outside 0 .. 32, blocks outside 0 .. 256; and last, only when noise is given, for a noise_eps
 * that is not finite or outside [0, 1].
 * One kernel launch on `stream`; vector stores only, no atomics; all row offsets are 64-bit.  The same inputs give the same bits.
 */
#ifndef EWN_PUCT_ARENA_H
#define EWN_PUCT_ARENA_H

#include "ewn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t ewn_puct_arena_scratch_bytes(int board_size, int cube_layer, int M, int sims, int tile, int blocks);
int ewn_puct_arena(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value,
        const float *params, const float *params_b, const float *noise /* [max_plies][M][6] or NULL */, float noise_eps,
        int temp_plies, uint64_t key, int64_t game_offset, int tile, int blocks,
        int8_t *boards, int8_t *dice, int32_t *game, const int8_t *first /* [M] or NULL */,
        int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
        void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PUCT_ARENA_H */
