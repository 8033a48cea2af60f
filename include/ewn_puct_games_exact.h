/*
 * include/ewn_puct_games_exact.h -- C ABI of libewn_hip.so, continued: the whole self-play games of ewn_puct_selfplay (ewn_hip.h) with
 * exact endgame values at the leaves that an endgame table covers.
 *
 * A header of its own beside ewn_hip.h, whose codes and conventions it takes (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void *, 0 or a negative EWN_E* code, nothing allocated or synchronised, so the call can be captured into
 * a hipGraph).  It reads no environment variable.  ewn_abi_version() is unchanged, and so is the trees' layout.
 *
 * ---- the definition ----
 * ewn_puct_selfplay's games, records and in-place updates (ewn_hip.h), with one change: a ply's search is ewn_puct_search_eg's
 * (ewn_puct_exact.h) on `table` instead of ewn_puct_search's.  Per ply of game m: ewn_puct_search_eg on its position with all
 * sims + 1 rounds (round 0 with row (ply * M + m) of `noise` when noise != NULL), then ewn_puct_play with key and game_offset + m
 * into row `ply` of the record buffers.  A pending leaf that the table covers is therefore worth fl(terminal_value * q) at the
 * first maximum of the six q in action order under a strict >, every other leaf the value head's output; the logits are always the
 * policy head's.  The records, boards, dice and game equal what that ply-by-ply sequence leaves, byte for byte; what scratch, the
 * record buffers or leaf_counts held before the call does not matter.
 *
 * `table` is the table that ewn_endgame_build(board_size, max_cubes, max_total) wrote (layout version 1, 4-byte aligned,
 * ewn_endgame_table_bytes() bytes).  It is only read, and it must be complete before this call in stream order.
 *
 * leaf_counts: NULL, or int32 [M][2], 4-byte aligned: per game the sums of ewn_puct_search_eg's leaf_counts over the plies this
 * call played for it: {the rounds whose pending leaf the table valued, the rounds whose pending leaf the value head valued}.  A
 * game that is not played (it enters over, or with a ply outside 0 .. max_plies - 1) has zeros; a game that enters at ply p > 0
 * counts the plies played here.  Every element is written.  The counts are 32 bits wide: a game can pass 65 535.
 *
 * tile, blocks and scratch: ewn_puct_selfplay's, scratch sized by ewn_puct_selfplay_scratch_bytes.  No byte of the result depends
 * on tile or blocks.
 *
 * Refusals, all before the launch: EWN_EINVAL for M < 0 or M > INT_MAX / 64; EWN_EUNSUPPORTED by geometry (served: cube_layer 3 on
 * 5x5 and 7x7); EWN_OK without a launch for M == 0, before anything else is looked at; EWN_ENULL for a missing params, boards,
 * dice, game, scratch or table; then EWN_EINVAL for sims outside 0 .. 4096, a scratch or game that is not 4-byte aligned, a
 * terminal_value that is not finite and positive, a c_puct that is not finite and non-negative; for max_plies < 1, temp_plies < 0,
 * tile outside 0 .. 32, blocks outside 0 .. 256; for (board_size, max_cubes, max_total) that ewn_endgame_table_bytes() refuses;
 * for a table or a given leaf_counts that is not 4-byte aligned; and last, only when noise is given, for a noise_eps that is not
 * finite or outside [0, 1].
 * One kernel launch on `stream`; vector stores only, no atomics; every index into the table lies inside it; all row offsets are
 * 64-bit.  The same inputs give the same bits.
 */
#ifndef EWN_PUCT_GAMES_EXACT_H
#define EWN_PUCT_GAMES_EXACT_H

#include "ewn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ewn_puct_selfplay_eg(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value,
        const float *params, const float *noise /* [max_plies][M][6] or NULL */, float noise_eps,
        int temp_plies, uint64_t key, int64_t game_offset, int tile, int blocks,
        int8_t *boards, int8_t *dice, int32_t *game,
        int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
        void *scratch, int max_cubes, int max_total, const float *table, int32_t *leaf_counts /* [M][2] or NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EWN_PUCT_GAMES_EXACT_H */
