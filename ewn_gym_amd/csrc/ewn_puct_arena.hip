// ewn_puct_arena.hip -- the arena: whole games between two networks' PUCT searches in one launch (C ABI: ewn_puct_arena,
// ewn_puct_arena_scratch_bytes, include/ewn_puct_arena.h).  A game's records are, byte for byte, what arena_puct's ply
// loop leaves: per ply ewn_puct_search with the MOVER's parameters (round 0 with that ply's noise row) and ewn_puct_play.  The mover
// of ply t of game m is network A (`params`) when (t + first[m]) is even and network B (`params_b`) otherwise.  The tree code and the
// move are ewn_puct.hpp's, the one copy every PUCT kernel calls; the network code is ewn_predict_policy's under the same compiler
// flags; the game loop is k_puct_selfplay's (ewn_puct_games.hip) with one addition: a phase has a network.
//
// Four weight images do not fit the CU's LDS at 7x7, so the block keeps two, as k_puct_selfplay does -- the policy and the value image
// of ONE network -- and repacks them when the phase's network changes.  A block has `tile` columns and owns a fixed, contiguous set
// of the M games exactly as there.  A phase is block-uniform:
//   refill:  wave 0's, unchanged: a column without a game takes the set's next game, in the set's order; bit 0 of first[m] goes into an
//            LDS word of the column.  A game that enters over, or with ply >= max_plies, is not played: its record rows are zeroed
//   network: wave 0 counts the held columns whose mover, (ply + first) & 1, is A and those whose mover is B, and writes the network
//            with more waiting columns (a tie: A) into a control word, and per column whether it plays in this phase: it holds a game
//            and its mover is the phase's network
//   stop:    the block stops when no column holds a game
//   pack:    when the phase's network is not the one the images hold, all 512 threads pack its two images (mlp3_pack_fwd), between the
//            barrier that follows the refill and the barrier that follows the fill of the trees: no barrier is added.  The last readers
//            of the old images, the last phase's final round, lie before that phase's play barrier
//   begin, search, play: k_puct_selfplay's, on the columns that play.  A waiting column keeps its game and its ply; its slot stays a
//            zero board with dice 1 (the slots are zeroed every phase), its tree is neither filled nor read
//
// What follows from this, beside the rules of ewn_puct_games.hip's header, which hold as written there:
//   Barriers and exits.  Every barrier and the loop's exit are block-uniform: the stop word, the phase's network and the columns' play
//     flags are LDS words written by wave 0 and read by every wave after the barrier that follows the refill; the network the images
//     hold is a register that every thread computes from that same word.
//   Progress.  In every phase with a held column the network with more waiting columns has at least one, so at least one game advances
//     a ply.  A game ends, or is cut at max_plies, so the loop ends.
//   Columns stay in step.  A column that plays in a phase waits for the other network in the next phase, as does every other column
//     that played: once a block's columns agree they alternate together, and each phase then searches every held column.  A refilled
//     column is out of step for at most one phase per game.
//   Independence from the layout.  A column's network outputs depend on that column and the phase's images alone, and the images on
//     the mover of the games that play: a game's records depend on its inputs, first[m], key, game_offset + m and its noise rows only,
//     not on tile, blocks, or what shares its block.
//   Hand-over between lanes, range checks, no atomics, vector stores only, plain C++, prior contents: as in ewn_puct_games.hip.  The
//     column's first bit is written by wave 0's lane 0 at the refill and read by wave 0 in later phases, across block barriers.
#include "ewn_puct.hpp"
#include "../../include/ewn_puct_arena.h"

#define PUA_NT 512           // threads per block: eight waves, as k_puct_selfplay
#define PUA_NW (PUA_NT / 64)
#define PUA_TILE 32          // the most columns of a block: the columns of an MFMA tile
#define PUA_MAX_BLOCKS 256   // one block per CU

// LDS of k_puct_arena<S, .>: policy image | value image (of the phase's network) | 32 slots of RecGeo<S>::STR bytes | dice [32] |
// logits [32][8] | value [32] | per wave PU_WAVE bytes | the columns' games int [32] | their plies int [32] | their first bits int [32] |
// whether they play in this phase int [32] | 4 words of the block's own (word 0: a column holds a game, word 1: the phase's network)
template <int S> struct PuaGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    static constexpr int O_SLOTS = 2 * Mlp3Geo<S>::FWD_BYTES;
    static constexpr int O_DICE = O_SLOTS + PUA_TILE * STR;
    static constexpr int O_LOGITS = O_DICE + PUA_TILE;
    static constexpr int O_VALUE = O_LOGITS + PUA_TILE * 8 * 4;
    static constexpr int O_WAVES = O_VALUE + PUA_TILE * 4;
    static constexpr int O_GAME = O_WAVES + PUA_NW * PU_WAVE;
    static constexpr int O_PLY = O_GAME + PUA_TILE * 4;
    static constexpr int O_FIRST = O_PLY + PUA_TILE * 4;
    static constexpr int O_PLAYS = O_FIRST + PUA_TILE * 4;
    static constexpr int O_CTRL = O_PLAYS + PUA_TILE * 4;
    static constexpr size_t lds_bytes() { return (size_t)O_CTRL + 16; }
    static_assert(Mlp3Geo<S>::FWD_BYTES % 16 == 0 && STR % 16 == 0 && PU_WAVE % 16 == 0, "every region starts on a 16-byte boundary");
    static_assert(CELLS <= STR, "a slot holds the board");
    static_assert(lds_bytes() <= POL_LDS_MAX, "two weight images + the tile's slots, outputs, the waves' own and the columns' words must fit the CU's LDS");
};

struct PuaBuf {
    const float *params, *params_b; const float *noise; float eps, keep; int8_t *boards; int8_t *dice; int *game; const int8_t *first;
    PuRecord rec; uint8_t *scratch;                            // rec: rows [max_plies][M], row ply * M + m is game m's ply
};

// zeros into rows t0 .. t1 - 1 of game m, by one wave
template <int CELLS>
EWN_DEV void pua_zero_rows(const PuRecord &R, int M, int m, int t0, int t1, int lane)
{
    #pragma unroll 1
    for (int t = t0; t < t1; t++) {                            // wave-uniform
        const size_t r = (size_t)t * (size_t)M + (size_t)m;
        if (lane < CELLS && R.board) R.board[r * CELLS + lane] = 0;
        if (lane < 6 && R.visits) R.visits[r * 6 + lane] = 0;
        if (lane < 2 && R.action) R.action[r * 2 + lane] = 0;
        if (lane == 0) {
            if (R.dice) R.dice[r] = 0;
            if (R.value) R.value[r] = 0.0f;
            if (R.live) R.live[r] = 0;
        }
    }
}

// tile: the columns of a block, 1 .. PUA_TILE; the grid's blocks share the M games (M >= 1, gridDim.x <= ceil(M / tile))
template <int S, bool NOISE>
__global__ __launch_bounds__(PUA_NT, 1) void k_puct_arena(int M, int sims, int max_plies, int tile, int temp_plies, float c_puct, float inv_tv,
                                                          u32 k0, u32 k1, long long game_offset, PuLayout L, PuaBuf B)
{
    using P = PuaGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR;
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wpi = lds, *Wvf = lds + Q3::FWD_BYTES;
    int8_t *slots = lds + P::O_SLOTS, *sdice = lds + P::O_DICE;
    float *slg = (float *)(lds + P::O_LOGITS), *sval = (float *)(lds + P::O_VALUE);
    int *sgame = (int *)(lds + P::O_GAME), *sply = (int *)(lds + P::O_PLY), *sfirst = (int *)(lds + P::O_FIRST);
    int *splays = (int *)(lds + P::O_PLAYS), *ctrl = (int *)(lds + P::O_CTRL);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + P::O_WAVES + wave * PU_WAVE;
    if (threadIdx.x < PUA_TILE) sgame[threadIdx.x] = -1;

    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;
    const size_t tree0 = (size_t)blockIdx.x * (size_t)tile;    // the block's first tree of `scratch`
    // the block's set of games: next .. end - 1; `next` is wave 0's alone
    int next = (int)((long long)blockIdx.x * (long long)M / (long long)gridDim.x);
    const int end = (int)(((long long)blockIdx.x + 1) * (long long)M / (long long)gridDim.x);
    const int j = lane & 31, h = lane >> 5;
    int packed = -1;                                           // the network the images hold: block-uniform, none yet

    #pragma unroll 1
    for (;;) {                                                 // a phase: block-uniform
        __syncthreads();                                       // the last phase's moves are made, its slots and images read
        if (wave == 0) {                                       // ---- refill, and the phase's network
            u32 held = 0u, moves_b = 0u;                       // wave-uniform masks over the columns: holds a game; its mover is B
            #pragma unroll 1
            for (int k = 0; k < tile; k++) {                   // wave-uniform
                int m = __builtin_amdgcn_readfirstlane(sgame[k]);   // a column's words are the same for every lane
                int ply = 0, fst = 0;
                if (m >= 0) { ply = __builtin_amdgcn_readfirstlane(sply[k]); fst = __builtin_amdgcn_readfirstlane(sfirst[k]); }
                #pragma unroll 1
                while (m < 0 && next < end) {
                    const int cand = next++;
                    const int *g = B.game + (size_t)cand * 4;
                    const int p0 = __builtin_amdgcn_readfirstlane(g[0]), over = __builtin_amdgcn_readfirstlane(g[1]);
                    if (over != 0 || p0 < 0 || p0 >= max_plies) {   // not played: its rows are zeros
                        pua_zero_rows<CELLS>(B.rec, M, cand, 0, max_plies, lane);
                        continue;
                    }
                    pua_zero_rows<CELLS>(B.rec, M, cand, 0, p0, lane);
                    m = cand;
                    ply = p0;
                    fst = B.first ? __builtin_amdgcn_readfirstlane((int)B.first[cand]) & 1 : 0;
                    if (lane == 0) { sgame[k] = cand; sply[k] = p0; sfirst[k] = fst; }
                }
                if (m >= 0) {
                    held |= 1u << k;
                    if ((ply + fst) & 1) moves_b |= 1u << k;
                }
            }
            const int nb = __builtin_popcount(moves_b), na = __builtin_popcount(held) - nb;
            const int net = nb > na ? 1 : 0;                   // the network with more waiting columns; a tie: A
            const u32 plays = net ? moves_b : held & ~moves_b;
            if (lane < PUA_TILE) splays[lane] = (int)((plays >> lane) & 1u);
            if (lane == 0) { ctrl[0] = held != 0u; ctrl[1] = net; }
        }
        for (int i = threadIdx.x; i < PUA_TILE * STR / 4; i += PUA_NT) ((u32 *)slots)[i] = 0u;
        if (threadIdx.x < PUA_TILE) sdice[threadIdx.x] = 1;
        __syncthreads();                                       // the columns' games and flags, the stop word and the network are there; the slots are zero
        if (__builtin_amdgcn_readfirstlane(ctrl[0]) == 0) break;                               // ---- stop: every wave reads the same word
        const int net = __builtin_amdgcn_readfirstlane(ctrl[1]);
        if (net != packed) {                                   // ---- pack: block-uniform; read first in round 0, two barriers on
            const float *params = net ? B.params_b : B.params;
            mlp3_pack_fwd<S>(Wpi, params, 0, threadIdx.x, PUA_NT);
            mlp3_pack_fwd<S>(Wvf, params, 1, threadIdx.x, PUA_NT);
            packed = net;
        }
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUA_NW) {            // ---- begin: the fill of this wave's trees that play
            if (__builtin_amdgcn_readfirstlane(splays[k]) == 0) continue;   // wave-uniform
            u32 *t = (u32 *)(B.scratch + (tree0 + (size_t)k) * (size_t)L.bytes);
            #pragma unroll 1
            for (u32 i = lane; i < words; i += 64) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                       // the fill is done before the roots go over it
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUA_NW) {
            if (__builtin_amdgcn_readfirstlane(splays[k]) == 0) continue;
            const size_t m = (size_t)__builtin_amdgcn_readfirstlane(sgame[k]);
            pu_root<S>(pu_tree(B.scratch, tree0 + (size_t)k, L), B.boards + m * CELLS, B.dice + m, sims, slots + k * STR, sdice + k, lane, base);
        }
        #pragma unroll 1
        for (int rnd = 0; rnd <= sims; rnd++) {                // ---- search: k_puct_search's round, on the phase's images
            __syncthreads();                                   // the leaves are in the slots, the trees' words are handed over; round 0: the images are packed
            if (wave < 2) {                                    // wave-uniform
                const int8_t *sj = slots + j * STR + 8 * h;
                const int dj = (int)sdice[j];
                auto xb = [&](int kb) { return pol_obs_operand<S>(sj, kb, h, dj); };
                f32x16 h1[2], h2[2];
                if (wave == 0) {
                    float lo[MLP_NA];
                    mlp3_forward<S, MLP_NA>(Wpi, lane, xb, h1, h2, lo);
                    if (h == 0) { float *p = slg + j * 8; p[0] = lo[0]; p[1] = lo[1]; p[2] = lo[2]; p[3] = lo[3]; p[4] = lo[4]; }
                } else {
                    float vo[1];
                    mlp3_forward<S, 1>(Wvf, lane, xb, h1, h2, vo);
                    if (h == 0) sval[j] = vo[0];
                }
            }
            __syncthreads();                                   // logits and value are there; the slots are read
            #pragma unroll 1
            for (int k = wave; k < tile; k += PUA_NW) {
                if (__builtin_amdgcn_readfirstlane(splays[k]) == 0) continue;   // waits, or holds no game: its slot stays a zero board with dice 1
                const int m0 = __builtin_amdgcn_readfirstlane(sgame[k]);
                PuNoise Z = { nullptr, 0.0f, 0.0f };
                if constexpr (NOISE) Z = PuNoise{ B.noise + ((size_t)__builtin_amdgcn_readfirstlane(sply[k]) * (size_t)M + (size_t)m0) * 6, B.eps, B.keep };
                // the noise instance is round 0's alone: on later rounds the pending node is never the root, and pu_evaluate asks
                pu_round<S, NOISE>(pu_tree(B.scratch, tree0 + (size_t)k, L), sims, c_puct, inv_tv, L.nodes, slg + k * 8, sval + k, Z, slots + k * STR,
                                   sdice + k, lane, base);
            }
        }
        __syncthreads();                                       // ---- play: the last round's header and root are handed over
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUA_NW) {
            if (__builtin_amdgcn_readfirstlane(splays[k]) == 0) continue;
            const int m0 = __builtin_amdgcn_readfirstlane(sgame[k]);
            const size_t m = (size_t)m0;
            const int ply = __builtin_amdgcn_readfirstlane(sply[k]);
            const bool goes_on = pu_play<S>(pu_tree(B.scratch, tree0 + (size_t)k, L), true, sims, L.nodes, B.boards + m * CELLS, B.dice + m,
                                            B.game + m * 4, temp_plies, k0, k1, (unsigned long long)game_offset + (unsigned long long)m, B.rec,
                                            (size_t)ply * (size_t)M + m, lane, base);
            if (goes_on && ply + 1 < max_plies) {
                if (lane == 0) sply[k] = ply + 1;
            } else {                                           // over, or cut at max_plies: the remaining rows, and the column is free
                pua_zero_rows<CELLS>(B.rec, M, m0, ply + 1, max_plies, lane);
                if (lane == 0) sgame[k] = -1;
            }
        }
    }
}

template <int S, bool NOISE>
static int pua_launch(int M, int sims, int max_plies, int tile, int blocks, int temp_plies, float c_puct, float inv_tv, uint64_t key,
                      int64_t game_offset, const PuaBuf &b, hipStream_t s)
{
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_arena<S, NOISE>, (unsigned)blocks, PUA_NT, PuaGeo<S>::lds_bytes(), 64 * 1024, POL_LDS_MAX, s, M, sims, max_plies,
                             tile, temp_plies, c_puct, inv_tv, (u32)key, (u32)(key >> 32), (long long)game_offset, L, b);
}

// ewn_puct_selfplay's choice where tile or blocks is 0: every CU gets a block, and the columns are as few as still hold all M games
// at once, ceil(M / 256) and at most 32; never more blocks than ceil(M / tile)
static inline void pua_geometry(int M, int &tile, int &blocks)
{
    if (tile == 0) {
        const int t = (M - 1) / PUA_MAX_BLOCKS + 1;
        tile = t > PUA_TILE ? PUA_TILE : t;
    }
    if (blocks == 0) blocks = PUA_MAX_BLOCKS;
    const int most = (M - 1) / tile + 1;
    if (blocks > most) blocks = most;
}

// ewn_puct_selfplay_scratch_bytes' rule: pu_refuse, then the range of sims, tile and blocks; M == 0: 0
int64_t ewn_puct_arena_scratch_bytes(int board_size, int cube_layer, int M, int sims, int tile, int blocks)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK) return rc;
    if (sims < 0 || sims > PU_MAX_SIMS || tile < 0 || tile > PUA_TILE || blocks < 0 || blocks > PUA_MAX_BLOCKS) return EWN_EINVAL;
    if (M == 0) return 0;
    pua_geometry(M, tile, blocks);
    return pu_layout(board_size, sims).bytes * (long long)tile * (long long)blocks;
}

// ewn_puct_selfplay's refusals in its order, params_b among the pointers, all before the launch; first and noise may be NULL, and
// noise_eps is looked at only when noise is given
int ewn_puct_arena(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value, const float *params,
                   const float *params_b, const float *noise, float noise_eps, int temp_plies, uint64_t key, int64_t game_offset, int tile,
                   int blocks, int8_t *boards, int8_t *dice, int32_t *game, const int8_t *first, int8_t *rec_board, int8_t *rec_dice,
                   int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live, void *scratch, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;                     // the empty batch: EWN_OK before anything else is looked at
    if (!(params && params_b && boards && dice && game && scratch)) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)scratch & 3) || ((uintptr_t)game & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (max_plies < 1 || temp_plies < 0 || tile < 0 || tile > PUA_TILE || blocks < 0 || blocks > PUA_MAX_BLOCKS) return EWN_EINVAL;
    if (noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    pua_geometry(M, tile, blocks);
    PuaBuf b = { params, params_b, noise, noise ? noise_eps : 0.0f, noise ? 1.0f - noise_eps : 1.0f, boards, dice, (int *)game, first,
                 PuRecord{ rec_board, rec_dice, (int *)rec_visits, rec_value, rec_action, rec_live }, (uint8_t *)scratch };
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    if (noise)
        return board_size == 5 ? pua_launch<5, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s)
                               : pua_launch<7, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s);
    return board_size == 5 ? pua_launch<5, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s)
                           : pua_launch<7, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s);
}
