// ewn_puct_games.hip -- whole self-play games of the PUCT search in one launch, finished columns refilled (C ABI: ewn_puct_selfplay,
// ewn_puct_selfplay_scratch_bytes).  A game's records are, byte for byte, what selfplay_puct's ply loop leaves: per
// ply ewn_puct_search (round 0 with that ply's noise row) and ewn_puct_play.  The tree code and the move are ewn_puct.hpp's, the one
// copy the staged kernels call; the network code is ewn_predict_policy's under the same compiler flags; the round structure is
// k_puct_search's (ewn_puct_fused.hip) with a game loop round it.
//
// A block has `tile` columns (1 .. 32, the columns of the MFMA tiles) and owns a fixed, contiguous set of the M games: block b of nb
// owns games b M / nb .. (b + 1) M / nb - 1, a function of M, tile and blocks alone.  Column k lives on wave k % PUG_NW and on tree
// blockIdx * tile + k of `scratch` for the whole launch; which game it holds (or none, -1) and that game's ply stand in LDS.
// A phase is block-uniform:
//   refill:  wave 0 hands every column without a game the set's next game, in the set's order.  A game that enters over, or with
//            ply >= max_plies, is not played: its record rows are zeroed and the column takes the next one
//   stop:    the block stops when no column holds a game (the set is then used up): one LDS word, read by every wave after a barrier
//   begin:   the slots are zeroed (dice 1); every wave fills its columns' trees (every byte: zeros, child -1), a block barrier,
//            pu_root from boards[m], dice[m]
//   search:  sims + 1 rounds as in k_puct_search; round 0 is the NOISE instance's, on row (ply M + m) of `noise`
//   play:    a block barrier, then pu_play into record row `ply` of game m; boards[m], dice[m], game[m] are updated in place.  A game
//            that is now over, or has reached max_plies, gets zeros in its rows ply + 1 .. max_plies - 1 and leaves its column
//
// The rules of ewn_puct_fused.hip's header, restated for this kernel:
//   Hand-over between lanes.  Per-edge words stay lane-a-only, a board cell of a tree is read by the lane that wrote it.  Every value
//     that travels between lanes through global memory -- the header, a node's dice and parent triple, begin's fill, the board and
//     dice pu_play wrote for the next pu_root, game[m] -- is written and read on ONE wave (a column never changes its wave, a game
//     never its column) and across a block barrier (__syncthreads: a workgroup-scope release and acquire, on one CU and one vector
//     cache): it is read at the earliest in the phase or round after the one that wrote it.  game[m] of a game not yet played is the
//     caller's, read by wave 0 at the refill.
//   Range checks.  Every index read from a tree stays range-checked (pu_round, pu_play).
//   No atomics.  The block's queue is a counter in wave 0's registers.
//   Stores.  Every store is a vector store, in plain C++.
//   Prior contents.  What `scratch` or the record buffers held before the call cannot matter: every byte of a tree is written before
//     any is read, and every record row 0 .. max_plies - 1 of every game is written (rows below the ply a game enters with: zeros).
//   Independence from the layout.  Which column or block plays a game changes no bit of its records: a column's network outputs
//     depend on that column alone, and a game's record on its inputs, key, game_offset + m and its noise rows only.
//
// The table instances, k_puct_selfplay<S, NOISE, true> (C ABI: ewn_puct_selfplay_eg, include/ewn_puct_games_exact.h): a
// ply's search is k_puct_search<S, NOISE, true>'s (ewn_puct_fused.hip), so a game's records are, byte for byte, what
// selfplay_puct(leaf_table=)'s ply loop leaves: per ply ewn_puct_search_eg and ewn_puct_play.  A pending leaf that the table covers is
// worth fl(terminal_value * q) at the first maximum of the six q under a strict >, in place of the value head's output.
//   search, between a round's two barriers: while wave 0 and wave 1 run the networks, waves 2 .. 7 look the block's columns up, column
//            k on wave 2 + k % 6, exactly as k_puct_search's table instances do: the ballot on the slot's non-empty cells against
//            max_total, eg_position, six eg_move on lanes 0 .. 5 with la_find / la_dice, the fold in action order, one rounding;
//            lane 0 writes (exact, covered) of column k into LDS words of the instance's own behind PugGeo<S>'s regions.  After the
//            barrier the tree's wave hands pu_round the exact value's address in place of the value head's where covered.  A column
//            without a game, and a tree without a pending leaf, shows a zero board: no cube, not covered.
//   leaf_counts (may be NULL): per game {rounds the table valued, rounds the value head valued}, summed over the plies played here.
//            Two 32-bit LDS words per column behind the exact values (a game can pass 65 535), zeroed by wave 0 when the column
//            takes a game, added to by lane 0 of the tree's wave every round, and stored by that lane when the column gives its game
//            up; a game that is not played gets two zeros from wave 0 on the zero-rows path.  A column's words are written and read
//            by one lane, but for wave 0's zeros, which a block barrier separates from the rounds.
// Every rule above holds for these instances as it stands: the phases are block-uniform and the barriers stand where they stood; a
// column stays on one wave for the whole launch (a looking-up wave reads the column's slot and dice in LDS, written before the
// round's first barrier, and the table, and touches no tree); the hand-over rule; pu_round's and pu_play's range checks; every byte
// of a tree and of every record row, and every element of leaf_counts, written before it is read; no atomics, vector stores only,
// plain C++.  The table is only read, with indices that eg_move's own arguments keep inside it: the coverage test comes first, and a
// move never adds a cube.  The instance's own arguments (the table, leaf_counts, terminal_value, EgGeo by value) travel in a struct
// at the END of the kernel's arguments, empty in the plain instances, whose LDS, registers and instructions are what they were; the
// larger LDS size has its own static_assert against POL_LDS_MAX.
#include "ewn_puct.hpp"
#include "ewn_endgame.hpp"
#include "../../include/ewn_puct_games_exact.h"

#define PUG_NT 512           // threads per block: eight waves (two per SIMD, up to 256 VGPRs each)
#define PUG_NW (PUG_NT / 64)
#define PUG_TILE 32          // the most columns of a block: the columns of an MFMA tile
#define PUG_MAX_BLOCKS 256   // one block per CU (the two images leave no room for a second)

// LDS of k_puct_selfplay<S, .>: policy image | value image | 32 slots of RecGeo<S>::STR bytes | dice [32] | logits [32][8] | value [32] |
// per wave PU_WAVE bytes | the columns' games int [32] | their plies int [32] | 4 words of the block's own (word 0: a column holds a game)
template <int S> struct PugGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    static constexpr int O_SLOTS = 2 * Mlp3Geo<S>::FWD_BYTES;
    static constexpr int O_DICE = O_SLOTS + PUG_TILE * STR;
    static constexpr int O_LOGITS = O_DICE + PUG_TILE;
    static constexpr int O_VALUE = O_LOGITS + PUG_TILE * 8 * 4;
    static constexpr int O_WAVES = O_VALUE + PUG_TILE * 4;
    static constexpr int O_GAME = O_WAVES + PUG_NW * PU_WAVE;
    static constexpr int O_PLY = O_GAME + PUG_TILE * 4;
    static constexpr int O_CTRL = O_PLY + PUG_TILE * 4;
    static constexpr size_t lds_bytes() { return (size_t)O_CTRL + 16; }
    static_assert(Mlp3Geo<S>::FWD_BYTES % 16 == 0 && STR % 16 == 0 && PU_WAVE % 16 == 0, "every region starts on a 16-byte boundary");
    static_assert(CELLS <= STR, "a slot holds the board");
    static_assert(lds_bytes() <= POL_LDS_MAX, "both weight images + the tile's slots, outputs, the waves' own and the columns' words must fit the CU's LDS");
};

struct PugBuf {
    const float *params; const float *noise; float eps, keep; int8_t *boards; int8_t *dice; int *game;
    PuRecord rec; uint8_t *scratch;                            // rec: rows [max_plies][M], row ply * M + m is game m's ply
};

// the table instances' own arguments; the plain instances carry an empty struct.  Their LDS, behind the plain instances': exact [32]
// floats | covered [32] words | the columns' leaf counts [32][2] words
template <bool EG> struct PugEg {};
template <> struct PugEg<true> { const float *tbl; int *counts; float tv; EgGeo g; };
#define PUG_EG_LDS (4 * PUG_TILE * 4)
#define PUG_NLOOK (PUG_NW - 2)   // the waves that look columns up while waves 0 and 1 run the networks

// zeros into rows t0 .. t1 - 1 of game m, by one wave
template <int CELLS>
EWN_DEV void pug_zero_rows(const PuRecord &R, int M, int m, int t0, int t1, int lane)
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

// tile: the columns of a block, 1 .. PUG_TILE; the grid's blocks share the M games (M >= 1, gridDim.x <= ceil(M / tile))
template <int S, bool NOISE, bool EG = false>
__global__ __launch_bounds__(PUG_NT, 1) void k_puct_selfplay(int M, int sims, int max_plies, int tile, int temp_plies, float c_puct, float inv_tv,
                                                             u32 k0, u32 k1, long long game_offset, PuLayout L, PugBuf B, PugEg<EG> E)
{
    using P = PugGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR;
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wpi = lds, *Wvf = lds + Q3::FWD_BYTES;
    int8_t *slots = lds + P::O_SLOTS, *sdice = lds + P::O_DICE;
    float *slg = (float *)(lds + P::O_LOGITS), *sval = (float *)(lds + P::O_VALUE);
    int *sgame = (int *)(lds + P::O_GAME), *sply = (int *)(lds + P::O_PLY), *ctrl = (int *)(lds + P::O_CTRL);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + P::O_WAVES + wave * PU_WAVE;
    mlp3_pack_fwd<S>(Wpi, B.params, 0, threadIdx.x, PUG_NT);
    mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, PUG_NT);
    if (threadIdx.x < PUG_TILE) sgame[threadIdx.x] = -1;

    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;
    const size_t tree0 = (size_t)blockIdx.x * (size_t)tile;    // the block's first tree of `scratch`
    // the block's set of games: next .. end - 1; `next` is wave 0's alone
    int next = (int)((long long)blockIdx.x * (long long)M / (long long)gridDim.x);
    const int end = (int)(((long long)blockIdx.x + 1) * (long long)M / (long long)gridDim.x);
    const int j = lane & 31, h = lane >> 5;

    #pragma unroll 1
    for (;;) {                                                 // a phase: block-uniform
        __syncthreads();                                       // the images are packed; the last phase's moves are made, its slots read
        if (wave == 0) {                                       // ---- refill
            int held = 0;
            #pragma unroll 1
            for (int k = 0; k < tile; k++) {                   // wave-uniform
                int m = __builtin_amdgcn_readfirstlane(sgame[k]);   // a column's words are the same for every lane
                #pragma unroll 1
                while (m < 0 && next < end) {
                    const int cand = next++;
                    const int *g = B.game + (size_t)cand * 4;
                    const int ply = __builtin_amdgcn_readfirstlane(g[0]), over = __builtin_amdgcn_readfirstlane(g[1]);
                    if (over != 0 || ply < 0 || ply >= max_plies) {   // not played: its rows are zeros
                        pug_zero_rows<CELLS>(B.rec, M, cand, 0, max_plies, lane);
                        if constexpr (EG) {                    // ... and so are its counts
                            if (E.counts && lane < 2) E.counts[2 * (size_t)cand + lane] = 0;
                        }
                        continue;
                    }
                    pug_zero_rows<CELLS>(B.rec, M, cand, 0, ply, lane);
                    m = cand;
                    if (lane == 0) { sgame[k] = cand; sply[k] = ply; }
                    if constexpr (EG) {                        // the column's counts start with its game
                        int *scnt = (int *)(lds + P::lds_bytes()) + 2 * PUG_TILE;
                        if (lane == 0) { scnt[2 * k] = 0; scnt[2 * k + 1] = 0; }
                    }
                }
                held |= m >= 0;
            }
            if (lane == 0) ctrl[0] = held;
        }
        for (int i = threadIdx.x; i < PUG_TILE * STR / 4; i += PUG_NT) ((u32 *)slots)[i] = 0u;
        if (threadIdx.x < PUG_TILE) sdice[threadIdx.x] = 1;
        __syncthreads();                                       // the columns' games and the stop word are there; the slots are zero
        if (__builtin_amdgcn_readfirstlane(ctrl[0]) == 0) break;                               // ---- stop: every wave reads the same word
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUG_NW) {            // ---- begin: the fill of this wave's trees
            if (__builtin_amdgcn_readfirstlane(sgame[k]) < 0) continue;   // wave-uniform
            u32 *t = (u32 *)(B.scratch + (tree0 + (size_t)k) * (size_t)L.bytes);
            #pragma unroll 1
            for (u32 i = lane; i < words; i += 64) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                       // the fill is done before the roots go over it
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUG_NW) {
            const int m0 = __builtin_amdgcn_readfirstlane(sgame[k]);
            if (m0 < 0) continue;
            const size_t m = (size_t)m0;
            pu_root<S>(pu_tree(B.scratch, tree0 + (size_t)k, L), B.boards + m * CELLS, B.dice + m, sims, slots + k * STR, sdice + k, lane, base);
        }
        #pragma unroll 1
        for (int rnd = 0; rnd <= sims; rnd++) {                // ---- search: k_puct_search's round
            __syncthreads();                                   // the leaves are in the slots, the trees' words are handed over
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
            if constexpr (EG) {
                // ---- the lookups, under the networks: column k by wave 2 + k % PUG_NLOOK, all 64 lanes on the one slot (k_puct_search's)
                float *sex = (float *)(lds + P::lds_bytes());
                int *scov = (int *)(sex + PUG_TILE);
                const int w2 = __builtin_amdgcn_readfirstlane(wave) - 2;
                if (w2 >= 0) {                                 // wave-uniform
                    #pragma unroll 1
                    for (int k = w2; k < tile; k += PUG_NLOOK) {
                        const int8_t *leaf = slots + k * STR;
                        // more cubes on the row than a table position has: not covered whatever else (eg_position counts every cell
                        // that is not empty, or refuses the row for a value outside -6 .. 6), and the scan is skipped
                        const int cubes = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < CELLS && leaf[lane < CELLS ? lane : 0] != 0));
                        bool covered = false;                  // wave-uniform: every lane scans the same row
                        float exact = 0.0f;
                        if (cubes <= E.g.T) {
                            int Ma, Mo, na, no;
                            u64 pa, po;
                            covered = __builtin_amdgcn_readfirstlane((int)eg_position<S>(leaf, E.g.K, E.g.T, Ma, Mo, na, no, pa, po)) != 0;
                            if (covered) {
                                float q = -__builtin_inff();
                                if (lane < 6) q = eg_move<S>(E.tbl, E.g, Ma, Mo, pa, po, la_find(lane / 3, la_dice((int)sdice[k]), Ma), lane % 3);
                                float qb = __shfl(q, 0, 64);   // k_endgame_lookup's fold: the first maximum, -0.0 == +0.0
                                #pragma unroll
                                for (int i = 1; i < 6; i++) { const float qi = __shfl(q, i, 64); if (qi > qb) qb = qi; }
                                exact = E.tv * qb;             // one rounding; pu_evaluate forms fl(exact * inv_tv)
                            }
                        }
                        if (lane == 0) { sex[k] = exact; scov[k] = covered ? 1 : 0; }
                    }
                }
            }
            __syncthreads();                                   // logits and value are there; the slots are read
            #pragma unroll 1
            for (int k = wave; k < tile; k += PUG_NW) {
                const int m0 = __builtin_amdgcn_readfirstlane(sgame[k]);
                if (m0 < 0) continue;                          // a column without a game: its slot stays a zero board with dice 1
                PuNoise Z = { nullptr, 0.0f, 0.0f };
                if constexpr (NOISE) Z = PuNoise{ B.noise + ((size_t)__builtin_amdgcn_readfirstlane(sply[k]) * (size_t)M + (size_t)m0) * 6, B.eps, B.keep };
                const PuTree T = pu_tree(B.scratch, tree0 + (size_t)k, L);
                const float *vp = sval + k;
                if constexpr (EG) {                            // a covered column holds a position, so its tree has a pending leaf
                    const float *sex = (const float *)(lds + P::lds_bytes());
                    int *scnt = (int *)(lds + P::lds_bytes()) + 2 * PUG_TILE;
                    const bool covered = __builtin_amdgcn_readfirstlane(((const int *)(sex + PUG_TILE))[k]) != 0;
                    const bool pending = __builtin_amdgcn_readfirstlane(T.hdr[2]) >= 0;
                    if (lane == 0) { scnt[2 * k] += covered ? 1 : 0; scnt[2 * k + 1] += pending && !covered ? 1 : 0; }
                    if (covered) vp = sex + k;
                }
                // the noise instance is round 0's alone: on later rounds the pending node is never the root, and pu_evaluate asks
                pu_round<S, NOISE>(T, sims, c_puct, inv_tv, L.nodes, slg + k * 8, vp, Z, slots + k * STR, sdice + k, lane, base);
            }
        }
        __syncthreads();                                       // ---- play: the last round's header and root are handed over
        #pragma unroll 1
        for (int k = wave; k < tile; k += PUG_NW) {
            const int m0 = __builtin_amdgcn_readfirstlane(sgame[k]);
            if (m0 < 0) continue;
            const size_t m = (size_t)m0;
            const int ply = __builtin_amdgcn_readfirstlane(sply[k]);
            const bool goes_on = pu_play<S>(pu_tree(B.scratch, tree0 + (size_t)k, L), true, sims, L.nodes, B.boards + m * CELLS, B.dice + m,
                                            B.game + m * 4, temp_plies, k0, k1, (unsigned long long)game_offset + (unsigned long long)m, B.rec,
                                            (size_t)ply * (size_t)M + m, lane, base);
            if (goes_on && ply + 1 < max_plies) {
                if (lane == 0) sply[k] = ply + 1;
            } else {                                           // over, or cut at max_plies: the remaining rows, and the column is free
                pug_zero_rows<CELLS>(B.rec, M, m0, ply + 1, max_plies, lane);
                if (lane == 0) sgame[k] = -1;
                if constexpr (EG) {                            // the game's counts: the lane that added to them stores them
                    const int *scnt = (const int *)(lds + P::lds_bytes()) + 2 * PUG_TILE;
                    if (E.counts && lane == 0) { E.counts[2 * m] = scnt[2 * k]; E.counts[2 * m + 1] = scnt[2 * k + 1]; }
                }
            }
        }
    }
}

template <int S, bool NOISE>
static int pug_launch(int M, int sims, int max_plies, int tile, int blocks, int temp_plies, float c_puct, float inv_tv, uint64_t key,
                      int64_t game_offset, const PugBuf &b, hipStream_t s)
{
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_selfplay<S, NOISE>, (unsigned)blocks, PUG_NT, PugGeo<S>::lds_bytes(), 64 * 1024, POL_LDS_MAX, s, M, sims, max_plies,
                             tile, temp_plies, c_puct, inv_tv, (u32)key, (u32)(key >> 32), (long long)game_offset, L, b, PugEg<false>{});
}

template <int S, bool NOISE>
static int pug_launch_eg(int M, int sims, int max_plies, int tile, int blocks, int temp_plies, float c_puct, float inv_tv, uint64_t key,
                         int64_t game_offset, const PugBuf &b, const PugEg<true> &e, hipStream_t s)
{
    constexpr size_t lds = PugGeo<S>::lds_bytes() + PUG_EG_LDS;
    static_assert(PugGeo<S>::lds_bytes() % 4 == 0 && lds <= POL_LDS_MAX, "the plain instance's LDS and the columns' exact values, flags and counts must fit the CU's LDS");
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_selfplay<S, NOISE, true>, (unsigned)blocks, PUG_NT, lds, 64 * 1024, POL_LDS_MAX, s, M, sims, max_plies, tile,
                             temp_plies, c_puct, inv_tv, (u32)key, (u32)(key >> 32), (long long)game_offset, L, b, e);
}

// The library's choice where tile or blocks is 0 (DESIGN.md 4s has the measurements): every CU gets a block, and the columns are as
// few as still hold all M games at once, ceil(M / 256) and at most 32 -- ewn_puct_search's rule: up to 8 192 games every game has a
// column from the start and the tiles are the smallest, beyond that the tiles are full and the columns are refilled
static inline void pug_geometry(int M, int &tile, int &blocks)
{
    if (tile == 0) {
        const int t = (M - 1) / PUG_MAX_BLOCKS + 1;
        tile = t > PUG_TILE ? PUG_TILE : t;
    }
    if (blocks == 0) blocks = PUG_MAX_BLOCKS;
    const int most = (M - 1) / tile + 1;                       // never more blocks than ceil(M / tile)
    if (blocks > most) blocks = most;
}

// pu_refuse, then the range of tile and blocks; M == 0: 0
int64_t ewn_puct_selfplay_scratch_bytes(int board_size, int cube_layer, int M, int sims, int tile, int blocks)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK) return rc;
    if (sims < 0 || sims > PU_MAX_SIMS || tile < 0 || tile > PUG_TILE || blocks < 0 || blocks > PUG_MAX_BLOCKS) return EWN_EINVAL;
    if (M == 0) return 0;
    pug_geometry(M, tile, blocks);
    return pu_layout(board_size, sims).bytes * (long long)tile * (long long)blocks;
}

// ewn_puct_search's order of refusals up to tile and blocks, for both entries; pointers: every pointer that must be given is.
// empty: M == 0, which is EWN_OK before anything else is looked at
static int pug_refuse(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value, bool pointers,
                      const void *scratch, const void *game, int temp_plies, int tile, int blocks, bool &empty)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    empty = rc == EWN_OK && M == 0;
    if (rc != EWN_OK || empty) return rc;
    if (!pointers) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)scratch & 3) || ((uintptr_t)game & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (max_plies < 1 || temp_plies < 0 || tile < 0 || tile > PUG_TILE || blocks < 0 || blocks > PUG_MAX_BLOCKS) return EWN_EINVAL;
    return EWN_OK;
}

// ewn_puct_search's order of refusals, all before the launch; noise_eps is looked at only when noise is given
int ewn_puct_selfplay(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value, const float *params,
                      const float *noise, float noise_eps, int temp_plies, uint64_t key, int64_t game_offset, int tile, int blocks,
                      int8_t *boards, int8_t *dice, int32_t *game, int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value,
                      int8_t *rec_action, int8_t *rec_live, void *scratch, void *stream)
{
    bool empty;
    const int rc = pug_refuse(board_size, cube_layer, M, sims, max_plies, c_puct, terminal_value, params && boards && dice && game && scratch,
                              scratch, game, temp_plies, tile, blocks, empty);
    if (rc != EWN_OK || empty) return rc;
    if (noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    pug_geometry(M, tile, blocks);
    PugBuf b = { params, noise, noise ? noise_eps : 0.0f, noise ? 1.0f - noise_eps : 1.0f, boards, dice, (int *)game,
                 PuRecord{ rec_board, rec_dice, (int *)rec_visits, rec_value, rec_action, rec_live }, (uint8_t *)scratch };
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    if (noise)
        return board_size == 5 ? pug_launch<5, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s)
                               : pug_launch<7, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s);
    return board_size == 5 ? pug_launch<5, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s)
                           : pug_launch<7, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, s);
}

// ewn_puct_selfplay's refusals in its order, the table among the pointers; then the table's values, the alignments; noise_eps last and
// only when noise is given.  The scratch is ewn_puct_selfplay_scratch_bytes': the same trees under the same geometry rule
int ewn_puct_selfplay_eg(int board_size, int cube_layer, int M, int sims, int max_plies, float c_puct, float terminal_value, const float *params,
                         const float *noise, float noise_eps, int temp_plies, uint64_t key, int64_t game_offset, int tile, int blocks,
                         int8_t *boards, int8_t *dice, int32_t *game, int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value,
                         int8_t *rec_action, int8_t *rec_live, void *scratch, int max_cubes, int max_total, const float *table,
                         int32_t *leaf_counts, void *stream)
{
    bool empty;
    const int rc = pug_refuse(board_size, cube_layer, M, sims, max_plies, c_puct, terminal_value,
                              params && boards && dice && game && scratch && table, scratch, game, temp_plies, tile, blocks, empty);
    if (rc != EWN_OK || empty) return rc;
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (((uintptr_t)table & 3) || ((uintptr_t)leaf_counts & 3)) return EWN_EINVAL;
    if (noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    pug_geometry(M, tile, blocks);
    PugBuf b = { params, noise, noise ? noise_eps : 0.0f, noise ? 1.0f - noise_eps : 1.0f, boards, dice, (int *)game,
                 PuRecord{ rec_board, rec_dice, (int *)rec_visits, rec_value, rec_action, rec_live }, (uint8_t *)scratch };
    PugEg<true> e;
    e.tbl = table; e.counts = (int *)leaf_counts; e.tv = terminal_value;
    eg_geo(board_size, max_cubes, max_total, e.g);
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    if (noise)
        return board_size == 5 ? pug_launch_eg<5, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, e, s)
                               : pug_launch_eg<7, true>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, e, s);
    return board_size == 5 ? pug_launch_eg<5, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, e, s)
                           : pug_launch_eg<7, false>(M, sims, max_plies, tile, blocks, temp_plies, c_puct, inv_tv, key, game_offset, b, e, s);
}
