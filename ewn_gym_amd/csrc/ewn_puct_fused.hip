// ewn_puct_fused.hip -- the whole PUCT search in one launch, the network inside the tree kernel (C ABI: ewn_puct_search).
// What it leaves in `tree` is, byte for byte, what ewn_puct_begin and then R rounds of ewn_predict_policy on the leaf rows and
// ewn_puct_advance (round 0: ewn_puct_advance_noise, when root noise is given) leave there: the tree code is ewn_puct.hpp's, the
// one copy the staged kernels call, and the network code is ewn_predict_policy's (mlp3_pack_fwd's images, pol_obs_operand on a
// zero-padded slot, mlp3_forward) under the same compiler flags.  No leaf row leaves the kernel: a tree's leaf row IS its column's
// observation slot in LDS, and the five logits and the value come back through LDS.
//
// A block owns a tile of up to 32 trees -- the 32 columns of the MFMA tiles -- for the whole search and walks further tiles
// grid-stride.  Wave w holds the tile's trees w, w + PUF_NW, ... from the fill to the last round.
//   phase 0:   the block packs both forward images ONCE per launch; per tile the slots are zeroed (dice 1), every wave fills its
//              trees (zeros, child -1), a block barrier, every wave writes its trees' roots (pu_root)
//   per round: a block barrier | wave 0 runs the policy net, wave 1 the value net on the tile's 32 slots, logits and value to LDS |
//              a block barrier | every wave runs pu_round on each of its trees: evaluation from LDS, backup, one simulation, the
//              new leaf into the tree's slot (a tree without a new leaf: a zero board with dice 1)
// A column's outputs depend on that column alone, so how many of the 32 columns hold a tree changes no bit; columns without a tree
// are zero boards with dice 1.
//
// Which values travel between lanes through global memory, and how (ewn_puct.hpp's rule, the fused form): a node's dice and parent
// triple and the header are written by lane 0 and read by every lane, and begin's fill is written by lanes other than those that
// later own the words.  A tree never changes its wave, every such value is read at the earliest in the round AFTER the one that
// wrote it, and between two rounds (and between the fill and the roots) lie block barriers: __syncthreads, a workgroup-scope
// release and acquire, on one CU and one vector cache.  Per-edge words stay lane-a-only, a board cell is read by the lane that
// wrote it.  Every index read from the tree is range-checked as in the staged kernels; what `tree` held before the call cannot
// matter, because every byte is written before any is read.  No atomics.
//
// The table instances, k_puct_search<S, NOISE, true> (C ABI: ewn_puct_search_eg, include/ewn_puct_exact.h): a pending
// leaf that an endgame table covers takes its exact value from the table in place of the value head's output; the logits stay the
// policy head's.  Byte for byte the sequence above with EndgameTable.lookup(leaf rows, leaf dice) between ewn_predict_policy and
// ewn_puct_advance: where the lookup says covered, the value handed on is fl(terminal_value * q) at the action the lookup returns,
// the first maximum of the six under a strict > (pu_evaluate then forms fl(that * inv_tv), so the kernel carries terminal_value
// as well as inv_tv); elsewhere the value head's.
//   per round, between the two barriers: while wave 0 and wave 1 run the networks, waves 2 .. 7 look the tile's columns up,
//              column k on wave 2 + k % 6 -- a ballot counts the slot's cubes (more than max_total: not covered, the lookup's test
//              counts the same cells); else every lane scans the slot (eg_position, the lookup's own coverage test, on the CELLS
//              bytes at the slot's start: broadcast reads); covered: lanes 0 .. 5 gather one eg_move each for (f, r) = (lane / 3,
//              lane % 3) with the cube from la_find / la_dice, the six go round the wave by shuffles and are folded in action
//              order; lane 0 writes (exact, covered) of column k into an LDS array of the instance's own, apart from `value`,
//              which wave 1 writes in the same phase.  After the barrier the tree's wave hands pu_round the exact value's address
//              in place of the value head's.  A column without a pending leaf is a zero board: no cube, not covered.
// Every rule above holds for these instances as it stands: the block barriers and their places; a tree -- its bytes in global
// memory -- stays on one wave from the fill to the end (a looking-up wave reads the column's slot and dice in LDS, written before
// the round's first barrier, and the table, and touches no tree); the hand-over rule of ewn_puct.hpp; pu_round's range checks;
// every byte written before any is read; no atomics, vector stores only.  EgGeo travels by value among the kernel's arguments.  The
// table is only read, with indices that eg_move's own argument keeps inside it: the coverage test comes first, and a move never
// adds a cube.  It must be complete before the launch in stream order.  leaf_counts (may be NULL): per tree {rounds the table
// valued, rounds the value head valued}, kept as wave-uniform registers (16 bits per tree of the wave, at most sims + 1 = 4097
// each) and stored once by lane 0 after the round loop.  LDS grows by 256 bytes; the plain instances' LDS, registers and
// instructions are what they were.
#include "ewn_puct.hpp"
#include "ewn_endgame.hpp"
#include "../../include/ewn_puct_exact.h"

#define PUF_NT 512           // threads per block: eight waves (two per SIMD, up to 256 VGPRs each)
#define PUF_NW (PUF_NT / 64)
#define PUF_TILE 32          // the most trees a tile holds: the columns of an MFMA tile
#define PUF_MAX_BLOCKS 256   // one block per CU (the two images leave no room for a second); more tiles are walked grid-stride

// LDS of k_puct_search<S, .>: policy image | value image | 32 slots of RecGeo<S>::STR bytes | dice [32] | logits [32][5] (padded to
// [32][8] floats) | value [32] | per wave PU_WAVE bytes
template <int S> struct PufGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    static constexpr int O_SLOTS = 2 * Mlp3Geo<S>::FWD_BYTES;
    static constexpr int O_DICE = O_SLOTS + PUF_TILE * STR;
    static constexpr int O_LOGITS = O_DICE + PUF_TILE;
    static constexpr int O_VALUE = O_LOGITS + PUF_TILE * 8 * 4;
    static constexpr int O_WAVES = O_VALUE + PUF_TILE * 4;
    static constexpr size_t lds_bytes() { return (size_t)O_WAVES + (size_t)PUF_NW * PU_WAVE; }
    static_assert(Mlp3Geo<S>::FWD_BYTES % 16 == 0 && STR % 16 == 0 && PU_WAVE % 16 == 0, "every region starts on a 16-byte boundary");
    static_assert(CELLS <= STR, "a slot holds the board");
};

struct PufBuf { const int8_t *boards; const int8_t *dice; const float *params; const float *noise; float eps, keep; uint8_t *tree; };

// the table instances' own arguments; the plain instances carry an empty struct.  Their LDS, behind the plain instances': exact [32]
// floats | covered [32] words
template <bool EG> struct PufEg {};
template <> struct PufEg<true> { const float *tbl; int *counts; float tv; EgGeo g; };
#define PUF_EG_LDS (2 * PUF_TILE * 4)
#define PUF_NLOOK (PUF_NW - 2)   // the waves that look columns up while waves 0 and 1 run the networks

// tile: the trees per tile, 1 .. PUF_TILE (block-uniform); rounds: R of the contract, 0 .. sims + 1
template <int S, bool NOISE, bool EG = false>
__global__ __launch_bounds__(PUF_NT, 1) void k_puct_search(int M, int sims, int rounds, int tile, float c_puct, float inv_tv, PuLayout L, PufBuf B,
                                                           PufEg<EG> E)
{
    using P = PufGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR;
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wpi = lds, *Wvf = lds + Q3::FWD_BYTES;
    int8_t *slots = lds + P::O_SLOTS, *sdice = lds + P::O_DICE;
    float *slg = (float *)(lds + P::O_LOGITS), *sval = (float *)(lds + P::O_VALUE);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + P::O_WAVES + wave * PU_WAVE;
    mlp3_pack_fwd<S>(Wpi, B.params, 0, threadIdx.x, PUF_NT);
    mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, PUF_NT);

    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;
    const int tiles = (M - 1) / tile + 1;                      // M >= 1
    const int j = lane & 31, h = lane >> 5;
    #pragma unroll 1
    for (int t0 = (int)blockIdx.x; t0 < tiles; t0 += (int)gridDim.x) {   // block-uniform
        const int first = t0 * tile, nt = min(tile, M - first);         // 1 .. tile trees of this tile exist
        __syncthreads();                                       // the images are packed; the last tile's slots are read
        for (int i = threadIdx.x; i < PUF_TILE * STR / 4; i += PUF_NT) ((u32 *)slots)[i] = 0u;
        if (threadIdx.x < PUF_TILE) sdice[threadIdx.x] = 1;
        #pragma unroll 1
        for (int k = wave; k < nt; k += PUF_NW) {              // wave-uniform: the fill of this wave's trees
            u32 *t = (u32 *)(B.tree + (size_t)(first + k) * (size_t)L.bytes);
            #pragma unroll 1
            for (u32 i = lane; i < words; i += 64) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                       // the fill is done before the roots go over it; the slots are zero
        #pragma unroll 1
        for (int k = wave; k < nt; k += PUF_NW) {
            const size_t m = (size_t)(first + k);
            pu_root<S>(pu_tree(B.tree, m, L), B.boards + m * CELLS, B.dice + m, sims, slots + k * STR, sdice + k, lane, base);
        }
        unsigned long long by_table = 0, by_value = 0;        // EG: 16 bits per tree of this wave, tree k in field k / PUF_NW (wave-uniform)
        #pragma unroll 1
        for (int rnd = 0; rnd < rounds; rnd++) {
            __syncthreads();                                   // the leaves are in the slots, the trees' words are handed over
            // ---- the networks: column j = the tile's tree j, both lane halves; lane (j, h) turns bytes 16 kb + 8 h .. + 7 of slot j into
            // the eight bf16 of its k-block operand (pol_obs_operand)
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
                // ---- the lookups, under the networks: column k by wave 2 + k % PUF_NLOOK, all 64 lanes on the one slot
                float *sex = (float *)(lds + P::lds_bytes());
                int *scov = (int *)(sex + PUF_TILE);
                const int w2 = __builtin_amdgcn_readfirstlane(wave) - 2;
                if (w2 >= 0) {                                 // wave-uniform
                    #pragma unroll 1
                    for (int k = w2; k < nt; k += PUF_NLOOK) {
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
            for (int k = wave; k < nt; k += PUF_NW) {
                const size_t m = (size_t)(first + k);
                PuNoise Z = { nullptr, 0.0f, 0.0f };
                if constexpr (NOISE) Z = PuNoise{ B.noise + m * 6, B.eps, B.keep };
                const PuTree T = pu_tree(B.tree, m, L);
                const float *vp = sval + k;
                if constexpr (EG) {                            // a covered column holds a position, so its tree has a pending leaf
                    const float *sex = (const float *)(lds + P::lds_bytes());
                    const bool covered = __builtin_amdgcn_readfirstlane(((const int *)(sex + PUF_TILE))[k]) != 0;
                    const bool pending = __builtin_amdgcn_readfirstlane(T.hdr[2]) >= 0;
                    const int sh = 16 * (__builtin_amdgcn_readfirstlane(k) / PUF_NW);
                    by_table += (unsigned long long)(covered ? 1 : 0) << sh;
                    by_value += (unsigned long long)(pending && !covered ? 1 : 0) << sh;
                    if (covered) vp = sex + k;
                }
                // the noise instance is round 0's alone: on later rounds the pending node is never the root, and pu_evaluate asks
                pu_round<S, NOISE>(T, sims, c_puct, inv_tv, L.nodes, slg + k * 8, vp, Z, slots + k * STR, sdice + k, lane, base);
            }
        }
        if constexpr (EG) {
            if (E.counts && lane == 0) {
                #pragma unroll 1
                for (int k = wave; k < nt; k += PUF_NW) {
                    const int sh = 16 * (k / PUF_NW);
                    E.counts[2 * (size_t)(first + k)] = (int)((by_table >> sh) & 0xFFFFull);
                    E.counts[2 * (size_t)(first + k) + 1] = (int)((by_value >> sh) & 0xFFFFull);
                }
            }
        }
    }
}

template <int S, bool NOISE>
static int puf_launch(int M, int sims, int rounds, int tile, float c_puct, float inv_tv, const PufBuf &b, hipStream_t s)
{
    constexpr size_t lds = PufGeo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "both weight images + the tile's slots, outputs and the waves' own must fit the CU's LDS");
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_search<S, NOISE>, la_blocks(M, tile, PUF_MAX_BLOCKS), PUF_NT, lds, 64 * 1024, POL_LDS_MAX, s, M, sims, rounds, tile,
                             c_puct, inv_tv, L, b, PufEg<false>{});
}

template <int S, bool NOISE>
static int puf_launch_eg(int M, int sims, int rounds, int tile, unsigned blocks, float c_puct, float inv_tv, const PufBuf &b, const PufEg<true> &e,
                         hipStream_t s)
{
    constexpr size_t lds = PufGeo<S>::lds_bytes() + PUF_EG_LDS;
    static_assert(lds <= POL_LDS_MAX, "the plain instance's LDS and the columns' exact values and flags must fit the CU's LDS");
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_search<S, NOISE, true>, blocks, PUF_NT, lds, 64 * 1024, POL_LDS_MAX, s, M, sims, rounds, tile, c_puct, inv_tv, L,
                             b, e);
}

// Trees per tile.  The networks cost a round the same whatever the tile holds, and a wave walks its trees one after the other, so
// the tiles are as small as still gives every CU at most one: ceil(M / PUF_MAX_BLOCKS), at most 32 (DESIGN.md 4r has the
// measurements).  EWN_PUCT_TILE (1 .. 32) overrides it (tuning, and the tests' way to full tiles at small M); the result does not
// depend on it.
static inline int puf_tile(int M)
{
    const char *e = getenv("EWN_PUCT_TILE");
    const int forced = e ? atoi(e) : 0;
    if (forced >= 1 && forced <= PUF_TILE) return forced;
    const int t = (M - 1) / PUF_MAX_BLOCKS + 1;
    return t < PUF_TILE ? t : PUF_TILE;
}

// ewn_puct_advance_noise's order of refusals, all before the launch; noise_eps is looked at only when root_noise is given
int ewn_puct_search(int board_size, int cube_layer, int M, int sims, int rounds, float c_puct, float terminal_value, const int8_t *boards,
                    const int8_t *dice, const float *params, const float *root_noise, float noise_eps, void *tree, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !params || !tree) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)tree & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (root_noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    const int R = rounds < 0 || rounds > sims + 1 ? sims + 1 : rounds;
    PufBuf b = { boards, dice, params, root_noise, root_noise ? noise_eps : 0.0f, root_noise ? 1.0f - noise_eps : 1.0f, (uint8_t *)tree };
    const float inv_tv = 1.0f / terminal_value;
    const int tile = puf_tile(M);
    hipStream_t s = (hipStream_t)stream;
    if (root_noise)
        return board_size == 5 ? puf_launch<5, true>(M, sims, R, tile, c_puct, inv_tv, b, s) : puf_launch<7, true>(M, sims, R, tile, c_puct, inv_tv, b, s);
    return board_size == 5 ? puf_launch<5, false>(M, sims, R, tile, c_puct, inv_tv, b, s) : puf_launch<7, false>(M, sims, R, tile, c_puct, inv_tv, b, s);
}

// ewn_puct_search's refusals in its order, the table among the pointers; then tile and blocks, the table's values, the alignments.
// No environment variable is read: tile and blocks are arguments, 0 the library's choice
int ewn_puct_search_eg(int board_size, int cube_layer, int M, int sims, int rounds, float c_puct, float terminal_value, const int8_t *boards,
                       const int8_t *dice, const float *params, const float *root_noise, float noise_eps, int tile, int blocks, int max_cubes,
                       int max_total, const float *table, void *tree, int32_t *leaf_counts, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !params || !tree || !table) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)tree & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (root_noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    if (tile < 0 || tile > PUF_TILE || blocks < 0 || blocks > EWN_PUCT_EXACT_MAX_BLOCKS) return EWN_EINVAL;
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (((uintptr_t)table & 3) || ((uintptr_t)leaf_counts & 3)) return EWN_EINVAL;
    const int R = rounds < 0 || rounds > sims + 1 ? sims + 1 : rounds;
    if (tile == 0) {                                           // as small as still gives every CU at most one tile
        tile = (M - 1) / PUF_MAX_BLOCKS + 1;
        tile = tile < PUF_TILE ? tile : PUF_TILE;
    }
    const unsigned need = la_blocks(M, tile, PUF_MAX_BLOCKS);
    const unsigned nb = blocks == 0 || (unsigned)blocks > need ? need : (unsigned)blocks;
    PufBuf b = { boards, dice, params, root_noise, root_noise ? noise_eps : 0.0f, root_noise ? 1.0f - noise_eps : 1.0f, (uint8_t *)tree };
    PufEg<true> e;
    e.tbl = table; e.counts = leaf_counts; e.tv = terminal_value;
    eg_geo(board_size, max_cubes, max_total, e.g);
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    if (root_noise)
        return board_size == 5 ? puf_launch_eg<5, true>(M, sims, R, tile, nb, c_puct, inv_tv, b, e, s)
                               : puf_launch_eg<7, true>(M, sims, R, tile, nb, c_puct, inv_tv, b, e, s);
    return board_size == 5 ? puf_launch_eg<5, false>(M, sims, R, tile, nb, c_puct, inv_tv, b, e, s)
                           : puf_launch_eg<7, false>(M, sims, R, tile, nb, c_puct, inv_tv, b, e, s);
}
