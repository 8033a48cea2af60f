// ewn_puct_wide.hip -- the PUCT search in one launch with up to L leaves per tree and round (C ABI: ewn_puct_search_wide,
// ewn_puct_search_wide_scratch_bytes; include/ewn_puct_wide.h).  A round of k_puct_search (ewn_puct_fused.hip) costs the
// two network passes over a 32-column tile whatever the tile holds; here a tree has L of the columns, and a round evaluates up to
// L of its leaves and collects up to L more under a virtual loss of one visit and one lost value per leaf in flight
// (ewn_puct_wide.hpp).  With L = 1 no mark is ever seen by a walk, and every byte of every tree is ewn_puct_search's.
//
// The structure is k_puct_search's: 512 threads, one block per CU, both forward images packed once per launch, 32 observation
// slots, logits and values in LDS, wave 0 runs the policy net and wave 1 the value net per round, block barriers round them.  A
// tile holds `tile` trees of L columns each, tile * L <= 32; tree k stays on wave k % PWD_NW from the fill to the end, and its
// i-th leaf of a round is column k * L + i.  Columns without a leaf are zero boards with dice 1; a column's outputs depend on that
// column alone, so neither the tile, the grid nor the wave changes a bit.
//   per round: the block barrier, at which the block learns whether any tree of the tile still has a pending node or simulations
//              left (one LDS word per wave; the loop ends block-uniformly, and after sims + 1 rounds at the latest) | the networks |
//              a block barrier | every wave, per tree: (A) the pending nodes in ascending order -- marks off along the parent
//              chain, pu_evaluate on the column's logits and value -- then (B) walks until L leaves are collected, the budget is
//              begun or a walk collides (pw_walk)
// Pending nodes are the nodes created in the last walk half, consecutive indices: hdr[2] holds the first while the search runs.
//
// Between lanes (ewn_puct.hpp's rule, the fused form): marks are per-edge words of lane a alone; the evaluate half reads boards,
// dice, parent triples and the header that other lanes wrote in the previous walk half, with the barriers round the networks in
// between; a walk half reads no such value of its own half (ewn_puct_wide.hpp).  Every index read from a tree is range-checked,
// every byte of `tree` and every mark is written before it is read.  No atomics.
#include "ewn_puct_wide.hpp"
#include "../../include/ewn_puct_wide.h"

#define PWD_NT 512           // threads per block: eight waves
#define PWD_NW (PWD_NT / 64)
#define PWD_COLS 32          // the columns of an MFMA tile
#define PWD_MAX_BLOCKS 256   // one block per CU (the two images leave no room for a second); more tiles are walked grid-stride

// LDS of k_puct_search_wide<S, .>: k_puct_search's -- policy image | value image | 32 slots of RecGeo<S>::STR bytes | dice [32] |
// logits [32][8] floats | value [32] | per wave PU_WAVE bytes -- and a word per wave: has a tree of mine work left
template <int S> struct PwdGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    static constexpr int O_SLOTS = 2 * Mlp3Geo<S>::FWD_BYTES;
    static constexpr int O_DICE = O_SLOTS + PWD_COLS * STR;
    static constexpr int O_LOGITS = O_DICE + PWD_COLS;
    static constexpr int O_VALUE = O_LOGITS + PWD_COLS * 8 * 4;
    static constexpr int O_MORE = O_VALUE + PWD_COLS * 4;
    static constexpr int O_WAVES = O_MORE + 16 * 4;
    static constexpr size_t lds_bytes() { return (size_t)O_WAVES + (size_t)PWD_NW * PU_WAVE; }
    static_assert(Mlp3Geo<S>::FWD_BYTES % 16 == 0 && STR % 16 == 0 && PU_WAVE % 16 == 0, "every region starts on a 16-byte boundary");
    static_assert(CELLS <= STR && PWD_NW <= 16, "a slot holds the board; a word per wave");
};

struct PwdBuf { const int8_t *boards; const int8_t *dice; const float *params; const float *noise; float eps, keep; uint8_t *tree; uint8_t *marks; };

// One round of one tree, by one wave.  slots / sdice / slg / sval: the tree's first column.  Returns whether the tree has a pending
// node or simulations left
template <int S, bool NOISE>
EWN_DEV bool pwd_round(const PuTree &T, const PwMarks &V, int sims, int leaves, float c_puct, float inv_tv, int nodes, const float *slg,
                       const float *sval, const PuNoise &Z, int8_t *slots, int8_t *sdice, int lane, int8_t *base)
{
    constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    int count = T.hdr[0], done = T.hdr[1];
    const int first = T.hdr[2];                                // the first pending node: they are first .. count - 1
    const bool ok = T.hdr[3] == 0 && T.hdr[4] == sims && T.hdr[5] == PU_LAYOUT && count >= 1 && count <= nodes && first < count &&
                    (first < 0 || count - first <= leaves) && done >= 0;
    int collected = 0;
    if (ok) {
        if (first >= 0) {                                      // ---- (A) the pending nodes, in ascending order
            #pragma unroll 1
            for (int i = 0; i < count - first; i++) {
                pw_unmark(T, V, first + i, lane, nodes);
                pu_evaluate<S, NOISE>(T, first + i, slg + i * 8, sval + i, inv_tv, Z, nodes, lane, base);
            }
        }
        const int count0 = count;                              // ---- (B) walks
        #pragma unroll 1
        while (collected < leaves && done < sims) {
            const int r = pw_walk<S>(T, V, count, count0, nodes, c_puct, slots + collected * STR, sdice + collected, lane, base);
            if (r == PW_COLLISION) break;
            done++;
            collected += r == PW_LEAF;
        }
        if (lane == 0) { T.hdr[0] = count; T.hdr[1] = done; T.hdr[2] = collected > 0 ? count0 : -1; }
    }
    #pragma unroll 1
    for (int i = collected; i < leaves; i++) {                 // the tree's other columns: zero boards with dice 1
        if (lane < CELLS) slots[i * STR + lane] = 0;
        if (lane == 0) sdice[i] = 1;
    }
    __builtin_amdgcn_wave_barrier();                           // this trip's LDS is read: the next may overwrite it
    return ok && (collected > 0 || done < sims);
}

// tile: the trees per tile, tile * leaves <= PWD_COLS (block-uniform)
template <int S, bool NOISE>
__global__ __launch_bounds__(PWD_NT, 1) void k_puct_search_wide(int M, int sims, int leaves, int tile, float c_puct, float inv_tv, PuLayout L, PwdBuf B)
{
    using P = PwdGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR;
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wpi = lds, *Wvf = lds + Q3::FWD_BYTES;
    int8_t *slots = lds + P::O_SLOTS, *sdice = lds + P::O_DICE;
    float *slg = (float *)(lds + P::O_LOGITS), *sval = (float *)(lds + P::O_VALUE);
    int *smore = (int *)(lds + P::O_MORE);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + P::O_WAVES + wave * PU_WAVE;
    mlp3_pack_fwd<S>(Wpi, B.params, 0, threadIdx.x, PWD_NT);
    mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, PWD_NT);

    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;
    const int tiles = (M - 1) / tile + 1;                      // M >= 1
    const int j = lane & 31, h = lane >> 5;
    #pragma unroll 1
    for (int t0 = (int)blockIdx.x; t0 < tiles; t0 += (int)gridDim.x) {   // block-uniform
        const int first = t0 * tile, nt = min(tile, M - first);         // 1 .. tile trees of this tile exist
        __syncthreads();                                       // the images are packed; the last tile's slots and words are read
        for (int i = threadIdx.x; i < PWD_COLS * STR / 4; i += PWD_NT) ((u32 *)slots)[i] = 0u;
        if (threadIdx.x < PWD_COLS) sdice[threadIdx.x] = 1;
        #pragma unroll 1
        for (int k = wave; k < nt; k += PWD_NW) {              // wave-uniform: the fill of this wave's trees
            u32 *t = (u32 *)(B.tree + (size_t)(first + k) * (size_t)L.bytes);
            #pragma unroll 1
            for (u32 i = lane; i < words; i += 64) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                       // the fill is done before the roots go over it; the slots are zero
        #pragma unroll 1
        for (int k = wave; k < nt; k += PWD_NW) {
            const size_t m = (size_t)(first + k);
            pu_root<S>(pu_tree(B.tree, m, L), B.boards + m * CELLS, B.dice + m, sims, slots + k * leaves * STR, sdice + k * leaves, lane, base);
            pw_clear(pw_marks(B.marks, m, L.nodes), 0, lane);
        }
        bool more = wave < nt;                                 // wave-uniform: round 0 looks at every tree
        if (lane == 0) smore[wave] = more;
        #pragma unroll 1
        for (int rnd = 0; rnd <= sims; rnd++) {                // sims + 1 rounds finish any tree
            __syncthreads();                                   // the leaves are in the slots, the trees' words are handed over
            int any = 0;
            #pragma unroll
            for (int w = 0; w < PWD_NW; w++) any |= smore[w];
            if (!any) break;                                   // block-uniform: every wave read the same eight words
            // ---- the networks: column j, both lane halves; lane (j, h) turns bytes 16 kb + 8 h .. + 7 of slot j into the eight bf16 of
            // its k-block operand (pol_obs_operand)
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
            __syncthreads();                                   // logits and value are there; the slots and the waves' words are read
            more = false;
            #pragma unroll 1
            for (int k = wave; k < nt; k += PWD_NW) {
                const size_t m = (size_t)(first + k);
                PuNoise Z = { nullptr, 0.0f, 0.0f };
                if constexpr (NOISE) Z = PuNoise{ B.noise + m * 6, B.eps, B.keep };
                const int col = k * leaves;
                more |= pwd_round<S, NOISE>(pu_tree(B.tree, m, L), pw_marks(B.marks, m, L.nodes), sims, leaves, c_puct, inv_tv, L.nodes, slg + col * 8,
                                            sval + col, Z, slots + col * STR, sdice + col, lane, base);
            }
            if (lane == 0) smore[wave] = more;
        }
    }
}

template <int S, bool NOISE>
static int pwd_launch(int M, int sims, int leaves, int tile, unsigned blocks, float c_puct, float inv_tv, const PwdBuf &b, hipStream_t s)
{
    constexpr size_t lds = PwdGeo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "both weight images + the tile's slots, outputs and the waves' own must fit the CU's LDS");
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_puct_search_wide<S, NOISE>, blocks, PWD_NT, lds, 64 * 1024, POL_LDS_MAX, s, M, sims, leaves, tile, c_puct, inv_tv, L, b);
}

int64_t ewn_puct_search_wide_scratch_bytes(int board_size, int cube_layer, int M, int sims)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK) return rc;
    if (sims < 0 || sims > PU_MAX_SIMS) return EWN_EINVAL;
    return (long long)M * PW_NODE_BYTES * (long long)(sims + 1);
}

// ewn_puct_search's order of refusals, then leaves, tile and blocks, all before the launch; noise_eps last and only with root_noise
int ewn_puct_search_wide(int board_size, int cube_layer, int M, int sims, int leaves, float c_puct, float terminal_value, const int8_t *boards,
                         const int8_t *dice, const float *params, const float *root_noise, float noise_eps, int tile, int blocks, void *tree,
                         void *scratch, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !params || !tree || !scratch) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)tree & 3) || ((uintptr_t)scratch & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (leaves < 1 || leaves > PW_MAX_LEAVES) return EWN_EINVAL;
    const int most = PWD_COLS / leaves;                        // the trees a tile has room for
    if (tile < 0 || tile > most || blocks < 0 || blocks > PWD_MAX_BLOCKS) return EWN_EINVAL;
    if (root_noise && !(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    if (tile == 0) {                                           // as small as still gives every CU at most one tile
        tile = (M - 1) / PWD_MAX_BLOCKS + 1;
        tile = tile < most ? tile : most;
    }
    const unsigned need = la_blocks(M, tile, PWD_MAX_BLOCKS);
    const unsigned nb = blocks == 0 || (unsigned)blocks > need ? need : (unsigned)blocks;
    PwdBuf b = { boards, dice, params, root_noise, root_noise ? noise_eps : 0.0f, root_noise ? 1.0f - noise_eps : 1.0f, (uint8_t *)tree,
                 (uint8_t *)scratch };
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    if (root_noise)
        return board_size == 5 ? pwd_launch<5, true>(M, sims, leaves, tile, nb, c_puct, inv_tv, b, s)
                               : pwd_launch<7, true>(M, sims, leaves, tile, nb, c_puct, inv_tv, b, s);
    return board_size == 5 ? pwd_launch<5, false>(M, sims, leaves, tile, nb, c_puct, inv_tv, b, s)
                           : pwd_launch<7, false>(M, sims, leaves, tile, nb, c_puct, inv_tv, b, s);
}
