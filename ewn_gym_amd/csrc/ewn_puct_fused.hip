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
#include "ewn_puct.hpp"

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

// tile: the trees per tile, 1 .. PUF_TILE (block-uniform); rounds: R of the contract, 0 .. sims + 1
template <int S, bool NOISE>
__global__ __launch_bounds__(PUF_NT, 1) void k_puct_search(int M, int sims, int rounds, int tile, float c_puct, float inv_tv, PuLayout L, PufBuf B)
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
            __syncthreads();                                   // logits and value are there; the slots are read
            #pragma unroll 1
            for (int k = wave; k < nt; k += PUF_NW) {
                const size_t m = (size_t)(first + k);
                PuNoise Z = { nullptr, 0.0f, 0.0f };
                if constexpr (NOISE) Z = PuNoise{ B.noise + m * 6, B.eps, B.keep };
                // the noise instance is round 0's alone: on later rounds the pending node is never the root, and pu_evaluate asks
                pu_round<S, NOISE>(pu_tree(B.tree, m, L), sims, c_puct, inv_tv, L.nodes, slg + k * 8, sval + k, Z, slots + k * STR, sdice + k, lane, base);
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
                             c_puct, inv_tv, L, b);
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
