// ewn_puct.hip -- a PUCT search on the trained actor-critic as tree kernels (C ABI: ewn_puct_tree_bytes, ewn_puct_begin,
// ewn_puct_advance, ewn_puct_result).  The staged shape of 4l: begin lays M trees out and hands their roots over as
// observations, the caller evaluates a row per tree with ewn_predict_policy, advance folds that evaluation into the tree (priors,
// backup) and walks one more simulation down to the next observation to evaluate, result reads the root.  No network runs here and
// no random number enters: the chance nodes are a stratified sample of the dice (the least visited dice first).
// Self-play on these trees (ewn_puct_advance_noise, ewn_puct_play): a second instance of advance mixes the caller's
// weights into the root's priors, and play takes a game's move off its finished tree -- the only kernel here that draws (Philox).
//
// A wave per tree.  The layout and the tree code (root, evaluation, walk, backup) are ewn_puct.hpp's, shared with the one-launch
// search of ewn_puct_fused.hip; its header states which values travel between lanes through global memory and how.  Here every
// such value is written one launch before it is read.
#include "ewn_puct.hpp"

#define PU_NT 256            // threads per block: four waves, one tree each per trip
#define PU_MAX_BLOCKS 1024   // more trees are walked grid-stride

struct PuBeginBuf { const int8_t *boards; const int8_t *dice; uint8_t *tree; int8_t *leaf_boards; int8_t *leaf_dice; };
struct PuAdvanceBuf { uint8_t *tree; const float *logits; const float *value; int8_t *leaf_boards; int8_t *leaf_dice; };
struct PuResultBuf { uint8_t *tree; int8_t *actions; int *visits; float *q; float *value; };
// the noise instance's buffers: PuAdvanceBuf first, so that the plain instance's kernel arguments are what they were
struct PuNoiseBuf : PuAdvanceBuf { const float *noise; float eps, keep; };   // noise [M][6]; keep = 1 - eps, formed once on the host
template <bool NOISE> struct PuAdvanceArg { typedef PuAdvanceBuf type; };
template <> struct PuAdvanceArg<true> { typedef PuNoiseBuf type; };
struct PuPlayBuf {
    const uint8_t *tree; int8_t *boards; int8_t *dice; int *game;
    int8_t *rec_board; int8_t *rec_dice; int *rec_visits; float *rec_value; int8_t *rec_action; int8_t *rec_live;
};

// A block per tree: every byte of the tree (zeros, child -1), then wave 0 writes the header, the root and the leaf row (pu_root)
template <int S>
__global__ __launch_bounds__(PU_NT) void k_puct_begin(int M, int sims, PuLayout L, PuBeginBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[PU_WAVE];
    const int lane = threadIdx.x & 63;
    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x; m0 < M; m0 += (int)gridDim.x) {   // block-uniform
        const size_t m = (size_t)m0;
        u32 *t = (u32 *)(B.tree + m * (size_t)L.bytes);
        #pragma unroll 1
        for (u32 i = threadIdx.x; i < words; i += PU_NT) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        __syncthreads();                                       // the fill is done before the root goes over it
        if (threadIdx.x < 64)
            pu_root<S>(pu_tree(B.tree, m, L), B.boards + m * CELLS, B.dice + m, sims, B.leaf_boards + m * CELLS, B.leaf_dice + m, lane, lds);
        __syncthreads();                                       // the LDS is read: the next trip may overwrite it
    }
}

// NOISE (ewn_puct_advance_noise): the noise instance of pu_round, a wave per tree and trip
template <int S, bool NOISE>
__global__ __launch_bounds__(PU_NT) void k_puct_advance(int M, int sims, float c_puct, float inv_tv, PuLayout L, typename PuAdvanceArg<NOISE>::type B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(PU_NT / 64) * PU_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * PU_WAVE;

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        PuNoise Z = { nullptr, 0.0f, 0.0f };
        if constexpr (NOISE) Z = PuNoise{ B.noise + m * 6, B.eps, B.keep };
        pu_round<S, NOISE>(pu_tree(B.tree, m, L), sims, c_puct, inv_tv, L.nodes, B.logits + m * 5, B.value + m, Z, B.leaf_boards + m * CELLS,
                           B.leaf_dice + m, lane, base);
    }
}

// The root's picture.  The budget (and with it the tree's size) is read from the first tree's header: begin wrote it
__global__ __launch_bounds__(PU_NT) void k_puct_result(int S, int M, PuResultBuf B)
{
    __shared__ __attribute__((aligned(16))) float lds[(PU_NT / 64) * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *sw = lds + wave * 16;
    int *sn = (int *)sw + 8;
    const float inf = __builtin_inff();
    const int sims = ((const int *)B.tree)[4];
    const bool known = sims >= 0 && sims <= PU_MAX_SIMS && ((const int *)B.tree)[5] == PU_LAYOUT;
    const PuLayout L = pu_layout(S, known ? sims : 0);

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        int kd = 0, nn = 0;
        float ww = 0.0f;
        if (known) {
            const PuTree T = pu_tree(B.tree, m, L);
            if (T.hdr[3] == 0 && T.hdr[4] == sims && lane < 6) { kd = T.kind[lane]; nn = T.n[lane]; ww = T.w[lane]; }
        }
        if (lane < 8) { sw[lane] = ww; sn[lane] = nn; }
        const u32 wins = (u32)__builtin_amdgcn_ballot_w64(kd == 1) & 0x3Fu, searched = (u32)__builtin_amdgcn_ballot_w64(kd == 2) & 0x3Fu;
        __builtin_amdgcn_wave_barrier();
        if (lane < 6) {
            if (B.visits) B.visits[m * 6 + lane] = nn;
            if (B.q) B.q[m * 6 + lane] = kd == 0 ? -inf : kd == 1 ? 1.0f : nn > 0 ? ww / (float)nn : 0.0f;
        }
        if (lane == 0) {
            const float tw = ((((sw[0] + sw[1]) + sw[2]) + sw[3]) + sw[4]) + sw[5];
            const int tn = sn[0] + sn[1] + sn[2] + sn[3] + sn[4] + sn[5];
            if (B.value) B.value[m] = tn > 0 ? tw / (float)tn : 0.0f;
            int best = 0;
            if (wins) best = __builtin_ctz(wins);              // a win on the board is played
            else if (searched) {
                best = __builtin_ctz(searched);
                int nb = sn[best];
                #pragma unroll
                for (int i = 1; i < 6; i++) if (((searched >> i) & 1u) && sn[i] > nb) { nb = sn[i]; best = i; }
            }
            B.actions[m * 2] = (int8_t)(best / 3); B.actions[m * 2 + 1] = (int8_t)(best % 3);
        }
        __builtin_amdgcn_wave_barrier();                       // this trip's LDS is read: the next may overwrite it
    }
}

// The move of a self-play game off a finished tree (ewn_puct_play): a wave per game and trip around ewn_puct.hpp's
// pu_play, the one copy that the whole-game kernel of ewn_puct_games.hip calls as well.  The budget is read from the first tree's header
template <int S>
__global__ __launch_bounds__(PU_NT) void k_puct_play(int M, int temp_plies, u32 k0, u32 k1, long long game_offset, PuPlayBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(PU_NT / 64) * PU_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * PU_WAVE;
    const int sims = ((const int *)B.tree)[4];
    const bool known = sims >= 0 && sims <= PU_MAX_SIMS && ((const int *)B.tree)[5] == PU_LAYOUT;
    const PuLayout L = pu_layout(S, known ? sims : 0);
    const PuRecord R = { B.rec_board, B.rec_dice, B.rec_visits, B.rec_value, B.rec_action, B.rec_live };

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        pu_play<S>(pu_tree((uint8_t *)B.tree, m, L), known, sims, L.nodes, B.boards + m * CELLS, B.dice + m, B.game + m * 4, temp_plies, k0, k1,
                   (unsigned long long)game_offset + (unsigned long long)m, R, m, lane, base);   // the tree is read only
    }
}

int64_t ewn_puct_tree_bytes(int board_size, int cube_layer, int sims)
{
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (sims < 0 || sims > PU_MAX_SIMS) return EWN_EINVAL;
    return pu_layout(board_size, sims).bytes;
}

int ewn_puct_begin(int board_size, int cube_layer, int M, int sims, const int8_t *boards, const int8_t *dice, void *tree,
                   int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !tree || !leaf_boards || !leaf_dice) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)tree & 3)) return EWN_EINVAL;
    const PuLayout L = pu_layout(board_size, sims);
    PuBeginBuf b = { boards, dice, (uint8_t *)tree, leaf_boards, leaf_dice };
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, 1, PU_MAX_BLOCKS);
    return board_size == 5 ? pol_launch_kernel(k_puct_begin<5>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, L, b)
                           : pol_launch_kernel(k_puct_begin<7>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, L, b);
}

// both advance entry points: the refusals in one order, `missing` says whether a pointer of the caller's own is NULL
template <bool NOISE>
static int pu_advance(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, bool missing, float noise_eps,
                      typename PuAdvanceArg<NOISE>::type b, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (missing || !b.tree || !b.logits || !b.value || !b.leaf_boards || !b.leaf_dice) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)b.tree & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (!(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    const PuLayout L = pu_layout(board_size, sims);
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS);
    return board_size == 5 ? pol_launch_kernel(k_puct_advance<5, NOISE>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, c_puct, inv_tv, L, b)
                           : pol_launch_kernel(k_puct_advance<7, NOISE>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, c_puct, inv_tv, L, b);
}

int ewn_puct_advance(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                     const float *logits, const float *value, int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    PuAdvanceBuf b = { (uint8_t *)tree, logits, value, leaf_boards, leaf_dice };
    return pu_advance<false>(board_size, cube_layer, M, sims, c_puct, terminal_value, false, 0.0f, b, stream);
}

int ewn_puct_advance_noise(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                           const float *logits, const float *value, const float *root_noise, float noise_eps,
                           int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    PuNoiseBuf b;
    b.tree = (uint8_t *)tree; b.logits = logits; b.value = value; b.leaf_boards = leaf_boards; b.leaf_dice = leaf_dice;
    b.noise = root_noise; b.eps = noise_eps; b.keep = 1.0f - noise_eps;
    return pu_advance<true>(board_size, cube_layer, M, sims, c_puct, terminal_value, root_noise == nullptr, noise_eps, b, stream);
}

int ewn_puct_result(int board_size, int cube_layer, int M, const void *tree, int8_t *actions, int32_t *visits, float *q, float *value,
                    void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!tree || !actions) return EWN_ENULL;
    if ((uintptr_t)tree & 3) return EWN_EINVAL;
    PuResultBuf b = { (uint8_t *)tree, actions, visits, q, value };
    return pol_launch_kernel(k_puct_result, la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS), PU_NT, 0, 64 * 1024, POL_LDS_MAX, (hipStream_t)stream, board_size, M, b);
}

int ewn_puct_play(int board_size, int cube_layer, int M, const void *tree, int8_t *boards, int8_t *dice, int32_t *game,
                  int temp_plies, uint64_t key, int64_t game_offset,
                  int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
                  void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!tree || !boards || !dice || !game) return EWN_ENULL;
    if (temp_plies < 0 || ((uintptr_t)tree & 3) || ((uintptr_t)game & 3)) return EWN_EINVAL;
    PuPlayBuf b = { (const uint8_t *)tree, boards, dice, (int *)game, rec_board, rec_dice, (int *)rec_visits, rec_value, rec_action, rec_live };
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS);
    const u32 k0 = (u32)key, k1 = (u32)(key >> 32);
    return board_size == 5 ? pol_launch_kernel(k_puct_play<5>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, temp_plies, k0, k1, (long long)game_offset, b)
                           : pol_launch_kernel(k_puct_play<7>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, temp_plies, k0, k1, (long long)game_offset, b);
}
