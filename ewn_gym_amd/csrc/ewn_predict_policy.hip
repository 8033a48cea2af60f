// ewn_predict_policy.hip -- the trained actor-critic as a stateless batched policy (C ABI: ewn_predict_policy), the member of the
// ewn_predict_* family that the reference's `model.predict(obs, deterministic=True)` (train.py:89, eval_A2C.py) maps to: M boards and
// M dice in, M actions (and optionally the logits and the value) out, no env behind it.  The arithmetic is the rollout kernel's
// (k_rollout_mlp, ewn_policy_body.inc): the same LDS weight images (mlp3_pack_fwd), the same feature operands out of zero-padded
// per-sample slots (pol_obs_operand), the same mlp3_forward, the same noise and pick (pol_gumbel, pol_pick_flag / pol_pick_dir) -- so a
// recorded rollout step replayed here gives the recorded logits, value and action bit for bit.
//
// Sampling (deterministic == 0): action = Gumbel-max of z[i] = logit[i] + g[i], g[i] = -ln(-ln u[i]) on pol_log, i = 0 .. 4.
//   uniforms given:  u[i] = uniforms[m][i] as it is (a rollout's recorded ewn_policy.noise replays its actions)
//   otherwise:       u[i] = pol_uniform(w, i),  w = fmix32(agent_hash(0, 0, id, key) ^ PRED_POL_SALT),  id = obs_id ? obs_id[m] : m
// i.e. w = fmix32(fmix32(fmix32(id) ^ fmix32((u32)key ^ 'AGNT') ^ (u32)(key >> 32) * 0x85ebca6b) ^ 'PRED') and
// u[i] = ((fmix32(w + (i + 1) * 0x9E3779B9) >> 9) + 0.5) / 2^23: a pure function of (key, id), whatever M, the tiling or the order.
#include "ewn_policy_host.hpp"

#define PRED_POL_SALT 0x50524544u   // 'PRED': the salt of this call's noise word; no other user of `key` hashes with it
#define PRED_NT 256                  // threads per block: four waves, one 32-observation tile each per trip
#define PRED_MAX_BLOCKS 256          // one block per CU (A2C_MAX_BLOCKS' reasoning); more tiles than that are walked grid-stride

// LDS of k_predict_mlp<S, .>: weight image(s) | per wave 32 slots of RecGeo<S>::STR bytes | per wave the tile's packed boards (+ 16:
// the slot builder reads whole dwords, the last of them up to 7 bytes past the last board)
template <int S> struct PredGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR, NW = PRED_NT / 64;
    static constexpr int STAGE = 32 * CELLS + 16;
    static_assert((32 * CELLS) % 16 == 0 && STAGE % 16 == 0, "a tile's boards start on a 16-byte boundary of the boards array");
    static_assert(CELLS % 4 == 1, "the slot builder's mask of the word that holds the last cell");
    static constexpr size_t lds_bytes(bool want_value)
    {
        return (size_t)(want_value ? 2 : 1) * Mlp3Geo<S>::FWD_BYTES + (size_t)NW * 32 * STR + (size_t)NW * STAGE;
    }
};

struct PredBuf {
    const int8_t *boards; const int8_t *dice; const float *params; const u32 *obs_id; const float *uniforms;
    int8_t *actions; float *logits; float *value;
};

// nbytes from global to LDS by ONE wave (block_copy_in's scheme): 16-byte pieces where the source allows, then dwords, then bytes.
// Reads exactly [g, g + nbytes)
EWN_DEV void wave_copy_in(int8_t *lds, const int8_t *g, int nbytes, int lane)
{
    const int nq = (((uintptr_t)g & 15) == 0) ? nbytes >> 4 : 0;
    for (int i = lane; i < nq; i += 64) ((uint4 *)lds)[i] = ((const uint4 *)g)[i];
    const int w0 = nq << 2, nw = (((uintptr_t)g & 3) == 0) ? nbytes >> 2 : w0;
    for (int i = w0 + lane; i < nw; i += 64) ((u32 *)lds)[i] = ((const u32 *)g)[i];
    for (int i = (nw << 2) + lane; i < nbytes; i += 64) lds[i] = g[i];
}

// Phases: (1) the block packs the forward image(s) into LDS, one barrier; (2) every wave walks its tiles: packed boards -> staging
// (coalesced), staging -> slots (stride STR, zero past the board and for samples >= M), both nets' forward on the matrix pipe, the
// Gumbel-max / argmax, the stores of lanes 0 .. 31.  Nothing in (2) crosses a wave: no block barrier after the pack.
template <int S, bool WANT_VALUE>
__global__ __launch_bounds__(PRED_NT, 1) void k_predict_mlp(int M, int deterministic, u64 key, PredBuf B)
{
    using P = PredGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR, WPS = STR / 4;      // dwords per slot
    static_assert(Q3::FWD_BYTES % 16 == 0, "image alignment");
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wpi = lds;
    int8_t *Wvf = Wpi + Q3::FWD_BYTES;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *slots = Wpi + (WANT_VALUE ? 2 : 1) * Q3::FWD_BYTES + wave * 32 * STR;
    int8_t *stage = Wpi + (WANT_VALUE ? 2 : 1) * Q3::FWD_BYTES + P::NW * 32 * STR + wave * P::STAGE;
    mlp3_pack_fwd<S>(Wpi, B.params, 0, threadIdx.x, PRED_NT);
    if constexpr (WANT_VALUE) mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, PRED_NT);
    __syncthreads();

    const int tiles = (M - 1) / 32 + 1;                    // M >= 1
    const int j = lane & 31, h = lane >> 5;
    #pragma unroll 1
    for (int t0 = (int)blockIdx.x * P::NW; t0 < tiles; t0 += (int)gridDim.x * P::NW) {   // block-uniform trip count
        const int tile = t0 + wave;
        if (tile >= tiles) continue;                       // wave-uniform: the last trip's waves without a tile
        const int nm = min(32, M - tile * 32);             // 1 .. 32 samples of this tile exist
        const size_t m = (size_t)tile * 32 + j;
        const bool live = j < nm;
        wave_copy_in(stage, B.boards + (size_t)tile * 32 * CELLS, nm * CELLS, lane);
        const int dj = live ? (int)B.dice[m] : 0;
        __builtin_amdgcn_wave_barrier();
        // slot dword q of sample jj = board bytes 4 q .. 4 q + 3: two aligned staging dwords and one v_alignbyte_b32; bytes from CELLS
        // on, and every byte of a sample that does not exist, are zero (what the staging area holds there is never used)
        #pragma unroll
        for (int i0 = 0; i0 < 32 * WPS; i0 += 64) {
            const int i = i0 + lane, jj = i / WPS, q = i % WPS;
            const int off = jj * CELLS + 4 * q;
            const u32 *wp = (const u32 *)(stage + (off & ~3));
            const u32 v = __builtin_amdgcn_alignbyte(wp[1], wp[0], (u32)(off & 3));
            const u32 keep = jj >= nm ? 0u : (q < CELLS / 4 ? 0xFFFFFFFFu : (q == CELLS / 4 ? 0xFFu : 0u));
            ((u32 *)slots)[i] = v & keep;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the network(s): the tile's 32 samples are the 32 columns of the MFMA tiles (sample j = column j, both lane halves); lane
        // (j, h) turns bytes 16 kb + 8 h .. + 7 of sample j's slot into the eight bf16 of its k-block operand (pol_obs_operand)
        const int8_t *sj = slots + j * STR + 8 * h;
        auto xb = [&](int kb) { return pol_obs_operand<S>(sj, kb, h, dj); };
        f32x16 h1[2], h2[2];
        float lo[MLP_NA];
        mlp3_forward<S, MLP_NA>(Wpi, lane, xb, h1, h2, lo);
        float vo[1] = { 0.0f };
        if constexpr (WANT_VALUE) mlp3_forward<S, 1>(Wvf, lane, xb, h1, h2, vo);
        __builtin_amdgcn_wave_barrier();                   // the slots are read: the next trip may overwrite them
        // ---- Gumbel-max sample (argmax of the logits when deterministic): a[0] ~ softmax(l0, l1), a[1] ~ softmax(l2, l3, l4)
        if (live && h == 0) {
            float gn[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
            if (!deterministic) {
                const u32 w = fmix32(agent_hash(0u, 0u, B.obs_id ? B.obs_id[m] : (u32)m, key) ^ PRED_POL_SALT);
                #pragma unroll
                for (int i = 0; i < 5; i++) {
                    const float u = B.uniforms ? B.uniforms[m * 5 + i] : pol_uniform(w, i);
                    gn[i] = pol_gumbel(u);
                }
            }
            const float z0 = lo[0] + gn[0], z1 = lo[1] + gn[1], z2 = lo[2] + gn[2], z3 = lo[3] + gn[3], z4 = lo[4] + gn[4];
            const int aflag = pol_pick_flag(z0, z1);
            const int adir = pol_pick_dir(z2, z3, z4);
            B.actions[m * 2] = (int8_t)aflag; B.actions[m * 2 + 1] = (int8_t)adir;
            if (B.logits) { float *p = B.logits + m * 5; p[0] = lo[0]; p[1] = lo[1]; p[2] = lo[2]; p[3] = lo[3]; p[4] = lo[4]; }
            if constexpr (WANT_VALUE) B.value[m] = vo[0];
        }
    }
}

template <int S, bool WANT_VALUE>
static int pred_launch(int M, int deterministic, u64 key, const PredBuf &pb, hipStream_t s)
{
    constexpr size_t lds = PredGeo<S>::lds_bytes(WANT_VALUE);
    static_assert(lds <= POL_LDS_MAX, "weight image(s) + the block's slots and staging must fit the CU's LDS");
    const int tiles = (M - 1) / 32 + 1, need = (tiles + PredGeo<S>::NW - 1) / PredGeo<S>::NW;
    return pol_launch_kernel(k_predict_mlp<S, WANT_VALUE>, (unsigned)(need < PRED_MAX_BLOCKS ? need : PRED_MAX_BLOCKS), PRED_NT, lds, 64 * 1024,
                             POL_LDS_MAX, s, M, deterministic, key, pb);
}

template <int S>
static int pred_by_value(int M, int deterministic, u64 key, const PredBuf &pb, hipStream_t s)
{
    return pb.value ? pred_launch<S, true>(M, deterministic, key, pb, s) : pred_launch<S, false>(M, deterministic, key, pb, s);
}

// the family's order of refusals (ewn_predict_mcts): arguments, geometry, the empty batch, pointers -- all before the launch
int ewn_predict_policy(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const float *params,
                       int deterministic, uint64_t key, const uint32_t *obs_id, const float *uniforms, int8_t *actions, float *logits,
                       float *value, void *stream)
{
    if (M < 0) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (M == 0) return EWN_OK;
    if (!boards || !dice || !params || !actions) return EWN_ENULL;
    PredBuf pb = { boards, dice, params, obs_id, uniforms, actions, logits, value };
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? pred_by_value<5>(M, deterministic ? 1 : 0, (u64)key, pb, s) : pred_by_value<7>(M, deterministic ? 1 : 0, (u64)key, pb, s);
}
