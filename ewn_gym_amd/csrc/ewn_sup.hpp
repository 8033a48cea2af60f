// ewn_sup.hpp -- the supervised gradient of the actor-critic on M given observations (ewn_sup_grad): the third consumer of the
// bf16 x 3 step body (a2c3_step, ewn_a2c3.hpp), beside the A2C and the PPO gradient passes.  Targets come from outside -- a search
// (ewn_predict_lookahead's q through k_lookahead_targets below: expert iteration) or anything else:
//   loss = (1/M) sum_m w_m (pi_coef CE_m + vf_coef (V_m - v*_m)^2),  CE_m = -sum_i p_i logsoftmax_head(i)(logits_m)_i
// with p = target_pi[m][0..4] (0-1 the flag head, 2-4 the direction head; a head's mass s is 1, or 0 to mask it).
//   k_sup_rows<S>        boards[M][S*S] + dice[M] -> record-format rows in scratch (stride RecGeo<S>::STR, padding zeroed), so that the
//                        gradient kernels read k_ppo_grad3's eight-byte pieces of an aligned row (a2c3_features), one tile ahead
//   k_sup_grad3<S, NET>  forward + backward of all M samples for one net: k_ppo_grad3's loop over 32-sample tiles without the gather,
//                        per-block partials summed by k_a2c_reduce*
//   k_lookahead_targets  q rows [M][6] -> (target_pi, target_value, weight)
// A sample with w == 0 (or a NaN w) is skipped by selection: its targets are never used in arithmetic, so they may be NaN or inf.
#pragma once
#include "ewn_a2c3.hpp"

struct SupCfg { int M; float pi_coef, vf_coef, inv_m; };
struct SupBuf {
    const uint8_t *rows;       // [M][STR] record-format observations (k_sup_rows)
    const float *target_pi;    // [M][5]
    const float *target_value; // [M]
    const float *weight;       // [M] or NULL (all ones)
    const float *params;       // [P]
    float *partial;            // [blocks][P] per-block gradient sums
    float *stats;              // [blocks][2][4] per block and pass: policy {w CE, w entropy, agreement, w}, value {w (V - v*)^2, 0, 0, 0}
};

// ---------------------------------------------------------------- rows
// One thread per dword of the rows: byte b of row m is boards[m][b] for b < CELLS, dice[m] for b == CELLS, zero behind.  Reads exactly
// boards[0 .. M * CELLS) and dice[0 .. M).
template <int S>
__global__ __launch_bounds__(256) void k_sup_rows(int M, const int8_t *boards, const int8_t *dice, u32 *rows)
{
    constexpr int CELLS = S * S, WPS = RecGeo<S>::STR / 4;
    const size_t n = (size_t)M * WPS;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t m = i / WPS;
        const int q = (int)(i % WPS);
        u32 v = 0u;
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const int b = 4 * q + k;
            if (b < CELLS) v |= (u32)(uint8_t)boards[m * CELLS + b] << (8 * k);
            else if (b == CELLS) v |= (u32)(uint8_t)dice[m] << (8 * k);
        }
        rows[i] = v;
    }
}

// ---------------------------------------------------------------- grad
// What a tile reads from global memory: the NEXT tile's observation is asked for at the top of the step and parked in LDS behind layer 2;
// the tile's own targets are asked for behind layer 1 and first touched right before the loss.  Plain loads between the step body's
// fences: a fence (sched_barrier) keeps a load in the region it is written in, and the s_waitcnt sits at the first use.  Left to itself
// the compiler sinks a load whose only use is in the loss's conditional blocks into them, and its whole latency is waited for there.
// The targets of one sample: each pass loads its own only.
struct Sup3Tg { float p[5]; float v, w; };

template <int NET>
EWN_DEV Sup3Tg sup3_targets(const SupCfg &c, const SupBuf &B, int pos)
{
    const size_t m = (size_t)(pos < c.M ? pos : c.M - 1);
    Sup3Tg T;
    T.w = (B.weight ? B.weight : B.target_value)[m];     // weight NULL: any readable float, the loss takes 1 (nothing here uses a loaded value)
    T.v = 0.0f;
    #pragma unroll
    for (int i = 0; i < 5; i++) T.p[i] = 0.0f;
    if constexpr (NET == 1) T.v = B.target_value[m];
    else {
        #pragma unroll
        for (int i = 0; i < 5; i++) T.p[i] = B.target_pi[m * 5 + i];
    }
    return T;
}

// the pieces ppo_load_obs (ewn_ppo.hpp) takes, of row min(pos, M - 1)
template <int S>
EWN_DEV A2c3Ld<S> sup3_load(const SupCfg &c, const SupBuf &B, int pos, int h)
{
    const size_t m = (size_t)(pos < c.M ? pos : c.M - 1);
    const uint8_t *rrow = B.rows + m * RecGeo<S>::STR;
    A2c3Ld<S> L;
    #pragma unroll
    for (int kb = 0; kb < Mlp3Geo<S>::KB1; kb++) {
        L.xb[kb] = *(const uint2 *)(rrow + 16 * kb + 8 * h);
    }
    L.dice = ((const int8_t *)rrow)[S * S];
    L.in = A2cStepIn{ 0, 0, false, 0.0f, 0.0f };
    return L;
}

// The loss of one sample and its gradient d[] w.r.t. the head's outputs.  NET 0: the cross-entropy of both heads against p,
// d_i = (w / M) pi_coef (s_head(i) softmax_i - p_i); the agreement counts a sample whose pick (pol_pick_flag / pol_pick_dir, the
// rollout's comparisons) is the target's first maximum on every head with target mass.  NET 1: d = (w / M) 2 vf_coef (V - v*).
template <int NET>
EWN_DEV void sup_loss_grad(const SupCfg &c, const Sup3Tg &L, bool has_weight, bool valid, bool stat_lane, const float *out, float (&d)[6], float *st)
{
    const float w = has_weight ? L.w : 1.0f;
    if (!valid || !(w > 0.0f)) return;
    const float g = w * c.inv_m;
    if constexpr (NET == 1) {
        const float e = out[0] - L.v;
        if (stat_lane) st[0] += w * (e * e);
        d[0] = g * (2.0f * c.vf_coef * e);
    } else {
        // the two softmaxes as a2c_loss_grad takes them
        const float *lg = out, *p = L.p;
        const float m0 = fmaxf(lg[0], lg[1]), m1 = fmaxf(lg[2], fmaxf(lg[3], lg[4]));
        const float e0 = __expf(lg[0] - m0), e1 = __expf(lg[1] - m0), e2 = __expf(lg[2] - m1), e3 = __expf(lg[3] - m1), e4 = __expf(lg[4] - m1);
        const float z0 = e0 + e1, z1 = e2 + e3 + e4, lz0 = __logf(z0), lz1 = __logf(z1);
        const float pr[5] = { e0 / z0, e1 / z0, e2 / z1, e3 / z1, e4 / z1 };
        const float s0 = p[0] + p[1], s1 = p[2] + p[3] + p[4];
        if (stat_lane) {
            const float lp[5] = { lg[0] - m0 - lz0, lg[1] - m0 - lz0, lg[2] - m1 - lz1, lg[3] - m1 - lz1, lg[4] - m1 - lz1 };
            const float H0 = -(pr[0] * lp[0] + pr[1] * lp[1]), H1 = -(pr[2] * lp[2] + pr[3] * lp[3] + pr[4] * lp[4]);
            const float ce = -((p[0] * lp[0] + p[1] * lp[1]) + (p[2] * lp[2] + p[3] * lp[3] + p[4] * lp[4]));
            const bool ok0 = s0 == 0.0f || pol_pick_flag(lg[0], lg[1]) == pol_pick_flag(p[0], p[1]);
            const bool ok1 = s1 == 0.0f || pol_pick_dir(lg[2], lg[3], lg[4]) == pol_pick_dir(p[2], p[3], p[4]);
            st[0] += w * ce; st[1] += w * (H0 + H1); st[2] += (ok0 && ok1) ? 1.0f : 0.0f; st[3] += w;
        }
        #pragma unroll
        for (int i = 0; i < 5; i++) d[i] = g * (c.pi_coef * ((i < 2 ? s0 : s1) * pr[i] - p[i]));
    }
}

// LDS of k_sup_grad3: k_a2c_grad3's images, then per thread, as [piece][thread] 16-byte slots that only the thread itself reads back:
// a stash of the NEXT tile's observation (its KB1 eight-byte pieces and the dice) and the thread's four loss sums
template <int S> struct Sup3Geo {
    using A = A2c3Geo<S>;
    static constexpr int KB1 = Mlp3Geo<S>::KB1, P_ST = (8 * KB1 + 4 + 15) / 16, NPIECE = P_ST + 1;
    static constexpr size_t O_NXT = (A::lds_bytes() + 15) & ~(size_t)15;
    static constexpr size_t lds_bytes() { return O_NXT + (size_t)NPIECE * 256 * 16; }
    static_assert(KB1 % 2 == 0, "two eight-byte pieces per slot");
};

template <int S>
EWN_DEV void sup3_stash(uint4 *slot, const A2c3Ld<S> &L)
{
    constexpr int KB1 = Mlp3Geo<S>::KB1;
    #pragma unroll
    for (int k = 0; k < KB1 / 2; k++) slot[k * 256] = make_uint4(L.xb[2 * k].x, L.xb[2 * k].y, L.xb[2 * k + 1].x, L.xb[2 * k + 1].y);
    *(int *)(slot + (KB1 / 2) * 256) = L.dice;
}

template <int S>
EWN_DEV A2c3Ld<S> sup3_unstash(const uint4 *slot)
{
    constexpr int KB1 = Mlp3Geo<S>::KB1;
    A2c3Ld<S> L;
    #pragma unroll
    for (int k = 0; k < KB1 / 2; k++) {
        const uint4 v = slot[k * 256];
        L.xb[2 * k] = make_uint2(v.x, v.y); L.xb[2 * k + 1] = make_uint2(v.z, v.w);
    }
    L.dice = *(const int *)(slot + (KB1 / 2) * 256);
    L.in = A2cStepIn{ 0, 0, false, 0.0f, 0.0f };
    return L;
}

// keeps the targets' loads out of the loss's conditional blocks: an empty statement that reads them in the step's main line
EWN_DEV void sup3_pin(Sup3Tg &T)
{
    asm volatile("" : "+v"(T.p[0]), "+v"(T.p[1]), "+v"(T.p[2]), "+v"(T.p[3]), "+v"(T.p[4]), "+v"(T.v), "+v"(T.w));
}

// NET 0: policy body + action head; NET 1: value body + value head.  256 threads: four waves, one per SIMD; one 32-sample tile per
// wave and trip, grid-stride over the tiles.  The step body and the epilogue are k_a2c_grad3's.  Registers: the step body leaves a lone
// wave none to spare on 7x7, and the loss is where it peaks, so (1) the next tile's observation, asked for at the top of the step, is
// parked in LDS behind layer 2 (the s_waitcnt is there) instead of staying in registers through the loss and the backward pass, and
// the targets live from layer 2 to the loss only, (2) the loss sums live in LDS, and (3) the lane id is made opaque per trip, so that
// what is derived from it (the identity operands, LDS addresses) is recomputed per tile, a few dozen VALU instructions, instead of
// living across the loop.
template <int S, int NET>
__global__ __launch_bounds__(256, 1) void k_sup_grad3(SupCfg c, SupBuf B)
{
    constexpr int NWV = 4;
    extern __shared__ __attribute__((aligned(16))) int8_t lds3s[];
    int8_t *img = lds3s;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // wave: uniform, so are the tile counters
    {
        uint4 *slot = (uint4 *)(img + Sup3Geo<S>::O_NXT) + threadIdx.x;
        slot[Sup3Geo<S>::P_ST * 256] = make_uint4(0u, 0u, 0u, 0u);
    }
    a2c3_pack<S, NET>(img, B.params);
    __syncthreads();
    A2c3Acc<S> acc;
    const int tiles = (c.M + 31) / 32, stride = (int)gridDim.x * NWV;
    int tile = (int)blockIdx.x * NWV + wave;
    sup3_stash<S>((uint4 *)(img + Sup3Geo<S>::O_NXT) + threadIdx.x, sup3_load<S>(c, B, tile * 32 + (lane & 31), lane >> 5));
    #pragma unroll 1
    for (; tile < tiles; tile += stride) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const A2c3Id id(ln);
        const int j = ln & 31, h = ln >> 5;
        uint4 *slot = (uint4 *)(img + Sup3Geo<S>::O_NXT) + (wave * 64 + ln);
        const int pos = tile * 32 + j;
        const bool valid = pos < c.M;
        const A2c3Ld<S> cur = sup3_unstash<S>(slot);
        const A2c3Ld<S> nxt = sup3_load<S>(c, B, tile + stride < tiles ? (tile + stride) * 32 + j : pos, h);
        A2C3_FENCE();      // the loads are issued here, in front of the step; their first use is the stash behind layer 2
        Sup3Tg tg;
        a2c3_step<S, NET>(img, ln, cur, id, acc, [&](const float *out, float (&d)[6]) {
            sup_loss_grad<NET>(c, tg, B.weight != nullptr, valid, h == 0, out, d, (float *)(slot + Sup3Geo<S>::P_ST * 256));
        }, [&](int region) {
            if (region == 1) tg = sup3_targets<NET>(c, B, pos);
            if (region == 2) sup3_stash<S>(slot, nxt);
            if (region == 5) sup3_pin(tg);
        });
    }
    float st[4];
    {
        const float4 v = *(const float4 *)((uint4 *)(img + Sup3Geo<S>::O_NXT) + Sup3Geo<S>::P_ST * 256 + threadIdx.x);
        st[0] = v.x; st[1] = v.y; st[2] = v.z; st[3] = v.w;
    }
    a2c3_epilogue<S, NET>(img, acc, st, B.partial, B.stats);
}

// ---------------------------------------------------------------- targets
// One thread per q row.  The finite set is the entries above -inf.  Empty: five zeros, value 0, weight 0.  Else weight 1, value the
// maximum; temperature 0: the first maximum (strict >, ewn_predict_lookahead's action) one-hot on both heads -- (0.5, 0.5) on the flag
// head when both flags' entries of that direction have equal bits (both flags name one cube); temperature > 0: the softmax of
// q / temperature over the finite set, summed over r for the flag head and over f for the direction head, in index order.
__global__ __launch_bounds__(256) void k_lookahead_targets(int M, const float *q, float temperature, float *target_pi, float *target_value,
                                                           float *weight)
{
    const float NINF = -__builtin_inff();
    for (size_t m = (size_t)blockIdx.x * 256 + threadIdx.x; m < (size_t)M; m += (size_t)gridDim.x * 256) {
        float x[6];
        #pragma unroll
        for (int i = 0; i < 6; i++) x[i] = q[m * 6 + i];
        int best = -1;
        float top = 0.0f;
        #pragma unroll
        for (int i = 0; i < 6; i++) {
            if (x[i] > NINF && (best < 0 || x[i] > top)) { best = i; top = x[i]; }
        }
        float pi[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (best >= 0) {
            if (temperature == 0.0f) {
                const int f = best / 3, r = best - 3 * f;
                u32 b0 = 0u, b1 = 0u;
                #pragma unroll
                for (int i = 0; i < 3; i++) { if (i == r) { b0 = __float_as_uint(x[i]); b1 = __float_as_uint(x[3 + i]); } }
                if (b0 == b1) pi[0] = pi[1] = 0.5f;
                else { pi[0] = f == 0 ? 1.0f : 0.0f; pi[1] = f == 1 ? 1.0f : 0.0f; }
                #pragma unroll
                for (int i = 0; i < 3; i++) pi[2 + i] = i == r ? 1.0f : 0.0f;
            } else {
                float e[6], z = 0.0f;
                #pragma unroll
                for (int i = 0; i < 6; i++) { e[i] = x[i] > NINF ? expf((x[i] - top) / temperature) : 0.0f; z += e[i]; }
                #pragma unroll
                for (int i = 0; i < 6; i++) e[i] = e[i] / z;
                pi[0] = (e[0] + e[1]) + e[2]; pi[1] = (e[3] + e[4]) + e[5];
                pi[2] = e[0] + e[3]; pi[3] = e[1] + e[4]; pi[4] = e[2] + e[5];
            }
        }
        #pragma unroll
        for (int i = 0; i < 5; i++) target_pi[m * 5 + i] = pi[i];
        target_value[m] = best >= 0 ? top : 0.0f;
        weight[m] = best >= 0 ? 1.0f : 0.0f;
    }
}
