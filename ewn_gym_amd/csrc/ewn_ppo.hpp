// ewn_ppo.hpp -- the PPO update of the reference's trainer (train.py:39-49, 178-183: stable_baselines3 PPO.train as
// ewn_gym_amd/ppo.py's PPOTrainer computes it) on the records of ewn_step_k_policy(record_initial_obs = 1):
//   k_ppo_prepare     one pass over the K + 1 record rows: both nets' forward (bf16 x 3, ewn_mlp3.hpp) and the backward GAE
//                     recursion per lane in registers -> one float4 per sample {old log pi(a), advantage, return, old value}
//   k_ppo_shuffle     the minibatch order of every epoch: a keyed Feistel bijection of [0, n) with cycle walking (no sort, no host)
//   k_ppo_grad3<S, NET>  forward + backward of ONE minibatch for one net (k_a2c_grad3's step body; the t-loop becomes a loop
//                     over the minibatch's gathered 32-sample tiles); the value pass also leaves the minibatch's advantage sums for
//                     the policy pass's normalisation; per-block partials, summed by k_a2c_reduce*
//   k_ppo_apply       clip_grad_norm_ + one torch.optim.Adam step, the step count in device memory (graph replays stay right).
// Sample s = t N + lane (PPOTrainer's reshape(T * N)): its observation is record row t, its action record row t + 1.
#pragma once
#include "ewn_a2c3.hpp"

struct PpoCfg {
    int N, K, B;              // lanes, steps, minibatch size
    float gamma, gae_lambda, clip, vf_coef, ent_coef, inv_batch;
    int normalize;            // normalise the minibatch's advantages (B > 1 only)
};
struct PpoBuf {
    const uint8_t *rec;       // [K + 1][N][STR]
    const double *reward;     // [K][N] (prepare)
    const float *params;      // [P]
    float4 *samples;          // [K N] {old_logp, adv, ret, old value}: written by prepare, read by grad
    const int32_t *idx;       // [B] the minibatch's sample indices (grad)
    float *partial;           // [blocks][P] per-block gradient sums
    float *stats;             // [blocks][2][4] per block and pass: policy {-min(surr), entropy, clipped, (r-1) - log r}, value {(R-V)^2, 0, 0, 0}
    double *advst;            // [blocks][2] the value pass's sums of adv and adv^2 over the minibatch samples it saw
};

// log-softmax of the two categoricals (flag: logits 0-1, direction: logits 2-4) as torch.log_softmax computes it, probabilities as
// exp(log p), entropies, and log pi of the action (a0, a1)
struct PpoHead { float lp[5], pr[5], H0, H1, logp; };
EWN_DEV PpoHead ppo_head(const float *lg, int a0, int a1)
{
    PpoHead o;
    const float m0 = fmaxf(lg[0], lg[1]), m1 = fmaxf(lg[2], fmaxf(lg[3], lg[4]));
    const float lz0 = logf(expf(lg[0] - m0) + expf(lg[1] - m0)), lz1 = logf(expf(lg[2] - m1) + expf(lg[3] - m1) + expf(lg[4] - m1));
    #pragma unroll
    for (int i = 0; i < 5; i++) { o.lp[i] = (lg[i] - (i < 2 ? m0 : m1)) - (i < 2 ? lz0 : lz1); o.pr[i] = expf(o.lp[i]); }
    o.H0 = -(o.pr[0] * o.lp[0] + o.pr[1] * o.lp[1]);
    o.H1 = -(o.pr[2] * o.lp[2] + o.pr[3] * o.lp[3] + o.pr[4] * o.lp[4]);
    o.logp = (a0 ? o.lp[1] : o.lp[0]) + (a1 == 0 ? o.lp[2] : (a1 == 1 ? o.lp[3] : o.lp[4]));
    return o;
}

// features of one record row (its board bytes and dice) as a2c3_features wants them
template <int S>
EWN_DEV A2c3Ld<S> ppo_load_obs(const uint8_t *rrow, int h)
{
    A2c3Ld<S> L;
    #pragma unroll
    for (int kb = 0; kb < Mlp3Geo<S>::KB1; kb++) L.xb[kb] = *(const uint2 *)(rrow + 16 * kb + 8 * h);
    L.dice = (int8_t)rrow[S * S];
    L.in = A2cStepIn{ 0, 0, false, 0.0f, 0.0f };
    return L;
}

// ---------------------------------------------------------------- prepare
// One wave per 32-lane tile, both nets' forward images in LDS.  t = K .. 0: V(s_t); for t < K also log pi(a_t | s_t) and the GAE step
//   delta = r_t + gamma V(s_{t+1}) (1 - done_t) - V(s_t),  A_t = delta + gamma lambda (1 - done_t) A_{t+1}
// in a2c.n_step_returns' operation order (done_t: step t's terminated byte; V(s_K) the bootstrap).
template <int S>
__global__ __launch_bounds__(256, 1) void k_ppo_prepare(PpoCfg c, PpoBuf B)
{
    using Q = Mlp3Geo<S>;
    constexpr int CELLS = S * S, STR = RecGeo<S>::STR, NWV = 4, KB1 = Q::KB1;
    extern __shared__ __attribute__((aligned(16))) int8_t lds_pp[];
    int8_t *imgp = lds_pp, *imgv = lds_pp + Q::FWD_BYTES;
    mlp3_pack_fwd<S>(imgp, B.params, 0, threadIdx.x, 256);
    mlp3_pack_fwd<S>(imgv, B.params, 1, threadIdx.x, 256);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const float gl = c.gamma * c.gae_lambda;
    const int tiles = (c.N + 31) / 32;
    #pragma unroll 1
    for (int tile = (int)blockIdx.x * NWV + wave; tile < tiles; tile += (int)gridDim.x * NWV) {
        const int game = tile * 32 + j;
        const bool valid = game < c.N;
        const int gc = valid ? game : c.N - 1;
        float vnext = 0.0f, adv = 0.0f;
        #pragma unroll 1
        for (int t = c.K; t >= 0; t--) {
            const uint8_t *rrow = B.rec + ((size_t)t * c.N + gc) * STR;
            const A2c3Ld<S> L = ppo_load_obs<S>(rrow, h);
            u32x4 xop[KB1];
            a2c3_features<S>(L, h, xop);
            f32x16 h1[2], h2[2];
            float vo[1];
            mlp3_forward<S, 1>(imgv, lane, [&](int kb) { return xop[kb]; }, h1, h2, vo);
            const float V = vo[0];
            if (t < c.K) {
                float lg[MLP_NA];
                mlp3_forward<S, MLP_NA>(imgp, lane, [&](int kb) { return xop[kb]; }, h1, h2, lg);
                const uint8_t *nrow = rrow + (size_t)c.N * STR;                 // row t + 1: action a_t, flags of step t
                const PpoHead hd = ppo_head(lg, nrow[CELLS + 1], nrow[CELLS + 2]);
                const float nonterm = nrow[CELLS + 3] ? 0.0f : 1.0f;
                const float r = (float)B.reward[(size_t)t * c.N + gc];
                const float delta = (r + c.gamma * vnext * nonterm) - V;
                adv = delta + gl * nonterm * adv;
                if (valid && h == 0) B.samples[(size_t)t * c.N + game] = make_float4(hd.logp, adv, adv + V, V);
            }
            vnext = V;
        }
    }
}

// ---------------------------------------------------------------- shuffle
// perm[e][i] for epoch e: a balanced Feistel network (four rounds, fmix32 round function) on 2 * half bits, 2^(2 half) >= n, applied
// until the value falls inside [0, n) (cycle walking: a bijection of [0, n), at most four applications on average).  The round keys
// come from (key, *counter, e) through splitmix64; tests/test_ppo_fused_cpu.py mirrors it in numpy.
__host__ __device__ inline u64 ppo_splitmix64(u64 z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
EWN_DEV u32 ppo_fmix32(u32 x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(256) void k_ppo_shuffle(long long n, int half, u64 key, const int32_t *counter, int32_t *perm)
{
    const int e = (int)blockIdx.y;
    const u32 ctr = counter ? (u32)*counter : 0u;
    const u64 ke = ppo_splitmix64(key ^ ppo_splitmix64(((u64)ctr << 32) | (u64)(u32)e));
    u32 rk[4];
    #pragma unroll
    for (int r = 0; r < 4; r++) rk[r] = (u32)ppo_splitmix64(ke + (u64)r);
    const u32 mask = (1u << half) - 1u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        u32 x = (u32)i;
        do {
            u32 L = x >> half, R = x & mask;
            #pragma unroll
            for (int r = 0; r < 4; r++) { const u32 nl = R; R = L ^ (ppo_fmix32(R ^ rk[r]) & mask); L = nl; }
            x = (L << half) | R;
        } while ((long long)x >= n);
        perm[(size_t)e * n + i] = (int32_t)x;
    }
}

// ---------------------------------------------------------------- grad
// What a tile reads for one sample (loaded one tile ahead, as k_a2c_grad3 loads one step ahead)
template <int S> struct Ppo3Ld { A2c3Ld<S> l; float4 smp; };

template <int S>
EWN_DEV Ppo3Ld<S> ppo3_load(const PpoCfg &c, const PpoBuf &B, int pos, int h)
{
    constexpr int CELLS = S * S, STR = RecGeo<S>::STR;
    int s = B.idx[pos < c.B ? pos : c.B - 1];
    if ((unsigned)s >= (unsigned)(c.K * c.N)) s = 0;      // an index outside the rollout reads sample 0 (never out of bounds)
    const uint8_t *rrow = B.rec + (size_t)s * STR;
    Ppo3Ld<S> L;
    L.l = ppo_load_obs<S>(rrow, h);
    const uint8_t *nrow = rrow + (size_t)c.N * STR;
    L.l.in.a0 = nrow[CELLS + 1]; L.l.in.a1 = nrow[CELLS + 2];
    L.smp = B.samples[s];
    return L;
}

// The loss of one sample and its gradient d[] w.r.t. the head's outputs: PPOTrainer.ppo_loss --
//   policy_loss = -mean(min(A r, A clamp(r, 1 - eps, 1 + eps))), r = exp(log pi - old log pi), A normalised per minibatch;
//   value_loss = mean((R - V)^2); loss = policy_loss - ent_coef mean(entropy) + vf_coef value_loss.
// torch's subgradients: minimum splits a tie half / half, clamp passes the gradient on its (inclusive) bounds.
template <int S, int NET>
EWN_DEV void ppo_loss_grad(const PpoCfg &c, const Ppo3Ld<S> &L, bool valid, bool stat_lane, const float *out, float amean, float astd,
                           float (&d)[6], float (&st)[4], double &sa, double &sq)
{
    const float4 smp = L.smp;
    if (!valid) return;
    if constexpr (NET == 1) {
        const float V = out[0], R = smp.z;
        if (stat_lane) { st[0] += (R - V) * (R - V); sa += (double)smp.y; sq += (double)smp.y * (double)smp.y; }
        d[0] = 2.0f * c.vf_coef * (V - R) * c.inv_batch;
    } else {
        const PpoHead hd = ppo_head(out, L.l.in.a0, L.l.in.a1);
        const float ratio = expf(hd.logp - smp.x);
        const float A = c.normalize ? (smp.y - amean) / (astd + 1e-8f) : smp.y;
        const float lo = 1.0f - c.clip, hi = 1.0f + c.clip;
        const float s1 = A * ratio, s2 = A * fminf(fmaxf(ratio, lo), hi);
        const float w1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f), w2 = s2 < s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
        const float gm = -c.inv_batch;                                       // d policy_loss / d min
        const float gr = (gm * w1) * A + ((gm * w2) * A) * ((ratio >= lo && ratio <= hi) ? 1.0f : 0.0f);
        const float glp = gr * ratio;                                        // d / d log pi (exp's backward)
        if (stat_lane) {
            st[0] += -fminf(s1, s2); st[1] += hd.H0 + hd.H1; st[2] += fabsf(ratio - 1.0f) > c.clip ? 1.0f : 0.0f;
            st[3] += (ratio - 1.0f) - (hd.logp - smp.x);
        }
        #pragma unroll
        for (int i = 0; i < 5; i++) {
            const float oh = (i < 2 ? (L.l.in.a0 == i) : (L.l.in.a1 == i - 2)) ? 1.0f : 0.0f;
            const float Hh = i < 2 ? hd.H0 : hd.H1;
            d[i] = glp * (oh - hd.pr[i]) + c.ent_coef * c.inv_batch * hd.pr[i] * (hd.lp[i] + Hh);   // d(-H)/dl_i = p_i (log p_i + H)
        }
    }
}

template <int S> struct Ppo3Geo {
    using A = A2c3Geo<S>;
    static constexpr size_t O_ADV = (A::lds_bytes() + 15) & ~(size_t)15;   // [4 waves][2] doubles: the value pass's advantage sums
    static constexpr size_t lds_bytes() { return O_ADV + 4 * 2 * sizeof(double); }
};

// NET 0: policy body + action head; NET 1: value body + value head.  256 threads: four waves, one per SIMD.  The value pass runs
// first: its blocks leave the advantage sums the policy pass normalises with (the same grid size for both).  The step body and the
// epilogue are k_a2c_grad3's (ewn_a2c3.hpp); the loop runs over the minibatch's gathered 32-sample tiles instead of the steps.
template <int S, int NET>
__global__ __launch_bounds__(256, 1) void k_ppo_grad3(PpoCfg c, PpoBuf B)
{
    constexpr int NWV = 4;
    extern __shared__ __attribute__((aligned(16))) int8_t lds3p[];
    int8_t *img = lds3p;
    double *ADV = (double *)(img + Ppo3Geo<S>::O_ADV);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;

    a2c3_pack<S, NET>(img, B.params);
    // the policy pass: the minibatch's advantage mean and unbiased std from the value pass's per-block sums (every wave sums the
    // blocks in the same fixed order: the same bits everywhere)
    float amean = 0.0f, astd = 1.0f;
    if (NET == 0 && c.normalize && c.B > 1) {
        double sa = 0.0, sq = 0.0;
        for (int b = lane; b < (int)gridDim.x; b += 64) { sa += B.advst[2 * b]; sq += B.advst[2 * b + 1]; }
        #pragma unroll
        for (int m = 1; m < 64; m <<= 1) { sa += __shfl_xor(sa, m, 64); sq += __shfl_xor(sq, m, 64); }
        const double mean = sa / (double)c.B, var = (sq - sa * mean) / (double)(c.B - 1);
        amean = (float)mean;
        astd = (float)sqrt(var > 0.0 ? var : 0.0);
    }
    __syncthreads();

    const A2c3Id id(lane);
    A2c3Acc<S> acc;
    float st[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    double st_sa = 0.0, st_sq = 0.0;

    const int tiles = (c.B + 31) / 32, stride = (int)gridDim.x * NWV;
    int tile = (int)blockIdx.x * NWV + wave;
    Ppo3Ld<S> cur = ppo3_load<S>(c, B, tile * 32 + j, h);
    #pragma unroll 1
    for (; tile < tiles; tile += stride) {
        const int pos = tile * 32 + j;
        const bool valid = pos < c.B;
        const Ppo3Ld<S> nxt = ppo3_load<S>(c, B, tile + stride < tiles ? (tile + stride) * 32 + j : pos, h);
        a2c3_step<S, NET>(img, lane, cur.l, id, acc, [&](const float *out, float (&d)[6]) {
            ppo_loss_grad<S, NET>(c, cur, valid, h == 0, out, amean, astd, d, st, st_sa, st_sq);
        }, [](int) {});
        cur = nxt;
    }

    if constexpr (NET == 1) {       // the wave's advantage sums, added up per block below
        #pragma unroll
        for (int m = 1; m < 32; m <<= 1) { st_sa += __shfl_xor(st_sa, m, 64); st_sq += __shfl_xor(st_sq, m, 64); }
        if (lane == 0) { ADV[2 * wave] = st_sa; ADV[2 * wave + 1] = st_sq; }
    }
    a2c3_epilogue<S, NET>(img, acc, st, B.partial, B.stats);     // its barriers make ADV visible to the block
    if (NET == 1 && threadIdx.x < 2) {
        double s = 0.0;
        for (int w = 0; w < NWV; w++) s += ADV[2 * w + threadIdx.x];
        B.advst[2 * blockIdx.x + threadIdx.x] = s;
    }
}

// ---------------------------------------------------------------- apply
// clip_grad_norm_(max_grad_norm) + torch.optim.Adam(lr, (beta1, beta2), eps) as torch's foreach implementation computes it:
//   m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
// with bc_i = 1 - beta_i^step and step read from and written back to device memory.  ONE block, as k_a2c_apply.
struct PpoApplyCfg { int P; float lr, beta1, beta2, eps, max_norm, grad_scale; };

template <bool VEC>
__global__ __launch_bounds__(1024) void k_ppo_apply(PpoApplyCfg c, float *params, float *exp_avg, float *exp_avg_sq, int32_t *step,
                                                    const float *grad, float *norm_out)
{
    const int tid = (int)threadIdx.x;
    const int t = *step + 1;
    const int n4 = VEC ? c.P >> 2 : 0, tail = VEC ? c.P & 3 : 0;
    float4 g[A2C_APPLY_V];
    float gt;
    const ApplyClip nc = apply_clip<VEC>(grad, c.P, c.grad_scale, c.max_norm, g, gt, [] {});
    const float clip = nc.clip;
    const double bc1 = 1.0 - pow((double)c.beta1, (double)t), bc2 = 1.0 - pow((double)c.beta2, (double)t);
    const float step_size = (float)((double)c.lr / bc1), bc2s = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - (double)c.beta1), w2 = (float)(1.0 - (double)c.beta2);
    auto adam = [&](float gg, float &m, float &v, float &p) {
        gg *= clip;
        m = m + w1 * (gg - m);
        v = v * c.beta2 + w2 * gg * gg;
        p = p + -step_size * (m / (sqrtf(v) / bc2s + c.eps));
    };
    if constexpr (VEC) {
        float4 m4[A2C_APPLY_V], v4[A2C_APPLY_V], p4[A2C_APPLY_V];
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) {
            const int i = tid + v * 1024;
            if (i < n4) { m4[v] = ((const float4 *)exp_avg)[i]; v4[v] = ((const float4 *)exp_avg_sq)[i]; p4[v] = ((const float4 *)params)[i]; }
        }
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) {
            const int i = tid + v * 1024;
            if (i < n4) {
                adam(g[v].x, m4[v].x, v4[v].x, p4[v].x); adam(g[v].y, m4[v].y, v4[v].y, p4[v].y);
                adam(g[v].z, m4[v].z, v4[v].z, p4[v].z); adam(g[v].w, m4[v].w, v4[v].w, p4[v].w);
                ((float4 *)exp_avg)[i] = m4[v]; ((float4 *)exp_avg_sq)[i] = v4[v]; ((float4 *)params)[i] = p4[v];
            }
        }
        if (tid < tail) {
            const int i = 4 * n4 + tid;
            float m = exp_avg[i], v = exp_avg_sq[i], p = params[i];
            adam(gt, m, v, p);
            exp_avg[i] = m; exp_avg_sq[i] = v; params[i] = p;
        }
    } else {
        for (int i = tid; i < c.P; i += 1024) {
            float m = exp_avg[i], v = exp_avg_sq[i], p = params[i];
            adam(grad[i] * c.grad_scale, m, v, p);
            exp_avg[i] = m; exp_avg_sq[i] = v; params[i] = p;
        }
    }
    if (tid == 0) {
        if (norm_out) *norm_out = nc.norm;
        *step = t;
    }
}
