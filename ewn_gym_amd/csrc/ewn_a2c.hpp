// ewn_a2c.hpp -- the A2C update of the reference's trainer (train.py:35-63, 148: stable_baselines3 A2C.train on the n-step
// rollout: policy-gradient loss + vf_coef * value MSE + ent_coef * entropy bonus, one RMSprop step, max_grad_norm clipping) over the
// trajectory records ewn_step_k_policy writes.  Here: the configuration, the per-sample loss and its gradient w.r.t. the head's
// outputs, and the kernels after the gradient pass:
//   k_a2c_reduce*     sums the per-block partial gradients into the flat gradient (the bucket a multi-GPU job all-reduces), and
//   k_a2c_apply       clips by the global norm and takes the RMSprop step on the flat parameter vector.
// The gradient pass itself is k_a2c_grad3 (ewn_a2c3.hpp): the value pass (bootstrap V(s_K), n-step returns, the advantages left in a
// scratch column), then the policy pass; forward and backward on the bf16 matrix pipe at fp32 accuracy.  Weight gradients accumulate
// in MFMA accumulators for all the samples a wave sees, and a block reduces its waves in a fixed order, so results are bit-reproducible.
#pragma once
#include "ewn_mlp.hpp"
#include "ewn_rollout.hpp"

struct A2cCfg { int N, K; float gamma, vf_coef, ent_coef, inv_batch; };
struct A2cBuf {
    const uint8_t *rec;      // [K + 1][N][STR] trajectory records, row 0 = the observation before step 0
    const double *reward;    // [K][N]
    const float *params;     // [P]
    float *adv;              // [K][N] advantages: written by the value pass, read by the policy pass
    float *partial;          // [blocks][P] per-block gradient sums (each pass writes its own body's and head's entries)
    float *stats;            // [blocks][2][4] per block and pass: loss sums {policy, value, entropy, -}
};

// sum over the 32 sample lanes of a half (lanes with the same lane >> 5): every lane of the half ends up with the total
EWN_DEV float a2c_sum32(float x)
{
    #pragma unroll
    for (int m = 1; m < 32; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The loss of one sample at step t and its gradient d[] w.r.t. the head's outputs (SB3 A2C.train: policy_loss = -(adv * log_prob).mean(),
// value_loss = mse(returns, values), entropy_loss = -entropy.mean(); loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss).
// NET 1 (value pass): the n-step return R_t = r_t + gamma (1 - done_t) R_{t+1} (GAE with lambda 1), the advantage R_t - V(s_t) left in
// B.adv for the policy pass.  NET 0 (policy pass): two categoricals (flag: logits 0-1, direction: logits 2-4).  stat_lane: this lane
// writes the advantage and counts the loss sums (one lane per sample).
// what a step's loss needs besides the head outputs
struct A2cStepIn { int a0, a1; bool term; float rew, adv; };
template <int NET>
EWN_DEV A2cStepIn a2c_step_in(const A2cCfg &c, const A2cBuf &B, const uint8_t *nrow, int cells, int t, int gc)
{
    A2cStepIn in;
    in.a0 = nrow[cells + 1]; in.a1 = nrow[cells + 2]; in.term = nrow[cells + 3] != 0;
    in.rew = NET == 1 ? (float)B.reward[(size_t)t * c.N + gc] : 0.0f;
    in.adv = NET == 0 ? B.adv[(size_t)t * c.N + gc] : 0.0f;
    return in;
}

template <int NET>
EWN_DEV void a2c_loss_grad(const A2cCfg &c, const A2cBuf &B, const A2cStepIn &in, int t, int game, bool valid, bool stat_lane,
                           const float *out, float &Rn, float (&d)[6], float &st_pl, float &st_vl, float &st_en)
{
    if constexpr (NET == 1) {
        const float R = in.rew + (in.term ? 0.0f : c.gamma * Rn);
        Rn = R;
        const float V = out[0];
        if (valid) {
            if (stat_lane) { B.adv[(size_t)t * c.N + game] = R - V; st_vl += (R - V) * (R - V); }
            d[0] = 2.0f * c.vf_coef * (V - R) * c.inv_batch;
        }
    } else {
        const float *lg = out;
        const int a0 = in.a0, a1 = in.a1;
        const float adv = in.adv;
        const float m0 = fmaxf(lg[0], lg[1]), m1 = fmaxf(lg[2], fmaxf(lg[3], lg[4]));
        const float e0 = __expf(lg[0] - m0), e1 = __expf(lg[1] - m0), e2 = __expf(lg[2] - m1), e3 = __expf(lg[3] - m1), e4 = __expf(lg[4] - m1);
        const float z0 = e0 + e1, z1 = e2 + e3 + e4, lz0 = __logf(z0), lz1 = __logf(z1);
        const float pr[5] = { e0 / z0, e1 / z0, e2 / z1, e3 / z1, e4 / z1 };
        const float lp[5] = { lg[0] - m0 - lz0, lg[1] - m0 - lz0, lg[2] - m1 - lz1, lg[3] - m1 - lz1, lg[4] - m1 - lz1 };
        const float H0 = -(pr[0] * lp[0] + pr[1] * lp[1]), H1 = -(pr[2] * lp[2] + pr[3] * lp[3] + pr[4] * lp[4]);
        const float logp = (a0 ? lp[1] : lp[0]) + (a1 == 0 ? lp[2] : (a1 == 1 ? lp[3] : lp[4]));
        if (valid) {
            if (stat_lane) { st_pl += -adv * logp; st_en += H0 + H1; }
            #pragma unroll
            for (int i = 0; i < 5; i++) {
                const float oh = (i < 2 ? (a0 == i) : (a1 == i - 2)) ? 1.0f : 0.0f;
                const float Hh = i < 2 ? H0 : H1;
                d[i] = c.inv_batch * (-adv * (oh - pr[i]) + c.ent_coef * pr[i] * (lp[i] + Hh));   // d(-H)/dl_i = p_i (log p_i + H)
            }
        }
    }
}

// ---- partials -> flat gradient (+ loss sums and the squared norm's per-block pieces)
struct A2cRedBuf { const float *partial; const float *stats; float *grad; int blocks, P; };

#define A2C_RED_E 32     // elements per block of k_a2c_reduce
__global__ __launch_bounds__(256) void k_a2c_reduce(A2cRedBuf B)
{
    // grad[i] = sum over blocks of partial[b][i]; grad[P .. P + 7] = loss sums {policy, value, entropy, 0} x {pi pass, vf pass}.
    // 32 elements per block, eight threads per element (each sums every eighth block with independent loads in flight, then the
    // eight partial sums are added in a fixed order): the first version walked all blocks in one thread per element, a chain of
    // 256 dependent-latency loads on 13 k threads (88 us for 13 MB).
    __shared__ float part[8][A2C_RED_E];
    const int e = (int)threadIdx.x & (A2C_RED_E - 1), q = (int)threadIdx.x / A2C_RED_E, i = (int)blockIdx.x * A2C_RED_E + e;
    float s = 0.0f;
    if (i < B.P) {
        const float *p = B.partial + i;
        float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        int b = q;
        for (; b + 24 < B.blocks; b += 32) {
            #pragma unroll
            for (int u = 0; u < 4; u++) acc[u] += p[(size_t)(b + 8 * u) * B.P];
        }
        for (; b < B.blocks; b += 8) acc[0] += p[(size_t)b * B.P];
        s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    } else if (i < B.P + 8) {
        for (int b = q; b < B.blocks; b += 8) s += B.stats[(size_t)b * 8 + (i - B.P)];
    }
    part[q][e] = s;
    __syncthreads();
    if (q == 0 && i < B.P + 8)
        B.grad[i] = ((part[0][e] + part[1][e]) + (part[2][e] + part[3][e])) + ((part[4][e] + part[5][e]) + (part[6][e] + part[7][e]));
}

// The same sum with 8-byte loads and every load of a thread in flight at once: 16 element PAIRS per block, sixteen threads per pair, each
// summing every sixteenth block (16 independent loads for the 256 blocks of a full launch), then the sixteen partial sums in a fixed
// order.  Needs an even P and an 8-byte aligned `partial` (the launcher checks; k_a2c_reduce above is the fallback).  11.2 -> measured
// in profiles/r03/a2c/kernel_stats.csv.
#define A2C_RED2_E 16
__global__ __launch_bounds__(256) void k_a2c_reduce2(A2cRedBuf B)
{
    __shared__ float2 part[16][A2C_RED2_E];
    const int e = (int)threadIdx.x & (A2C_RED2_E - 1), q = (int)threadIdx.x / A2C_RED2_E, i = 2 * ((int)blockIdx.x * A2C_RED2_E + e);
    float2 s = make_float2(0.0f, 0.0f);
    if (i < B.P) {
        const float2 *p = (const float2 *)(B.partial + i);
        const size_t row = (size_t)(B.P >> 1);
        float2 v[16];
        int b = q;
        for (; b + 240 < B.blocks; b += 256) {
            #pragma unroll
            for (int u = 0; u < 16; u++) v[u] = p[(size_t)(b + 16 * u) * row];
            #pragma unroll
            for (int u = 0; u < 16; u += 4) {   // a fixed tree: bit-reproducible
                s.x += (v[u].x + v[u + 1].x) + (v[u + 2].x + v[u + 3].x);
                s.y += (v[u].y + v[u + 1].y) + (v[u + 2].y + v[u + 3].y);
            }
        }
        for (; b < B.blocks; b += 16) { const float2 w = p[(size_t)b * row]; s.x += w.x; s.y += w.y; }
    } else if (i < B.P + 8) {
        for (int b = q; b < B.blocks; b += 16) { s.x += B.stats[(size_t)b * 8 + (i - B.P)]; s.y += B.stats[(size_t)b * 8 + (i - B.P) + 1]; }
    }
    part[q][e] = s;
    __syncthreads();
    if (q == 0 && i < B.P + 8) {
        float2 t = make_float2(0.0f, 0.0f);
        #pragma unroll
        for (int k = 0; k < 16; k += 4) {
            t.x += (part[k][e].x + part[k + 1][e].x) + (part[k + 2][e].x + part[k + 3][e].x);
            t.y += (part[k][e].y + part[k + 1][e].y) + (part[k + 2][e].y + part[k + 3][e].y);
        }
        B.grad[i] = t.x; B.grad[i + 1] = t.y;
    }
}

// ---- clip_grad_norm_(max_grad_norm) + RMSprop(alpha, eps) step (torch.optim.RMSprop as SB3's A2C configures it: centered = False,
// momentum 0, weight_decay 0): sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps).  ONE block (13 k parameters): the norm
// needs every element, and a second launch would cost more than the arithmetic.
struct A2cApplyCfg { int P; float lr, alpha, eps, max_norm, grad_scale; };

// The clip_grad_norm_ half of an apply kernel (ONE block of 1024 threads): the gradient times grad_scale, its global norm and the
// clip factor.  VEC: 16-byte aligned buffers, P <= 1024 x 4 x A2C_APPLY_V -- the thread's float4 pieces of the scaled gradient g[] and
// its tail element gt are loaded together and stay in registers for the step (the step reloads nothing); else the plain strided loop.
// prefetch(): the caller's own loads, issued behind the gradient's and before the norm's reduction.
#define A2C_APPLY_V 4
struct ApplyClip { float norm, clip; };

template <bool VEC, class PREFETCH>
EWN_DEV ApplyClip apply_clip(const float *grad, int P, float grad_scale, float max_norm, float4 (&g)[A2C_APPLY_V], float &gt, PREFETCH &&prefetch)
{
    __shared__ float red[16];
    const int tid = (int)threadIdx.x;
    float ss = 0.0f;
    gt = 0.0f;
    if constexpr (VEC) {
        const int n4 = P >> 2, tail = P & 3;
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) { const int i = tid + v * 1024; g[v] = i < n4 ? ((const float4 *)grad)[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
        gt = tid < tail ? grad[4 * n4 + tid] * grad_scale : 0.0f;
        prefetch();
        ss = gt * gt;
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) {
            g[v].x *= grad_scale; g[v].y *= grad_scale; g[v].z *= grad_scale; g[v].w *= grad_scale;
            ss += (g[v].x * g[v].x + g[v].y * g[v].y) + (g[v].z * g[v].z + g[v].w * g[v].w);
        }
    } else {
        for (int i = tid; i < P; i += 1024) { const float gg = grad[i] * grad_scale; ss += gg * gg; }
    }
    #pragma unroll
    for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.0f;
    #pragma unroll
    for (int k = 0; k < 16; k++) tot += red[k];
    const float norm = sqrtf(tot);
    return { norm, max_norm > 0.0f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f };   // torch.nn.utils.clip_grad_norm_
}

// VEC: the thread's pieces of sq_avg and params are asked for under the gradient's, before the norm's reduction -- three memory round
// trips in all, where the plain loop makes 2 x 13 dependent ones (the kernel is one block, nothing else hides them).
template <bool VEC>
__global__ __launch_bounds__(1024) void k_a2c_apply(A2cApplyCfg c, float *params, float *sq_avg, const float *grad, float *norm_out)
{
    const int tid = (int)threadIdx.x;
    const int n4 = VEC ? c.P >> 2 : 0, tail = VEC ? c.P & 3 : 0;
    float4 g[A2C_APPLY_V], q[A2C_APPLY_V], w[A2C_APPLY_V];
    float gt;
    const ApplyClip nc = apply_clip<VEC>(grad, c.P, c.grad_scale, c.max_norm, g, gt, [&] {
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) {
            const int i = tid + v * 1024;
            if (i < n4) { q[v] = ((const float4 *)sq_avg)[i]; w[v] = ((const float4 *)params)[i]; }
        }
    });
    const float clip = nc.clip;
    auto step = [&](float gg, float &sq, float &pp) {
        gg *= clip;
        sq = c.alpha * sq + (1.0f - c.alpha) * gg * gg;
        pp -= c.lr * gg / (sqrtf(sq) + c.eps);
    };
    if constexpr (VEC) {
        #pragma unroll
        for (int v = 0; v < A2C_APPLY_V; v++) {
            const int i = tid + v * 1024;
            if (i < n4) {
                step(g[v].x, q[v].x, w[v].x); step(g[v].y, q[v].y, w[v].y); step(g[v].z, q[v].z, w[v].z); step(g[v].w, q[v].w, w[v].w);
                ((float4 *)sq_avg)[i] = q[v]; ((float4 *)params)[i] = w[v];
            }
        }
        if (tid < tail) { float sq = sq_avg[4 * n4 + tid], pp = params[4 * n4 + tid]; step(gt, sq, pp); sq_avg[4 * n4 + tid] = sq; params[4 * n4 + tid] = pp; }
    } else {
        for (int i = tid; i < c.P; i += 1024) { float sq = sq_avg[i], pp = params[i]; step(grad[i] * c.grad_scale, sq, pp); sq_avg[i] = sq; params[i] = pp; }
    }
    if (tid == 0 && norm_out) *norm_out = nc.norm;
}
