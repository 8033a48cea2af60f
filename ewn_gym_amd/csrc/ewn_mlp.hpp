// ewn_mlp.hpp -- the actor-critic of the reference's trainer (train.py:35-63: stable_baselines3 "MultiInputPolicy" with
// activation_fn=Tanh, i.e. SB3's default two SEPARATE 64-64 tanh bodies for policy and value, a MultiDiscrete([2, 3]) action
// head of 5 logits and a scalar value head): its parameter layout and the pieces of the MFMA result layout that the bf16 x 3
// matrix products (ewn_mlp3.hpp) of the rollout (k_rollout_mlp) and the gradient kernels (k_a2c_grad3, k_ppo_grad3) share.
//
// A 32x32 MFMA tile has its sample (game) on the lane (lane & 31) and its units in the 16 registers: register r of lane half
// h = lane >> 5 holds unit row mlp_row(r, h).  (The exact-f32 v_mfma_f32_32x32x2_f32 was dropped: measured with tools/mfma_probe.hip,
// it takes 64 cycles for K = 2 and does not overlap with VALU work on its SIMD.)
#pragma once
#include "ewn_core.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MLP_H 64     // hidden width of both bodies (SB3 default net_arch)
#define MLP_NA 5     // logits of MultiDiscrete([2, 3]) (envs/ewn.py:59)

// features: the S*S board cells as floats, then one_hot(dice_roll - 1) of width cube_num + 1 = 7 (the observation space's
// Discrete(cube_num + 1, start=1), envs/ewn.py:66-68; cube_layer 3)
template <int S> struct MlpGeo {
    static constexpr int F = S * S + 7;
    // flat fp32 parameter vector, in the order of a2c.ActorCritic.parameters(): body pi (W1 [64][F], b1, W2 [64][64], b2),
    // body vf (same), action head W [5][64], b [5], value head W [1][64], b [1]
    static constexpr int BODY = MLP_H * F + MLP_H + MLP_H * MLP_H + MLP_H;
    static constexpr int O_PI = 0, O_VF = BODY, O_AW = 2 * BODY, O_AB = O_AW + MLP_NA * MLP_H, O_VW = O_AB + MLP_NA, O_VB = O_VW + MLP_H;
    static constexpr int P = O_VB + 1;
};

// unit row of a 32x32 MFMA result held in register r of a lane of half h (lane >> 5)
EWN_DEV constexpr int mlp_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// accumulator initialised with the bias: register r <- b[mlp_row(r, h)]; rows 8g + 4h .. + 3 are one 16-byte read
EWN_DEV f32x16 mlp_bias_acc(const float *b, int h)
{
    f32x16 a;
    #pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 v = *(const float4 *)(b + 8 * g + 4 * h);
        a[4 * g] = v.x; a[4 * g + 1] = v.y; a[4 * g + 2] = v.z; a[4 * g + 3] = v.w;
    }
    return a;
}

// tanh(x) = 1 - 2 / (exp(2x) + 1): one v_exp_f32, one v_rcp_f32; absolute error ~1e-7 (saturates cleanly to +-1)
EWN_DEV float mlp_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f); }

EWN_DEV f32x16 mlp_tanh16(f32x16 a)
{
    #pragma unroll
    for (int i = 0; i < 16; i++) a[i] = mlp_tanh(a[i]);
    return a;
}

// value of x in the lane of the other half with the same sample (lane ^ 32)
EWN_DEV float mlp_other_half(float x, int lane)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(((lane ^ 32) & 63) << 2, __float_as_int(x)));
}
