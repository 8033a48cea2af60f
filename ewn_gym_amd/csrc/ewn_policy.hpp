// ewn_policy.hpp -- K env steps per launch with the TRAINED policy as the agent (C ABI: ewn_step_k_policy, EWN_AGENT_MLP):
// the rollout collector of the reference's trainer (train.py:35-63, 134, 148: SB3 A2C.learn -> collect_rollouts over
// SubprocVecEnv workers of `MiniMaxHeuristicEnv`, envs/training_ewn.py:40-99) as ONE kernel.  Per env step and game:
// observation -> features -> the policy network on the matrix cores (ewn_mlp3.hpp) -> Gumbel-max sample of MultiDiscrete([2, 3])
// -> the env step (plain or reward-shaped, with its tolerance counter) -> the opponent's search -> reply -> auto-reset ->
// one trajectory record.  The game never leaves its registers, the network's weights never leave LDS.
//
// Lock-step over env steps (not the slot-task loop of k_rollout_slots): the network is evaluated for a whole wave of games at
// once, so the games of a wave have to be at the same step.  Two lanes per game (as k_rollout_d3), 512 threads = 256 games per
// block so that ONE table image and ONE weight image serve eight waves: 65 536 games are 256 blocks, one per CU, two waves per
// SIMD -- while one wave's MFMAs run, the other's search has the VALU.
#pragma once
#include "ewn_rollout.hpp"
#include "ewn_mlp3.hpp"

struct PolCfg {
    int N, autoreset, lane_offset, depth, K;
    int shaped, refresh, deterministic, want_value, rec0;   // rec0: record row 0 = the observation before step 0 (then K + 1 rows)
    u32 seed_stride, W;
    double reward, illegal_reward;
    u64 key, noise_key;
};

struct PolBuf {
    int8_t *board; int8_t *dice; uint8_t *done; u32 *rng; double *prev_score; int32_t *tolerance;
    const void *tables;
    const float *params;
    // trajectory (all optional): the columns of ewn_rollout_out, the record, and the policy's own outputs
    int8_t *t_board; int8_t *t_dice; int8_t *t_action; double *t_reward; uint8_t *t_term; uint8_t *t_trunc; uint8_t *t_info; uint8_t *t_rec;
    float *t_logits; float *t_value; float *t_noise;
    double *ret_sum; int32_t *n_steps; int32_t *n_episodes; int32_t *n_wins;
};

// the policy opponent of k_rollout_mlp_vs (OPP 3): a second parameter vector, frozen for the launch
struct PolOpp {
    const float *params;
    int8_t *t_action;          // [K][N][3] {dice, flag, dir} of the opponent's move, {0, 0, 0} when it did not move (optional; never with TRJ 1)
    u64 noise_key;
    int deterministic;
};

// LDS-DMA copy of the table image for a block of NT threads (tables_to_lds assumes 256)
template <int BYTES, int NT>
EWN_DEV void tables_to_lds_nt(int8_t *lds, const int8_t *g)
{
    static_assert(BYTES % 4096 == 0, "table size must be padded to 4 KiB");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int off = wave * 1024; off < BYTES; off += (NT / 64) * 1024)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off + lane * 16),
                                         (__attribute__((address_space(3))) void *)(lds + off), 16, 0, 0);
}

// LDS bytes of k_rollout_mlp<S, ., NT>: table image | weight image(s) | 8 floats of head outputs per game | game slots | decode scratch
// (opp_net: k_rollout_mlp_vs, one more image for the opponent's policy net)
template <int S, int NT>
constexpr size_t pol_lds_bytes(bool want_value, bool opp_net = false)
{
    constexpr int GPB = NT / 2;
    return (size_t)FAST_TAB_BYTES(S) + (size_t)((want_value ? 2 : 1) + (opp_net ? 1 : 0)) * Mlp3Geo<S>::FWD_BYTES + (size_t)GPB * 8 * 4
           + (size_t)GPB * RecGeo<S>::STR + (size_t)GPB * 16;
}

// the uniforms behind a step's Gumbel noise: five words hashed out of the engine's per-step agent hash (the stream
// ewn_step_out.random_action draws from), as floats in (0, 1)
EWN_DEV float pol_uniform(u32 w0, int i)
{
    const u32 w = fmix32(w0 + (u32)(i + 1) * 0x9E3779B9u);
    return ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f);
}

// ln x on v_log_f32 (log2, ~1 ulp) -- the Gumbel noise -ln(-ln u) ten times per game and step; the library logf is ~20 instructions each
EWN_DEV float pol_log(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
// Gumbel noise of a uniform in (0, 1)
EWN_DEV float pol_gumbel(float u) { return -pol_log(-pol_log(u)); }

// the policy opponent's noise word: fmix32(the step's agent hash under (key ^ its noise_key) ^ this), so an opponent that shares the
// agent's noise_key still draws its own noise
#define POL_OPP_SALT 0x4F505031u
// ... taken before the step moves the stream, and keyed like the agent's own word (k_rollout_mlp: episode, draws so far, lane, tolerance
// left).  k_rollout_mlp_vs and k_step_vs both call this, so a step of one is a step of the other, bit for bit
EWN_DEV u32 pol_opp_noise_word(u32 seed_mix, int tol, u32 draws, int lane_global, u64 key, u64 opp_noise_key)
{
    return fmix32(agent_hash(seed_mix ^ ((u32)tol * 0x632BE5ABu), draws, (u32)lane_global, key ^ opp_noise_key) ^ POL_OPP_SALT);
}

// OPP 0: minimax max_depth 1-4 on a (level, count) table image; 1: RandomAgent; 2: minimax max_depth 5 / 6 on such an image (the
// closed form, d5_dispatch; TRJ 2 only).  RNGK: the dice, 1 Philox; 0 MT19937-compat (TRJ 2 only: one episode per lane).
// TRJ 1: the trainer's call, known at compile time -- records (row 0 = the initial observation) and the reward column, nothing else
// written per step, actions sampled, no value output (FusedA2CTrainer; the gradient kernels recompute the forward pass).  0: everything
// by PolCfg / PolBuf at run time (a dozen loop-invariant tests whose masks the compiler keeps in spilled SGPRs: 126 of them).
// TRJ 2: the evaluation (ewn_policy_eval), known at compile time -- argmax actions (no noise computed), un-shaped env, no auto-reset,
// no records and no policy outputs; the per-lane totals and optionally the action column of the steps a lane plays.  Nothing is
// written for a finished lane, so a wave whose 32 games are all finished leaves the step loop (there is no block barrier inside it);
// the other instances write rows for finished lanes and keep stepping.  Held to 256 registers (two waves per SIMD) at every NT.
// OPP 3 (k_rollout_mlp_vs below): the opponent is a second actor-critic, O.params -- after the agent half the wave runs one more forward
// pass on the opponent's canonical view of the same slots and the opponent plays its argmax / Gumbel-max sample; nothing is drawn from
// the dice stream for it.  Everything it adds is inside `if constexpr (OPP == 3)`.
template <int S, int OPP, int NT, int TRJ = 0, int RNGK = 1>
__global__ __launch_bounds__(NT, TRJ == 2 ? 2 : NT / 256) void k_rollout_mlp(PolCfg c, PolBuf B)
{
    static_assert(OPP != 3, "the policy opponent has a kernel of its own: k_rollout_mlp_vs");
    const PolOpp O{};   // named only inside `if constexpr (OPP == 3)`
#include "ewn_policy_body.inc"
}

// OPP 3: the opponent is the actor-critic O.params.  Two waves per SIMD (256 registers) at every block size.
template <int S, int NT, int TRJ = 0, int RNGK = 1, int OPP = 3>
__global__ __launch_bounds__(NT, 2) void k_rollout_mlp_vs(PolCfg c, PolBuf B, PolOpp O)
{
    static_assert(OPP == 3, "the policy opponent");
#include "ewn_policy_body.inc"
}
