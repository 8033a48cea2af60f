// ewn_policy.hip -- the policy-driven rollout (ewn_step_k_policy), its evaluation form (ewn_policy_eval: instances in
// ewn_policy_eval.hip), the fused A2C update (ewn_a2c_*) and the fused PPO update (ewn_ppo_*): kernels in ewn_policy.hpp /
// ewn_a2c.hpp / ewn_ppo.hpp, C ABI here.  The supervised gradient on given observations and targets (ewn_sup_*, ewn_lookahead_targets:
// ewn_sup.hpp) is the step body's third consumer and lives here with the other two (the reduce kernels link from this unit only).
#include "ewn_policy_host.hpp"
#include "ewn_a2c.hpp"
#include "ewn_a2c3.hpp"
#include "ewn_ppo.hpp"
#include "ewn_sup.hpp"

// which instantiation serves the configuration: opp 0 minimax (table image, max_depth 1-4), 1 RandomAgent
static int policy_plan(const ewn_config *cfg, const Geom &g, int &opp)
{
    if (!pol_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->rng_kind != EWN_RNG_PHILOX) return EWN_EUNSUPPORTED;
    if (cfg->opponent_kind == EWN_OPP_RANDOM) opp = 1;
    else if (cfg->opponent_kind == EWN_OPP_MINIMAX && fast_heur_lean(cfg->heuristic) && cfg->max_depth <= 4) opp = 0;
    else return EWN_EUNSUPPORTED;
    return EWN_OK;
}

int ewn_policy_supported(const ewn_config *cfg, const Geom &g)
{
    int opp;
    return policy_plan(cfg, g, opp);
}

int64_t ewn_policy_param_count(int board_size, int cube_layer)
{
    if (cube_layer != 3) return EWN_EUNSUPPORTED;
    switch (board_size) {
    case 5: return MlpGeo<5>::P;
    case 7: return MlpGeo<7>::P;
    default: return EWN_EUNSUPPORTED;
    }
}

template <int S, int OPP, int NT, int TRJ = 0>
static int pol_launch(const PolCfg &pc, const PolBuf &pb, hipStream_t s)
{
    if constexpr (TRJ == 0 && OPP == 0) {
        if (pol_trainer_call(pc, pb)) return pol_launch<S, OPP, NT, 1>(pc, pb, s);   // the instance that knows it at compile time
    }
    return pol_launch_games(k_rollout_mlp<S, OPP, NT, TRJ>, pc.N, NT, pol_lds_bytes<S, NT>(pc.want_value != 0), s, pc, pb);
}

template <int S>
static int pol_dispatch(const PolCfg &pc, const PolBuf &pb, int opp, hipStream_t s)
{
    // 512 threads (256 games) per block where the block's LDS fits the CU, else 256
    const bool big = pol_lds_bytes<S, 512>(pc.want_value != 0) <= POL_LDS_MAX;
    if (opp == 0) return big ? pol_launch<S, 0, 512>(pc, pb, s) : pol_launch<S, 0, 256>(pc, pb, s);
    return big ? pol_launch<S, 1, 512>(pc, pb, s) : pol_launch<S, 1, 256>(pc, pb, s);
}

int ewn_step_k_policy(const ewn_config *cfg, const ewn_state *st, int K, const ewn_policy *pol, const ewn_rollout_out *out, void *stream)
{
    Geom g; KCfg k;
    int rc = check_cfg(cfg, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (pol_state_missing(st, true, cfg->shaped != 0) || !pol || !pol->params) return EWN_ENULL;
    int opp;
    rc = policy_plan(cfg, g, opp);
    if (rc) return rc;
    const PolCfg pc = pol_cfg(k, K, pol);
    const PolBuf pb = pol_buf_rollout(st, opp == 1 ? st->tables : fast_image(st->tables, g.S, g.L, cfg->max_depth, cfg->heuristic), pol, out);
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? pol_dispatch<5>(pc, pb, opp, s) : pol_dispatch<7>(pc, pb, opp, s);
}

// ---------------------------------------------------------------- the evaluation (ewn_policy_eval)

// which evaluation instance serves the configuration: un-shaped, no auto-reset, either dice kind; opp 0 minimax max_depth 1-4,
// 1 RandomAgent, 2 minimax max_depth 5 / 6 (the closed form: the (level, count) images only, not 'two_min_dist')
static int policy_eval_plan(const ewn_config *cfg, const Geom &g, int &opp)
{
    if (!pol_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->shaped || cfg->autoreset) return EWN_EUNSUPPORTED;
    if (cfg->opponent_kind == EWN_OPP_RANDOM) opp = 1;
    else if (cfg->opponent_kind == EWN_OPP_MINIMAX && fast_heur_lean(cfg->heuristic)) opp = cfg->max_depth > 4 ? 2 : 0;
    else return EWN_EUNSUPPORTED;
    return EWN_OK;
}

int ewn_policy_eval_supported(const ewn_config *cfg)
{
    Geom g; KCfg k;
    int rc = check_cfg(cfg, g, k);
    if (rc) return rc;
    int opp;
    rc = policy_eval_plan(cfg, g, opp);
    return supported_answer(rc);
}

int ewn_policy_eval(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_rollout_out *out, void *stream)
{
    Geom g; KCfg k;
    int rc = check_cfg(cfg, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (pol_state_missing(st, true, false) || !params || !out) return EWN_ENULL;
    rc = pol_eval_out_check(out);
    if (rc) return rc;
    int opp;
    rc = policy_eval_plan(cfg, g, opp);
    if (rc) return rc;
    const PolCfg pc = pol_cfg(k, K, nullptr);
    PolBuf pb = pol_buf(st, opp == 1 ? st->tables : fast_image(st->tables, g.S, g.L, cfg->max_depth, cfg->heuristic), params);
    pb.t_action = out->action; fill_totals(pb, out);
    return ewn_launch_policy_eval(pc, pb, g.S, opp, k.rng_kind, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the A2C update

#define A2C_MAX_BLOCKS 256   // one block per CU

static int a2c_blocks(int N, int nwv)
{
    const int tiles = (N + 31) / 32, need = (tiles + nwv - 1) / nwv;
    return need < A2C_MAX_BLOCKS ? need : A2C_MAX_BLOCKS;
}

static int a2c_geom(const ewn_config *cfg, Geom &g, KCfg &k)
{
    int rc = check_cfg(cfg, g, k);
    if (rc) return rc;
    if (g.L != 3 || (g.S != 5 && g.S != 7)) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

int64_t ewn_a2c_scratch_bytes(const ewn_config *cfg, int K)
{
    Geom g; KCfg k;
    int rc = a2c_geom(cfg, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    const int64_t P = ewn_policy_param_count(g.S, g.L);
    return ((int64_t)K * k.N + (int64_t)A2C_MAX_BLOCKS * (P + 8) + 64) * 4;
}

// partials -> flat gradient: the 8-byte-load kernel where the layout allows it
static void a2c_reduce_launch(const A2cRedBuf &rb, hipStream_t s)
{
    if ((rb.P & 1) == 0 && ((uintptr_t)rb.partial & 7) == 0) k_a2c_reduce2<<<(rb.P + 8 + 2 * A2C_RED2_E - 1) / (2 * A2C_RED2_E), 256, 0, s>>>(rb);
    else k_a2c_reduce<<<(rb.P + 8 + A2C_RED_E - 1) / A2C_RED_E, 256, 0, s>>>(rb);
}

// the bf16 x 3 gradient kernels (ewn_a2c3.hpp: one wave per tile and SIMD, everything in registers) launch alike: the value pass first
// (it leaves the advantages for the policy pass), the policy pass, then the blocks' partials -> the flat gradient
template <typename Kern, typename Cfg, typename Buf>
static int grad3_launch(Kern kv, Kern kp, int blocks, size_t lds, const Cfg &c, const Buf &b, const A2cRedBuf &rb, hipStream_t s)
{
    if (hipFuncSetAttribute((const void *)kv, hipFuncAttributeMaxDynamicSharedMemorySize, POL_LDS_MAX) != hipSuccess) return EWN_ELAUNCH;
    if (hipFuncSetAttribute((const void *)kp, hipFuncAttributeMaxDynamicSharedMemorySize, POL_LDS_MAX) != hipSuccess) return EWN_ELAUNCH;
    kv<<<blocks, 256, lds, s>>>(c, b);
    kp<<<blocks, 256, lds, s>>>(c, b);
    a2c_reduce_launch(rb, s);
    return launch_status();
}

template <int S>
static int a2c_grad_launch(const A2cCfg &ac, const A2cBuf &ab, float *grad, hipStream_t s)
{
    constexpr size_t lds = A2c3Geo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "weight images + the gradient image must fit the CU's LDS");
    const int blocks = a2c_blocks(ac.N, 4);
    return grad3_launch(k_a2c_grad3<S, 1>, k_a2c_grad3<S, 0>, blocks, lds, ac, ab, A2cRedBuf{ ab.partial, ab.stats, grad, blocks, MlpGeo<S>::P }, s);
}

int ewn_a2c_grad(const ewn_config *cfg, int K, const uint8_t *record, const double *reward, const float *params, const ewn_a2c_hyper *hp,
                 float *grad, void *scratch, void *stream)
{
    Geom g; KCfg k;
    int rc = a2c_geom(cfg, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (!record || !reward || !params || !hp || !grad || !scratch) return EWN_ENULL;
    const int64_t P = ewn_policy_param_count(g.S, g.L);
    A2cCfg ac = { k.N, K, hp->gamma, hp->vf_coef, hp->ent_coef, 1.0f / ((float)K * (float)k.N) };
    A2cBuf ab;
    ab.rec = record; ab.reward = reward; ab.params = params;
    ab.adv = (float *)scratch;
    ab.partial = ab.adv + (size_t)K * k.N;
    ab.stats = ab.partial + (size_t)A2C_MAX_BLOCKS * P;
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? a2c_grad_launch<5>(ac, ab, grad, s) : a2c_grad_launch<7>(ac, ab, grad, s);
}

int ewn_a2c_apply(const ewn_config *cfg, float *params, float *sq_avg, const float *grad, const ewn_a2c_hyper *hp, float *grad_norm_out,
                  void *stream)
{
    Geom g; KCfg k;
    int rc = a2c_geom(cfg, g, k);
    if (rc) return rc;
    if (!params || !sq_avg || !grad || !hp) return EWN_ENULL;
    if (hp->world_size < 1) return EWN_EINVAL;
    A2cApplyCfg ac = { (int)ewn_policy_param_count(g.S, g.L), hp->learning_rate, hp->rms_alpha, hp->rms_eps, hp->max_grad_norm, 1.0f / (float)hp->world_size };
    const bool vec = ac.P <= 1024 * 4 * A2C_APPLY_V && ((uintptr_t)params | (uintptr_t)sq_avg | (uintptr_t)grad) % 16 == 0;
    if (vec) k_a2c_apply<true><<<1, 1024, 0, (hipStream_t)stream>>>(ac, params, sq_avg, grad, grad_norm_out);
    else k_a2c_apply<false><<<1, 1024, 0, (hipStream_t)stream>>>(ac, params, sq_avg, grad, grad_norm_out);
    return launch_status();
}

// ---------------------------------------------------------------- the PPO update

// the geometry ewn_a2c_* serves, 1 <= K, K * N samples addressable by int32, 1 <= batch_size <= K * N
static int ppo_check(const ewn_config *cfg, int K, int batch_size, Geom &g, KCfg &k)
{
    int rc = a2c_geom(cfg, g, k);
    if (rc) return rc;
    if (K < 1 || (int64_t)K * k.N > INT32_MAX) return EWN_EINVAL;
    if (batch_size < 1 || (int64_t)batch_size > (int64_t)K * k.N) return EWN_EINVAL;
    return EWN_OK;
}

int64_t ewn_ppo_scratch_bytes(const ewn_config *cfg, int K, int batch_size)
{
    Geom g; KCfg k;
    int rc = ppo_check(cfg, K, batch_size, g, k);
    if (rc) return rc;
    const int64_t P = ewn_policy_param_count(g.S, g.L);
    return (int64_t)A2C_MAX_BLOCKS * (P + 8) * 4 + (int64_t)A2C_MAX_BLOCKS * 2 * 8;
}

static PpoCfg ppo_cfg(const KCfg &k, int K, int batch_size, const ewn_ppo_hyper *hp)
{
    PpoCfg c = { k.N, K, batch_size, hp->gamma, hp->gae_lambda, hp->clip_range, hp->vf_coef, hp->ent_coef, 1.0f / (float)batch_size,
                 hp->normalize_advantage ? 1 : 0 };
    return c;
}

int ewn_ppo_prepare(const ewn_config *cfg, int K, const uint8_t *record, const double *reward, const float *params, const ewn_ppo_hyper *hp,
                    float *samples, void *stream)
{
    Geom g; KCfg k;
    int rc = ppo_check(cfg, K, 1, g, k);
    if (rc) return rc;
    if (!record || !reward || !params || !hp || !samples) return EWN_ENULL;
    PpoBuf b;
    memset(&b, 0, sizeof(b));
    b.rec = record; b.reward = reward; b.params = params; b.samples = (float4 *)samples;
    const PpoCfg c = ppo_cfg(k, K, 1, hp);
    const int blocks = (k.N + 127) / 128;            // one 32-lane tile per wave
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern, size_t lds) { return pol_launch_kernel(kern, blocks, 256, lds, 0, POL_LDS_MAX, s, c, b); };   // always opts in
    static_assert(2 * Mlp3Geo<7>::FWD_BYTES <= POL_LDS_MAX, "both nets' forward images must fit the CU's LDS");
    return g.S == 5 ? launch(k_ppo_prepare<5>, 2 * (size_t)Mlp3Geo<5>::FWD_BYTES) : launch(k_ppo_prepare<7>, 2 * (size_t)Mlp3Geo<7>::FWD_BYTES);
}

int ewn_ppo_shuffle(int64_t n, int n_epochs, uint64_t key, const int32_t *counter, int32_t *perm, void *stream)
{
    if (n < 1 || n > INT32_MAX || n_epochs < 1 || n_epochs > 65535) return EWN_EINVAL;
    if (!perm) return EWN_ENULL;
    int bits = 0;
    while ((1ll << bits) < n) bits++;
    const int half = bits < 2 ? 1 : (bits + 1) / 2;
    const int64_t need = (n + 255) / 256;
    const unsigned gx = (unsigned)(need < 1024 ? need : 1024);
    k_ppo_shuffle<<<dim3(gx, (unsigned)n_epochs), 256, 0, (hipStream_t)stream>>>((long long)n, half, (u64)key, counter, perm);
    return launch_status();
}

template <int S>
static int ppo_grad_launch(const PpoCfg &c, const PpoBuf &b, float *grad, hipStream_t s)
{
    constexpr size_t lds = Ppo3Geo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "weight images + the gradient image must fit the CU's LDS");
    const int blocks = a2c_blocks(c.B, 4);
    return grad3_launch(k_ppo_grad3<S, 1>, k_ppo_grad3<S, 0>, blocks, lds, c, b, A2cRedBuf{ b.partial, b.stats, grad, blocks, MlpGeo<S>::P }, s);
}

int ewn_ppo_grad(const ewn_config *cfg, int K, const uint8_t *record, const float *samples, const float *params, const ewn_ppo_hyper *hp,
                 const int32_t *idx, int batch_size, float *grad, void *scratch, void *stream)
{
    Geom g; KCfg k;
    int rc = ppo_check(cfg, K, batch_size, g, k);
    if (rc) return rc;
    if (!record || !samples || !params || !hp || !idx || !grad || !scratch) return EWN_ENULL;
    const int64_t P = ewn_policy_param_count(g.S, g.L);
    PpoBuf b;
    memset(&b, 0, sizeof(b));
    b.rec = record; b.params = params; b.samples = (float4 *)samples; b.idx = idx;
    b.partial = (float *)scratch;
    b.stats = b.partial + (size_t)A2C_MAX_BLOCKS * P;
    b.advst = (double *)(b.stats + (size_t)A2C_MAX_BLOCKS * 8);
    const PpoCfg c = ppo_cfg(k, K, batch_size, hp);
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? ppo_grad_launch<5>(c, b, grad, s) : ppo_grad_launch<7>(c, b, grad, s);
}

int ewn_ppo_apply(const ewn_config *cfg, float *params, float *exp_avg, float *exp_avg_sq, int32_t *step, const float *grad,
                  const ewn_ppo_hyper *hp, float *grad_norm_out, void *stream)
{
    Geom g; KCfg k;
    int rc = a2c_geom(cfg, g, k);
    if (rc) return rc;
    if (!params || !exp_avg || !exp_avg_sq || !step || !grad || !hp) return EWN_ENULL;
    if (hp->world_size < 1) return EWN_EINVAL;
    PpoApplyCfg ac = { (int)ewn_policy_param_count(g.S, g.L), hp->learning_rate, hp->adam_beta1, hp->adam_beta2, hp->adam_eps, hp->max_grad_norm,
                       1.0f / (float)hp->world_size };
    const bool vec = ac.P <= 1024 * 4 * A2C_APPLY_V && ((uintptr_t)params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grad) % 16 == 0;
    if (vec) k_ppo_apply<true><<<1, 1024, 0, (hipStream_t)stream>>>(ac, params, exp_avg, exp_avg_sq, step, grad, grad_norm_out);
    else k_ppo_apply<false><<<1, 1024, 0, (hipStream_t)stream>>>(ac, params, exp_avg, exp_avg_sq, step, grad, grad_norm_out);
    return launch_status();
}

// ---------------------------------------------------------------- the supervised update (targets from outside: a search)

// M is counted in 32-sample tiles by int arithmetic: a grid's worth of tiles past the last one must still fit an int
#define SUP_MAX_M (INT32_MAX - 32 * 4 * (A2C_MAX_BLOCKS + 1))

// scratch (4-byte aligned): partial [256][P] | stats [256][8] | up to 12 bytes of alignment | rows [M][STR] (16-byte aligned)
static size_t sup_rows_offset(int64_t P) { return (size_t)A2C_MAX_BLOCKS * (size_t)(P + 8) * 4; }

int64_t ewn_sup_scratch_bytes(int board_size, int cube_layer, int M)
{
    if (M < 1 || M > SUP_MAX_M) return EWN_EINVAL;
    const int64_t P = ewn_policy_param_count(board_size, cube_layer);
    if (P < 0) return EWN_EUNSUPPORTED;
    return (int64_t)sup_rows_offset(P) + 16 + (int64_t)M * EWN_TRAJ_RECORD_STRIDE(board_size);
}

template <int S>
static int sup_grad_launch(const SupCfg &c, SupBuf b, const int8_t *boards, const int8_t *dice, float *grad, void *scratch, hipStream_t s)
{
    constexpr size_t lds = Sup3Geo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "weight images, the gradient image and the observation stash must fit the CU's LDS");
    constexpr int64_t P = MlpGeo<S>::P;
    b.partial = (float *)scratch;
    b.stats = b.partial + (size_t)A2C_MAX_BLOCKS * P;
    uint8_t *rows = (uint8_t *)(((uintptr_t)scratch + sup_rows_offset(P) + 15) & ~(uintptr_t)15);
    b.rows = rows;
    auto kv = k_sup_grad3<S, 1>;                 // named before k_sup_rows: the unit's kernels keep their order in the code object
    auto kp = k_sup_grad3<S, 0>;
    const size_t words = (size_t)c.M * (RecGeo<S>::STR / 4), need = (words + 255) / 256;
    k_sup_rows<S><<<(unsigned)(need < 65536 ? need : 65536), 256, 0, s>>>(c.M, boards, dice, (u32 *)rows);
    const int blocks = a2c_blocks(c.M, 4);
    return grad3_launch(kv, kp, blocks, lds, c, b, A2cRedBuf{ b.partial, b.stats, grad, blocks, (int)P }, s);
}

int ewn_sup_grad(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const float *target_pi,
                 const float *target_value, const float *weight, const float *params, float pi_coef, float vf_coef, float *grad,
                 void *scratch, void *stream)
{
    if (M < 1 || M > SUP_MAX_M) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (!boards || !dice || !target_pi || !target_value || !params || !grad || !scratch) return EWN_ENULL;
    if (!std::isfinite(pi_coef) || !std::isfinite(vf_coef) || pi_coef < 0.0f || vf_coef < 0.0f) return EWN_EINVAL;
    if (((uintptr_t)scratch & 3) != 0) return EWN_EINVAL;       // partial and stats are float arrays
    const SupCfg c = { M, pi_coef, vf_coef, 1.0f / (float)M };
    SupBuf b;
    memset(&b, 0, sizeof(b));
    b.target_pi = target_pi; b.target_value = target_value; b.weight = weight; b.params = params;
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? sup_grad_launch<5>(c, b, boards, dice, grad, scratch, s) : sup_grad_launch<7>(c, b, boards, dice, grad, scratch, s);
}

int ewn_lookahead_targets(int M, const float *q, float temperature, float *target_pi, float *target_value, float *weight, void *stream)
{
    if (M < 0) return EWN_EINVAL;
    if (M == 0) return EWN_OK;
    if (!q || !target_pi || !target_value || !weight) return EWN_ENULL;
    if (!std::isfinite(temperature) || temperature < 0.0f) return EWN_EINVAL;
    const int need = (M + 255) / 256;
    k_lookahead_targets<<<need < 4096 ? need : 4096, 256, 0, (hipStream_t)stream>>>(M, q, temperature, target_pi, target_value, weight);
    return launch_status();
}
