// ewn_selfplay.hip -- a trained policy against a trained policy (the reference's `A2C.load(opponent_policy)` opponent, envs/ewn.py:265-296),
// K env steps per launch: k_rollout_mlp_vs (ewn_policy.hpp, OPP 3), the rollout form (C ABI: ewn_step_k_selfplay, with the trainer's
// compile-time instance) and the evaluation form (ewn_policy_eval_vs).  A unit of its own: the existing instances of the body stay in
// ewn_policy.hip / ewn_policy_eval.hip and compile to the code they were.
#include "ewn_host.hpp"
#include "ewn_lds.hpp"
#include "ewn_policy.hpp"

#define VS_LDS_MAX (160 * 1024)

// threads per block of the rollout form: 512 (256 games) where the block's LDS fits the CU, else 256, else 0 = no instance
template <int S>
static constexpr int vs_threads(bool want_value)
{
    return pol_lds_bytes<S, 512>(want_value, true) <= VS_LDS_MAX ? 512 : (pol_lds_bytes<S, 256>(want_value, true) <= VS_LDS_MAX ? 256 : 0);
}
// what the byte counts of ewn_mlp3.hpp / ewn_fast.hpp decide: 5x5 keeps 512 threads with two weight images and falls back to 256 with
// the value image (three); 7x7 falls back to 256 threads, and with the value image (three of 51.7 KB) nothing fits
static_assert(vs_threads<5>(false) == 512 && vs_threads<5>(true) == 256, "5x5: 256 games per block with two weight images, 128 with three");
static_assert(vs_threads<7>(false) == 256, "7x7: two weight images + 256 games' slots exceed the CU's LDS, 128 games fit");
static_assert(vs_threads<7>(true) == 0, "7x7 with the value image: three weight images fit no block size");

// the configurations the calls serve; the opponent fields of cfg are not read (the copy handed to check_cfg names RandomAgent)
static int vs_check(const ewn_config *cfg, ewn_config &c2, Geom &g, KCfg &k)
{
    if (!cfg) return EWN_ENULL;
    c2 = *cfg;
    c2.opponent_kind = EWN_OPP_RANDOM; c2.max_depth = 1; c2.heuristic = EWN_H_HYBRID; c2.num_simulations = 1; c2.num_env_copies = 1;
    return check_cfg(&c2, g, k);
}

static int vs_geometry(const Geom &g)
{
    return (fast_tables_bytes(g.S, g.L) <= 0 || (g.S != 5 && g.S != 7)) ? EWN_EUNSUPPORTED : EWN_OK;
}

static int selfplay_plan(const ewn_config *cfg, const Geom &g, bool want_value)
{
    if (vs_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->rng_kind != EWN_RNG_PHILOX) return EWN_EUNSUPPORTED;
    if ((g.S == 5 ? vs_threads<5>(want_value) : vs_threads<7>(want_value)) == 0) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

static int eval_vs_plan(const ewn_config *cfg, const Geom &g)
{
    if (vs_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->shaped || cfg->autoreset) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

template <int S, int NT, int TRJ, int RNGK>
static int vs_launch(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    auto kern = k_rollout_mlp_vs<S, NT, TRJ, RNGK>;
    const size_t lds = pol_lds_bytes<S, NT>(pc.want_value != 0, true);
    if (lds > VS_LDS_MAX) return EWN_EUNSUPPORTED;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, VS_LDS_MAX) != hipSuccess) return EWN_ELAUNCH;
    constexpr int gpb = NT / 2;
    kern<<<dim3((unsigned)((pc.N + gpb - 1) / gpb)), NT, lds, s>>>(pc, pb, po);
    return launch_status();
}

template <int S, bool WV>
static int selfplay_dispatch(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    constexpr int NT = vs_threads<S>(WV);
    if constexpr (NT == 0) return EWN_EUNSUPPORTED;
    else {
        if constexpr (!WV) {
            // the trainer's call (see pol_launch in ewn_policy.hip): its compile-time instance
            const bool trainer = pb.t_rec && pb.t_reward && pc.rec0 && !pc.deterministic && !pb.t_board && !pb.t_dice && !pb.t_action
                                 && !pb.t_term && !pb.t_trunc && !pb.t_info && !pb.t_logits && !pb.t_noise && !po.t_action;
            if (trainer) return vs_launch<S, NT, 1, 1>(pc, pb, po, s);
        }
        return vs_launch<S, NT, 0, 1>(pc, pb, po, s);
    }
}

int ewn_step_k_selfplay_supported(const ewn_config *cfg, const ewn_policy *pol)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = vs_check(cfg, c2, g, k);
    if (rc == EWN_OK) rc = selfplay_plan(&c2, g, pol && pol->value);
    return rc == EWN_OK ? 1 : (rc == EWN_EUNSUPPORTED ? 0 : rc);
}

int ewn_step_k_selfplay(const ewn_config *cfg, const ewn_state *st, int K, const ewn_policy *pol, const ewn_opponent_policy *opp,
                        const ewn_rollout_out *out, void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = vs_check(cfg, c2, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (!st || !st->board || !st->dice || !st->done || !st->rng || !st->tables || !pol || !pol->params || !opp || !opp->params) return EWN_ENULL;
    if (c2.shaped && (!st->prev_score || !st->tolerance)) return EWN_ENULL;
    rc = selfplay_plan(&c2, g, pol->value != nullptr);
    if (rc) return rc;
    PolCfg pc;
    pc.N = k.N; pc.autoreset = k.autoreset; pc.lane_offset = k.lane_offset; pc.depth = 0; pc.K = K;
    pc.shaped = k.shaped; pc.refresh = k.refresh; pc.deterministic = pol->deterministic ? 1 : 0; pc.want_value = pol->value ? 1 : 0;
    pc.rec0 = pol->record_initial_obs ? 1 : 0;
    pc.seed_stride = k.seed_stride; pc.W = k.W; pc.reward = k.reward; pc.illegal_reward = k.illegal_reward;
    pc.key = k.key; pc.noise_key = pol->noise_key;
    PolBuf pb;
    memset(&pb, 0, sizeof(pb));
    pb.board = st->board; pb.dice = st->dice; pb.done = st->done; pb.rng = st->rng; pb.prev_score = st->prev_score; pb.tolerance = st->tolerance;
    pb.tables = st->tables;
    pb.params = pol->params;
    pb.t_logits = pol->logits; pb.t_value = pol->value; pb.t_noise = pol->noise;
    if (out) {
        pb.t_board = out->board; pb.t_dice = out->dice; pb.t_action = out->action; pb.t_reward = out->reward;
        pb.t_term = out->terminated; pb.t_trunc = out->truncated; pb.t_info = out->info; pb.t_rec = out->record;
        pb.ret_sum = out->return_sum; pb.n_steps = out->n_steps; pb.n_episodes = out->n_episodes; pb.n_wins = out->n_wins;
    }
    const PolOpp po = { opp->params, opp->action, opp->noise_key, opp->deterministic ? 1 : 0 };
    hipStream_t s = (hipStream_t)stream;
    if (pc.want_value) return g.S == 5 ? selfplay_dispatch<5, true>(pc, pb, po, s) : selfplay_dispatch<7, true>(pc, pb, po, s);
    return g.S == 5 ? selfplay_dispatch<5, false>(pc, pb, po, s) : selfplay_dispatch<7, false>(pc, pb, po, s);
}

// ---------------------------------------------------------------- the evaluation (ewn_policy_eval_vs)

// ewn_policy_eval's rule (ewn_policy_eval.hip): one wave per block up to 8 192 games, 256 threads beyond; EWN_EVAL_NT overrides it
static int eval_vs_threads(int n_games)
{
    static const int forced = [] { const char *e = getenv("EWN_EVAL_NT"); return e ? atoi(e) : 0; }();
    if (forced == 64 || forced == 256) return forced;
    return n_games <= 8192 ? 64 : 256;
}

template <int S, int RNGK>
static int eval_vs_by_nt(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    static_assert(pol_lds_bytes<S, 256>(false, true) <= VS_LDS_MAX, "table image + two weight images + the block's game slots must fit the CU's LDS");
    return eval_vs_threads(pc.N) == 64 ? vs_launch<S, 64, 2, RNGK>(pc, pb, po, s) : vs_launch<S, 256, 2, RNGK>(pc, pb, po, s);
}

template <int S>
static int eval_vs_by_rng(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, int rngk, hipStream_t s)
{
    return rngk == EWN_RNG_MT19937 ? eval_vs_by_nt<S, 0>(pc, pb, po, s) : eval_vs_by_nt<S, 1>(pc, pb, po, s);
}

int ewn_policy_eval_vs_supported(const ewn_config *cfg)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = vs_check(cfg, c2, g, k);
    if (rc == EWN_OK) rc = eval_vs_plan(&c2, g);
    return rc == EWN_OK ? 1 : (rc == EWN_EUNSUPPORTED ? 0 : rc);
}

int ewn_policy_eval_vs(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_opponent_policy *opp,
                       const ewn_rollout_out *out, void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = vs_check(cfg, c2, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (!st || !st->board || !st->dice || !st->done || !st->rng || !st->tables || !params || !opp || !opp->params || !out) return EWN_ENULL;
    if (!out->return_sum || !out->n_steps || !out->n_episodes || !out->n_wins) return EWN_ENULL;
    if (out->board || out->dice || out->reward || out->terminated || out->truncated || out->info || out->record) return EWN_EINVAL;
    rc = eval_vs_plan(&c2, g);
    if (rc) return rc;
    PolCfg pc;
    memset(&pc, 0, sizeof(pc));
    pc.N = k.N; pc.lane_offset = k.lane_offset; pc.K = K;
    pc.deterministic = 1;
    pc.seed_stride = k.seed_stride; pc.W = k.W; pc.reward = k.reward; pc.illegal_reward = k.illegal_reward; pc.key = k.key;
    PolBuf pb;
    memset(&pb, 0, sizeof(pb));
    pb.board = st->board; pb.dice = st->dice; pb.done = st->done; pb.rng = st->rng;
    pb.tables = st->tables;
    pb.params = params;
    pb.t_action = out->action;
    pb.ret_sum = out->return_sum; pb.n_steps = out->n_steps; pb.n_episodes = out->n_episodes; pb.n_wins = out->n_wins;
    const PolOpp po = { opp->params, opp->action, opp->noise_key, opp->deterministic ? 1 : 0 };
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? eval_vs_by_rng<5>(pc, pb, po, k.rng_kind, s) : eval_vs_by_rng<7>(pc, pb, po, k.rng_kind, s);
}
