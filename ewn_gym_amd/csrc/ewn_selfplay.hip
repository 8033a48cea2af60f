// ewn_selfplay.hip -- a trained policy against a trained policy (the reference's `A2C.load(opponent_policy)` opponent, envs/ewn.py:265-296),
// K env steps per launch: k_rollout_mlp_vs (ewn_policy.hpp, OPP 3), the rollout form (C ABI: ewn_step_k_selfplay, with the trainer's
// compile-time instance) and the evaluation form (ewn_policy_eval_vs).  A unit of its own for the build's sake (the instances compile in
// parallel); the host plumbing it shares with the other policy units is ewn_policy_host.hpp.
#include "ewn_policy_host.hpp"

// threads per block of the rollout form: 512 (256 games) where the block's LDS fits the CU, else 256, else 0 = no instance
template <int S>
static constexpr int vs_threads(bool want_value)
{
    return pol_lds_bytes<S, 512>(want_value, true) <= POL_LDS_MAX ? 512 : (pol_lds_bytes<S, 256>(want_value, true) <= POL_LDS_MAX ? 256 : 0);
}
// what the byte counts of ewn_mlp3.hpp / ewn_fast.hpp decide: 5x5 keeps 512 threads with two weight images and falls back to 256 with
// the value image (three); 7x7 falls back to 256 threads, and with the value image (three of 51.7 KB) nothing fits
static_assert(vs_threads<5>(false) == 512 && vs_threads<5>(true) == 256, "5x5: 256 games per block with two weight images, 128 with three");
static_assert(vs_threads<7>(false) == 256, "7x7: two weight images + 256 games' slots exceed the CU's LDS, 128 games fit");
static_assert(vs_threads<7>(true) == 0, "7x7 with the value image: three weight images fit no block size");

static int selfplay_plan(const ewn_config *cfg, const Geom &g, bool want_value)
{
    if (!pol_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->rng_kind != EWN_RNG_PHILOX) return EWN_EUNSUPPORTED;
    if ((g.S == 5 ? vs_threads<5>(want_value) : vs_threads<7>(want_value)) == 0) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

static int eval_vs_plan(const ewn_config *cfg, const Geom &g)
{
    if (!pol_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->shaped || cfg->autoreset) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

template <int S, int NT, int TRJ, int RNGK>
static int vs_launch(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    return pol_launch_games(k_rollout_mlp_vs<S, NT, TRJ, RNGK>, pc.N, NT, pol_lds_bytes<S, NT>(pc.want_value != 0, true), s, pc, pb, po);
}

template <int S, bool WV>
static int selfplay_dispatch(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    constexpr int NT = vs_threads<S>(WV);
    if constexpr (NT == 0) return EWN_EUNSUPPORTED;
    else {
        if constexpr (!WV) {
            if (pol_trainer_call(pc, pb) && !po.t_action) return vs_launch<S, NT, 1, 1>(pc, pb, po, s);   // its compile-time instance
        }
        return vs_launch<S, NT, 0, 1>(pc, pb, po, s);
    }
}

int ewn_step_k_selfplay_supported(const ewn_config *cfg, const ewn_policy *pol)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc == EWN_OK) rc = selfplay_plan(&c2, g, pol && pol->value);
    return supported_answer(rc);
}

int ewn_step_k_selfplay(const ewn_config *cfg, const ewn_state *st, int K, const ewn_policy *pol, const ewn_opponent_policy *opp,
                        const ewn_rollout_out *out, void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (pol_state_missing(st, true, c2.shaped != 0) || !pol || !pol->params || !opp || !opp->params) return EWN_ENULL;
    rc = selfplay_plan(&c2, g, pol->value != nullptr);
    if (rc) return rc;
    PolCfg pc = pol_cfg(k, K, pol);
    pc.depth = 0;                                          // no search: the opponent is the network
    const PolBuf pb = pol_buf_rollout(st, st->tables, pol, out);
    const PolOpp po = pol_opp(opp);
    hipStream_t s = (hipStream_t)stream;
    if (pc.want_value) return g.S == 5 ? selfplay_dispatch<5, true>(pc, pb, po, s) : selfplay_dispatch<7, true>(pc, pb, po, s);
    return g.S == 5 ? selfplay_dispatch<5, false>(pc, pb, po, s) : selfplay_dispatch<7, false>(pc, pb, po, s);
}

// ---------------------------------------------------------------- the evaluation (ewn_policy_eval_vs)

template <int S, int RNGK>
static int eval_vs_by_nt(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, hipStream_t s)
{
    static_assert(pol_lds_bytes<S, 256>(false, true) <= POL_LDS_MAX, "table image + two weight images + the block's game slots must fit the CU's LDS");
    return pol_eval_threads(pc.N) == 64 ? vs_launch<S, 64, 2, RNGK>(pc, pb, po, s) : vs_launch<S, 256, 2, RNGK>(pc, pb, po, s);
}

template <int S>
static int eval_vs_by_rng(const PolCfg &pc, const PolBuf &pb, const PolOpp &po, int rngk, hipStream_t s)
{
    return rngk == EWN_RNG_MT19937 ? eval_vs_by_nt<S, 0>(pc, pb, po, s) : eval_vs_by_nt<S, 1>(pc, pb, po, s);
}

int ewn_policy_eval_vs_supported(const ewn_config *cfg)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc == EWN_OK) rc = eval_vs_plan(&c2, g);
    return supported_answer(rc);
}

int ewn_policy_eval_vs(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_opponent_policy *opp,
                       const ewn_rollout_out *out, void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (pol_state_missing(st, true, false) || !params || !opp || !opp->params || !out) return EWN_ENULL;
    rc = pol_eval_out_check(out);
    if (rc) return rc;
    rc = eval_vs_plan(&c2, g);
    if (rc) return rc;
    PolCfg pc = pol_cfg(k, K, nullptr);
    pc.depth = 0;
    PolBuf pb = pol_buf(st, st->tables, params);
    pb.t_action = out->action; fill_totals(pb, out);
    const PolOpp po = pol_opp(opp);
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? eval_vs_by_rng<5>(pc, pb, po, k.rng_kind, s) : eval_vs_by_rng<7>(pc, pb, po, k.rng_kind, s);
}
