// ewn_step_vs.hip -- a trained policy as the env's opponent for ANY agent (the reference's `opponent_policy=<path>` env,
// envs/ewn.py:265-296): k_step_vs (ewn_step_vs.hpp), one step per launch with the caller's actions (C ABI: ewn_step_vs, ewn_step's
// contract) and K steps per launch with a classical agent (ewn_step_k_vs, ewn_step_k's contract).  A unit of its own for the build's
// sake (the instances compile in parallel); the host plumbing it shares with the other policy units is ewn_policy_host.hpp.
#include "ewn_policy_host.hpp"
#include "ewn_step_vs.hpp"

// cube_layer 3 on 5x5 and 7x7, plain or shaped; Philox dice, or MT19937-compat dice without auto-reset (the windows of an auto-resetting
// lane are rebuilt between launches by ewn_step's own machinery, which this kernel does not carry)
static int sv_plan(const ewn_config *cfg, const Geom &g)
{
    if (!pol_geometry(g)) return EWN_EUNSUPPORTED;
    if (cfg->rng_kind == EWN_RNG_MT19937 && cfg->autoreset) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

// AG of k_step_vs for a classical agent; the trained policy as the agent is ewn_step_k_selfplay's, the MCTS agent is not served
static int sv_agent(int agent_kind, int agent_max_depth, int &ag)
{
    if (agent_kind == EWN_AGENT_RANDOM || agent_kind == EWN_AGENT_SAMPLE) { ag = 1; return EWN_OK; }
    if (agent_kind == EWN_AGENT_MINIMAX) {
        if (agent_max_depth < 1) return EWN_EINVAL;
        if (agent_max_depth > EWN_MAX_DEPTH) return EWN_EUNSUPPORTED;
        ag = agent_max_depth > 4 ? 4 : 3;
        return EWN_OK;
    }
    if (agent_kind == EWN_AGENT_MLP || agent_kind == EWN_AGENT_MCTS) return EWN_EUNSUPPORTED;
    return EWN_EINVAL;
}

template <int S, int NT, int AG, int RNGK>
static int sv_launch(const VsCfg &vc, const VsBuf &vb, hipStream_t s)
{
    constexpr size_t lds = pol_lds_bytes<S, NT>(false);
    static_assert(lds <= POL_LDS_MAX, "table image + one weight image + the block's game slots must fit the CU's LDS");
    return pol_launch_games(k_step_vs<S, NT, AG, RNGK>, vc.N, NT, lds, s, vc, vb);
}

template <int S, int AG, int RNGK>
static int sv_by_nt(const VsCfg &vc, const VsBuf &vb, hipStream_t s)
{
    return pol_eval_threads(vc.N) == 64 ? sv_launch<S, 64, AG, RNGK>(vc, vb, s) : sv_launch<S, 256, AG, RNGK>(vc, vb, s);
}

template <int S, int AG>
static int sv_by_rng(const VsCfg &vc, const VsBuf &vb, int rngk, hipStream_t s)
{
    return rngk == EWN_RNG_MT19937 ? sv_by_nt<S, AG, 0>(vc, vb, s) : sv_by_nt<S, AG, 1>(vc, vb, s);
}

template <int AG>
static int sv_by_board(const VsCfg &vc, const VsBuf &vb, int S, int rngk, hipStream_t s)
{
    return S == 5 ? sv_by_rng<5, AG>(vc, vb, rngk, s) : sv_by_rng<7, AG>(vc, vb, rngk, s);
}

static VsCfg sv_cfg(const KCfg &k, int K, const ewn_opponent_policy *opp)
{
    VsCfg vc;
    memset(&vc, 0, sizeof(vc));
    vc.N = k.N; vc.autoreset = k.autoreset; vc.lane_offset = k.lane_offset; vc.K = K;
    vc.shaped = k.shaped; vc.refresh = k.refresh; vc.opp_deterministic = opp->deterministic ? 1 : 0;
    vc.seed_stride = k.seed_stride; vc.W = k.W; vc.reward = k.reward; vc.illegal_reward = k.illegal_reward;
    vc.key = k.key; vc.opp_noise_key = opp->noise_key;
    return vc;
}

static VsBuf sv_buf(const ewn_state *st, const ewn_opponent_policy *opp)
{
    VsBuf vb;
    memset(&vb, 0, sizeof(vb));
    pol_fill_state(vb, st);
    vb.tables = st->tables;
    vb.opp_params = opp->params; vb.o_action = opp->action;
    return vb;
}

int ewn_step_vs_supported(const ewn_config *cfg)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc == EWN_OK) rc = sv_plan(&c2, g);
    return supported_answer(rc);
}

int ewn_step_vs(const ewn_config *cfg, const ewn_state *st, const int8_t *actions, const ewn_opponent_policy *opp, const ewn_step_out *out,
                void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc) return rc;
    if (pol_state_missing(st, true, c2.shaped != 0) || !actions || !opp || !opp->params || !out) return EWN_ENULL;
    if (!out->reward || !out->terminated || !out->truncated || !out->info) return EWN_ENULL;
    if (out->random_action) return EWN_EINVAL;             // RandomAgent.predict fused into the step is ewn_step's (and ewn_step_k_vs plays it)
    rc = sv_plan(&c2, g);
    if (rc) return rc;
    const VsCfg vc = sv_cfg(k, 1, opp);
    VsBuf vb = sv_buf(st, opp);
    vb.actions = actions;
    vb.t_reward = out->reward; vb.t_term = out->terminated; vb.t_trunc = out->truncated; vb.t_info = out->info;
    vb.tboard = out->terminal_board; vb.tdice = out->terminal_dice;
    return sv_by_board<0>(vc, vb, g.S, k.rng_kind, (hipStream_t)stream);
}

int ewn_step_k_vs_supported(const ewn_config *cfg, int agent_kind, int agent_max_depth)
{
    ewn_config c2; Geom g; KCfg k;
    int ag;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc == EWN_OK) rc = sv_agent(agent_kind, agent_max_depth, ag);
    if (rc == EWN_OK) rc = sv_plan(&c2, g);
    return supported_answer(rc);
}

int ewn_step_k_vs(const ewn_config *cfg, const ewn_state *st, int K, int agent_kind, int agent_max_depth, const ewn_opponent_policy *opp,
                  const ewn_rollout_out *out, void *stream)
{
    ewn_config c2; Geom g; KCfg k;
    int ag = 1;
    int rc = pol_check_cfg_blind(cfg, c2, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    rc = sv_agent(agent_kind, agent_max_depth, ag);
    if (rc) return rc;
    if (pol_state_missing(st, true, c2.shaped != 0) || !opp || !opp->params) return EWN_ENULL;
    rc = sv_plan(&c2, g);
    if (rc) return rc;
    VsCfg vc = sv_cfg(k, K, opp);
    vc.agent_depth = agent_max_depth; vc.agent_sample = agent_kind == EWN_AGENT_SAMPLE ? 1 : 0;
    VsBuf vb = sv_buf(st, opp);
    if (ag != 1) vb.tables = fast_image(st->tables, g.S, g.L, agent_max_depth, EWN_H_HYBRID);   // the image of the agent's search
    fill_trajectory(vb, out);
    hipStream_t s = (hipStream_t)stream;
    if (ag == 3) return sv_by_board<3>(vc, vb, g.S, k.rng_kind, s);
    if (ag == 4) return sv_by_board<4>(vc, vb, g.S, k.rng_kind, s);
    return sv_by_board<1>(vc, vb, g.S, k.rng_kind, s);
}
