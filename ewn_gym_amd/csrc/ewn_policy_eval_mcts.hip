// ewn_policy_eval_mcts.hip -- a trained policy against the flat Monte-Carlo opponent, K env steps per launch (C ABI:
// ewn_policy_eval_mcts / ewn_policy_eval_mcts_supported): rollout_mcts_body's third agent (AG 3, ewn_mcts_body.hpp), the actor-critic's
// argmax on the bf16 matrix pipe (ewn_mlp3.hpp) in front of the MCTS opponent's playout phase.  A unit of its own because the matrix
// code is built with -fno-slp-vectorize (build.py FILE_FLAGS, ewn_mlp3.hpp) and ewn_kernels.hip, where the body's other instances
// live, is not.
#include "ewn_mcts_body.hpp"
#include "ewn_policy_host.hpp"

template <int S>
__global__ __launch_bounds__(BS) void k_policy_eval_mcts(Geom g, KCfg c, KState st, MctsRoll mr, RollBuf B, AgentRoll ar)
{
    rollout_mcts_body<3, 2, S>(g, c, st, mr, B, ar);
}

// un-shaped, no auto-reset (one episode per lane), either dice kind, the geometries the actor-critic exists for; the playout numbering
// (root move * total + playout) must fit 32 bits
static int policy_eval_mcts_plan(const ewn_config *cfg, const Geom &g)
{
    if (cfg->opponent_kind != EWN_OPP_MCTS) return EWN_EUNSUPPORTED;
    if (g.L != 3 || (g.S != 5 && g.S != 7)) return EWN_EUNSUPPORTED;
    if (cfg->shaped || cfg->autoreset) return EWN_EUNSUPPORTED;
    if ((long long)cfg->num_simulations * cfg->num_env_copies > 0x7fffffffll / 6) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

template <int S>
static int policy_eval_mcts_launch(const Geom &g, const KCfg &k, const KState &ks, const MctsRoll &mr, const RollBuf &rb, hipStream_t s)
{
    constexpr size_t worst = MctsNet<S>::lds_bytes(MR_GPB, RecGeo<S>::STR);
    static_assert(worst <= 128 * 1024, "boards + weight image + observation slots must fit the CU's LDS beside the body's static arrays");
    const size_t lds = MctsNet<S>::lds_bytes(mr.gpb, mr.strd);
    // A kernel gets 64 KB of LDS by default.  ewn_step_k_agent asks for more above 64 KB of dynamic LDS; here the threshold is 48 KB,
    // so that the body's static arrays (9 616 bytes) never decide whether a launch fits: 7x7 from 32 games per block on is below
    // 64 KB dynamic and above it with them.
    const AgentRoll ar = { 0, 0, 0, 3, 0u, 0ull };
    return pol_launch_kernel(k_policy_eval_mcts<S>, (unsigned)((k.N + mr.gpb - 1) / mr.gpb), BS, lds, 48 * 1024, worst, s, g, k, ks, mr, rb, ar);
}

int ewn_policy_eval_mcts_supported(const ewn_config *cfg)
{
    Geom g; KCfg k;
    int rc = check_cfg(cfg, g, k);
    if (rc == EWN_OK) rc = policy_eval_mcts_plan(cfg, g);   // a configuration check_cfg itself calls unsupported (cube_layer 2) answers 0 too
    return supported_answer(rc);
}

int ewn_policy_eval_mcts(const ewn_config *cfg, const ewn_state *st, int K, const float *params, const ewn_rollout_out *out, void *stream)
{
    Geom g; KCfg k;
    int rc = check_cfg(cfg, g, k);
    if (rc) return rc;
    if (K < 1) return EWN_EINVAL;
    if (pol_state_missing(st, false, false) || !params || !out) return EWN_ENULL;    // the MCTS opponent reads no table image
    rc = pol_eval_out_check(out);
    if (rc) return rc;
    rc = policy_eval_mcts_plan(cfg, g);
    if (rc) return rc;
    RollBuf rb;
    memset(&rb, 0, sizeof(rb));
    rb.agent_tables = params;   // the agent's image: AG 3 has no search table, the body packs the actor-critic's parameters from here
    rb.t_action = out->action; fill_totals(rb, out);
    // games per block: ewn_step_k_agent's rule for its MCTS-only instances (8 .. MR_GPB, about 2 048 blocks)
    int gpb = 8;
    while (gpb < MR_GPB && (long long)k.N / (2 * gpb) >= 2048) gpb *= 2;
    const MctsRoll mr = { K, k.nsim_total, playout_group_log2(k.nsim_total), 0, (g.cells + 6 + 15) & ~15, gpb };
    const KState ks = { st->board, st->dice, st->done, st->rng, nullptr, nullptr, nullptr };
    hipStream_t s = (hipStream_t)stream;
    return g.S == 5 ? policy_eval_mcts_launch<5>(g, k, ks, mr, rb, s) : policy_eval_mcts_launch<7>(g, k, ks, mr, rb, s);
}
