// ewn_policy_eval.hip -- the evaluation instances of the policy-driven rollout (k_rollout_mlp<S, OPP, NT, 2, RNGK>, ewn_policy.hpp):
// a deterministic policy against RandomAgent or minimax max_depth 1-6 on MT19937-compat or Philox dice, one episode per lane.  The C ABI
// (ewn_policy_eval / ewn_policy_eval_supported) is in ewn_policy.hip; this unit holds the launcher and the kernel instances.
#include "ewn_policy_host.hpp"

template <int S, int OPP, int RNGK, int NT>
static int eval_launch(const PolCfg &pc, const PolBuf &pb, hipStream_t s)
{
    constexpr size_t lds = pol_lds_bytes<S, NT>(false);
    static_assert(lds <= POL_LDS_MAX, "table image + weight image + the block's game slots must fit the CU's LDS");
    return pol_launch_games(k_rollout_mlp<S, OPP, NT, 2, RNGK>, pc.N, NT, lds, s, pc, pb);
}

template <int S, int OPP, int RNGK>
static int eval_by_nt(const PolCfg &pc, const PolBuf &pb, hipStream_t s)
{
    return pol_eval_threads(pc.N) == 64 ? eval_launch<S, OPP, RNGK, 64>(pc, pb, s) : eval_launch<S, OPP, RNGK, 256>(pc, pb, s);
}

template <int S, int OPP>
static int eval_by_rng(const PolCfg &pc, const PolBuf &pb, int rngk, hipStream_t s)
{
    return rngk == EWN_RNG_MT19937 ? eval_by_nt<S, OPP, 0>(pc, pb, s) : eval_by_nt<S, OPP, 1>(pc, pb, s);
}

template <int S>
static int eval_by_opp(const PolCfg &pc, const PolBuf &pb, int opp, int rngk, hipStream_t s)
{
    switch (opp) {
    case 0: return eval_by_rng<S, 0>(pc, pb, rngk, s);
    case 1: return eval_by_rng<S, 1>(pc, pb, rngk, s);
    default: return eval_by_rng<S, 2>(pc, pb, rngk, s);
    }
}

int ewn_launch_policy_eval(const PolCfg &pc, const PolBuf &pb, int S, int opp, int rngk, hipStream_t s)
{
    return S == 5 ? eval_by_opp<5>(pc, pb, opp, rngk, s) : eval_by_opp<7>(pc, pb, opp, rngk, s);
}
