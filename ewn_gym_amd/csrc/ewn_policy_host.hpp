// ewn_policy_host.hpp -- the host plumbing the policy units share (ewn_policy.hip, ewn_policy_eval.hip, ewn_policy_eval_mcts.hip,
// ewn_selfplay.hip, ewn_step_vs.hip, ewn_predict_policy.hip): limits, configuration and argument checks, the fillers of the kernel
// argument structs and the launch tail.  Building blocks, not a validator: every entry point calls them in its own order, and that
// order of refusals is part of its contract (tests/test_policy_host_cpu.py).  Host code only: nothing here enters a device object.
#pragma once
#include "ewn_host.hpp"
#include "ewn_lds.hpp"
#include "ewn_policy.hpp"

#define POL_LDS_MAX (160 * 1024)   // the CU's LDS: what a block of any policy kernel may ask for

// the geometries the actor-critic and its table images exist for: cube_layer 3 on 5x5 and 7x7
static inline bool pol_geometry(const Geom &g) { return fast_tables_bytes(g.S, g.L) > 0 && (g.S == 5 || g.S == 7); }

// Threads per block of the evaluation kernels and of k_step_vs by lane count.  An evaluation is small (20 .. 1 024 games) and its step
// is one wave's latency chain (network, then the opponent's search), so the waves are spread one per CU while that is possible:
// 64 threads = 32 games per block up to 8 192 games (256 blocks), 256 threads beyond.  EWN_EVAL_NT (64 / 256) overrides it (tuning;
// DESIGN.md has the measurements); read once per process.
inline int pol_eval_threads(int n_games)
{
    static const int forced = [] { const char *e = getenv("EWN_EVAL_NT"); return e ? atoi(e) : 0; }();
    if (forced == 64 || forced == 256) return forced;
    return n_games <= 8192 ? 64 : 256;
}

// check_cfg for the calls whose opponent is a policy network: the opponent fields of cfg are not read (the copy handed to check_cfg,
// and left in c2 for the caller's plan, names RandomAgent)
static inline int pol_check_cfg_blind(const ewn_config *cfg, ewn_config &c2, Geom &g, KCfg &k)
{
    if (!cfg) return EWN_ENULL;
    c2 = *cfg;
    c2.opponent_kind = EWN_OPP_RANDOM; c2.max_depth = 1; c2.heuristic = EWN_H_HYBRID; c2.num_simulations = 1; c2.num_env_copies = 1;
    return check_cfg(&c2, g, k);
}

// a NULL among the members of the state that a call reads (-> EWN_ENULL); shaped: the shaped env's prev_score / tolerance as well
static inline bool pol_state_missing(const ewn_state *st, bool need_tables, bool shaped)
{
    if (!st || !st->board || !st->dice || !st->done || !st->rng || (need_tables && !st->tables)) return true;
    return shaped && (!st->prev_score || !st->tolerance);
}

// the `out` of an evaluation call (not NULL): the four totals, optionally the action column, no other trajectory column
static inline int pol_eval_out_check(const ewn_rollout_out *out)
{
    if (!out->return_sum || !out->n_steps || !out->n_episodes || !out->n_wins) return EWN_ENULL;
    if (out->board || out->dice || out->reward || out->terminated || out->truncated || out->info || out->record) return EWN_EINVAL;
    return EWN_OK;
}

// pol NULL: an evaluation -- deterministic, un-shaped, no auto-reset, no policy outputs
static inline PolCfg pol_cfg(const KCfg &k, int K, const ewn_policy *pol)
{
    PolCfg pc;
    memset(&pc, 0, sizeof(pc));
    pc.N = k.N; pc.lane_offset = k.lane_offset; pc.depth = k.depth; pc.K = K;
    pc.seed_stride = k.seed_stride; pc.W = k.W; pc.reward = k.reward; pc.illegal_reward = k.illegal_reward; pc.key = k.key;
    pc.deterministic = 1;
    if (pol) {
        pc.autoreset = k.autoreset; pc.shaped = k.shaped; pc.refresh = k.refresh;
        pc.deterministic = pol->deterministic ? 1 : 0; pc.want_value = pol->value ? 1 : 0; pc.rec0 = pol->record_initial_obs ? 1 : 0;
        pc.noise_key = pol->noise_key;
    }
    return pc;
}

// the filler of a zeroed kernel argument struct's state: PolBuf and VsBuf carry the same field names; `tables` is the caller's.
// (The trajectory and the totals: fill_trajectory / fill_totals, ewn_host.hpp.)
template <class Buf>
static inline void pol_fill_state(Buf &b, const ewn_state *st)
{
    b.board = st->board; b.dice = st->dice; b.done = st->done; b.rng = st->rng; b.prev_score = st->prev_score; b.tolerance = st->tolerance;
}

static inline PolBuf pol_buf(const ewn_state *st, const void *tables, const float *params)
{
    PolBuf pb;
    memset(&pb, 0, sizeof(pb));
    pol_fill_state(pb, st);
    pb.tables = tables;
    pb.params = params;
    return pb;
}

// a rollout's buffers: the state, the policy's own outputs and the caller's trajectory
static inline PolBuf pol_buf_rollout(const ewn_state *st, const void *tables, const ewn_policy *pol, const ewn_rollout_out *out)
{
    PolBuf pb = pol_buf(st, tables, pol->params);
    pb.t_logits = pol->logits; pb.t_value = pol->value; pb.t_noise = pol->noise;
    fill_trajectory(pb, out);
    return pb;
}

static inline PolOpp pol_opp(const ewn_opponent_policy *opp)
{
    return PolOpp{ opp->params, opp->action, opp->noise_key, opp->deterministic ? 1 : 0 };
}

// the trainer's call (FusedA2CTrainer): records from the initial observation on + the reward column, nothing else per step, sampled
// actions, no value output -- what the TRJ 1 instances know at compile time
static inline bool pol_trainer_call(const PolCfg &pc, const PolBuf &pb)
{
    return pb.t_rec && pb.t_reward && pc.rec0 && !pc.want_value && !pc.deterministic && !pb.t_board && !pb.t_dice && !pb.t_action
           && !pb.t_term && !pb.t_trunc && !pb.t_info && !pb.t_logits && !pb.t_value && !pb.t_noise;
}

// The launch tail.  A kernel gets 64 KB of dynamic LDS by default; above `optin_above` bytes the launch first asks for `optin_bytes`.
// Asked per launch: the attribute belongs to the current device's copy of the kernel, and a process may drive several devices.
template <class Kern, class... Args>
static inline int pol_launch_kernel(Kern kern, unsigned blocks, unsigned threads, size_t lds, size_t optin_above, size_t optin_bytes, hipStream_t s,
                                    const Args &...args)
{
    if (lds > optin_above && hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)optin_bytes) != hipSuccess)
        return EWN_ELAUNCH;
    kern<<<dim3(blocks), dim3(threads), lds, s>>>(args...);
    return launch_status();
}

// the policy kernels' own: two lanes per game, NT / 2 games per block, the CU's LDS asked for above the default; a block that would
// need more than the CU has is not served
template <class Kern, class... Args>
static inline int pol_launch_games(Kern kern, int n_games, int NT, size_t lds, hipStream_t s, const Args &...args)
{
    if (lds > POL_LDS_MAX) return EWN_EUNSUPPORTED;
    const int gpb = NT / 2;
    return pol_launch_kernel(kern, (unsigned)((n_games + gpb - 1) / gpb), (unsigned)NT, lds, 64 * 1024, POL_LDS_MAX, s, args...);
}
