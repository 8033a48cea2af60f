// ewn_host.hpp -- host-side pieces shared by the translation units of libewn_hip.so: kernel argument structs, geometry and
// configuration checks, and the launchers each unit exports to the C ABI in ewn_kernels.hip.
#pragma once
#include "ewn_core.hpp"
#include "ewn_fast.hpp"
#include "../../include/ewn_hip.h"
#include <cstdlib>

#define D3_BS 256 // threads per block of the lean step / rollout kernels

struct KCfg {
    int N, opp, depth, heur, rng_kind, shaped, autoreset, refresh, lane_offset, nsim_total;
    u32 seed_stride, W, rng_words;
    double reward, illegal_reward;
    u64 key;
};

struct KState {
    int8_t *board; int8_t *dice; uint8_t *done; u32 *rng; double *prev_score; int32_t *tolerance; const void *tables;
};

struct KOut {
    double *reward; uint8_t *terminated; uint8_t *truncated; uint8_t *info; int8_t *tboard; int8_t *tdice; int8_t *ract;
};

struct KScratch { // split-phase step (MCTS opponent)
    uint8_t *phase; int8_t *cboard; int8_t *cdice; int8_t *act; int32_t *wins; u32 *obs_id;
};

static inline bool make_geom(int S, int L, Geom &g)
{
    if (S < 3 || S > EWN_MAX_BOARD || L < 1 || L >= S - 1) return false; // assert cube_layer < board_size - 1, envs/ewn.py:47
    const int CN = L * (L + 1) / 2;
    if (CN > EWN_MAX_CUBES) return false;
    g.S = S; g.L = L; g.CN = CN; g.cells = S * S;
    g.div_magic = 65536u / (u32)S + 1u;
    g.not_lastcol = g.not_lastrow = g.not_firstcol = g.not_firstrow = 0;
    for (int t = 0; t < 8; t++) g.sq[t] = 0;
    const bool wide = S > 8; // 9x9 .. 11x11: no 64-bit masks, 7-bit positions nine per word (ewn_core.hpp GState<3>)
    if (!wide)
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                const u64 b = 1ull << (i * S + j);
                if (j < S - 1) g.not_lastcol |= b;
                if (i < S - 1) g.not_lastrow |= b;
                if (j > 0) g.not_firstcol |= b;
                if (i > 0) g.not_firstrow |= b;
                for (int t = 0; t < S; t++) if (i >= t && j >= t) g.sq[t] |= b;
            }
    g.corner_br = wide ? 0 : 1ull << (S * S - 1);
    for (int c = 0; c < 128; c++) g.init[c] = 0;
    int cnt = 1;
    for (int i = 1; i <= L; i++)
        for (int j = 0; j < i; j++) {
            g.init[j * S + (i - j - 1)] = (int8_t)cnt;
            g.init[(S - 1 - j) * S + (S - i + j)] = (int8_t)(-cnt);
            cnt++;
        }
    g.init_occP = g.init_occN = 0; g.init_alive = 0;
    for (int w = 0; w < 3; w++) g.init_posP[w] = g.init_posN[w] = 0;
    const int per = wide ? 9 : 10, bits = wide ? 7 : 6;
    for (int c = 0; c < S * S; c++) {
        const int v = g.init[c];
        if (v > 0) { if (!wide) g.init_occP |= 1ull << c; g.init_alive |= 1u << (v - 1); g.init_posP[(v - 1) / per] |= (u64)c << (bits * ((v - 1) % per)); }
        if (v < 0) { if (!wide) g.init_occN |= 1ull << c; g.init_posN[(-v - 1) / per] |= (u64)c << (bits * ((-v - 1) % per)); }
    }
    return true;
}

static inline int check_cfg(const ewn_config *cfg, Geom &g, KCfg &k)
{
    if (!cfg) return EWN_ENULL;
    if (cfg->board_size > EWN_MAX_BOARD && cfg->cube_layer >= 1 && cfg->cube_layer < cfg->board_size - 1) return EWN_EUNSUPPORTED;
    if (!make_geom(cfg->board_size, cfg->cube_layer, g)) return EWN_EINVAL;
    if (cfg->n_lanes < 1) return EWN_EINVAL;
    if (cfg->opponent_kind < 0 || cfg->opponent_kind > EWN_OPP_MCTS) return EWN_EINVAL;
    if (cfg->rng_kind != EWN_RNG_MT19937 && cfg->rng_kind != EWN_RNG_PHILOX) return EWN_EINVAL;
    if (cfg->opponent_kind == EWN_OPP_MINIMAX) {
        if (cfg->max_depth < 1 || cfg->max_depth > EWN_MAX_DEPTH) return EWN_EUNSUPPORTED;
        if (cfg->heuristic < 0 || cfg->heuristic > EWN_H_SIM_WINRATE) return EWN_EUNSUPPORTED;
        if (cfg->heuristic == EWN_H_SIM_WINRATE && cfg->max_depth > EWN_SIM_WINRATE_MAX_DEPTH) return EWN_EUNSUPPORTED;
    }
    // the searches and rollouts roll dice 1..6 (minimax.py:68, mcts.py:29): cube_num < 6 raises IndexError upstream
    if (cfg->opponent_kind != EWN_OPP_RANDOM && g.CN < 6) return EWN_EUNSUPPORTED;
    if (cfg->opponent_kind == EWN_OPP_MCTS && (cfg->num_simulations < 1 || cfg->num_env_copies < 1)) return EWN_EINVAL;
    u32 W = cfg->mt_window ? cfg->mt_window : 128u;
    if (W < 16 || W > EWN_MT_WINDOW_MAX) return EWN_EINVAL;
    k.N = cfg->n_lanes; k.opp = cfg->opponent_kind; k.depth = cfg->max_depth; k.heur = cfg->heuristic;
    k.rng_kind = cfg->rng_kind; k.shaped = cfg->shaped; k.autoreset = cfg->autoreset; k.refresh = cfg->shaped_refresh_on_reset;
    k.lane_offset = cfg->lane_offset; k.nsim_total = cfg->num_simulations * cfg->num_env_copies;
    k.seed_stride = cfg->seed_stride; k.W = W;
    k.rng_words = EWN_RNG_HDR + (cfg->rng_kind == EWN_RNG_MT19937 ? 3u * W + 1u : 0u);
    k.reward = cfg->reward; k.illegal_reward = cfg->illegal_move_reward; k.key = cfg->philox_key;
    return EWN_OK;
}

static inline int launch_status()
{
    return hipGetLastError() == hipSuccess ? EWN_OK : EWN_ELAUNCH;
}

// the answer of an ewn_*_supported call from a plan's code: 1 served, 0 not served, a negative code for a malformed configuration
static inline int supported_answer(int rc) { return rc == EWN_OK ? 1 : (rc == EWN_EUNSUPPORTED ? 0 : rc); }

// the fillers of a zeroed kernel argument struct (RollBuf, PolBuf, VsBuf: the same field names) from the caller's ewn_rollout_out.
// An evaluation writes the totals and optionally the action column, nothing else.
template <class Buf>
static inline void fill_totals(Buf &b, const ewn_rollout_out *out)
{
    b.ret_sum = out->return_sum; b.n_steps = out->n_steps; b.n_episodes = out->n_episodes; b.n_wins = out->n_wins;
}

// every column of a rollout's `out` (which may be NULL: nothing is written then) and the totals
template <class Buf>
static inline void fill_trajectory(Buf &b, const ewn_rollout_out *out)
{
    if (!out) return;
    b.t_board = out->board; b.t_dice = out->dice; b.t_action = out->action; b.t_reward = out->reward;
    b.t_term = out->terminated; b.t_trunc = out->truncated; b.t_info = out->info; b.t_rec = out->record;
    fill_totals(b, out);
}

// bytes per game of the LDS staging area of the one-thread-per-game K-step kernels: a record of ewn_rollout_out.record (or a board)
static inline int traj_record_stride(const Geom &g) { return EWN_TRAJ_RECORD_STRIDE(g.S); }

// SV = the board size of a table-driven kernel instance as a compile-time constant, in the style of BY_NW.  Serves the sizes with a
// table image, 5 .. 8: every caller has established fast_tables_bytes(S, L) > 0 first, so the last case takes what is left.
#define BY_S(S, X) do { switch (S) { case 5: { constexpr int SV = 5; X; } break; case 6: { constexpr int SV = 6; X; } break; \
                                     case 7: { constexpr int SV = 7; X; } break; default: { constexpr int SV = 8; X; } break; } } while (0)

// specialised depth-3 tables exist for cube_layer 3 and board sizes whose distinct leaf values fit 10-bit ranks
static inline int64_t fast_tables_bytes(int S, int L)
{
    if (L != 3 || S < 5 || S > 8) return 0;
    int64_t bytes = 0;
    BY_S(S, bytes = (int64_t)FAST_TAB_BYTES(SV));
    return bytes;
}

// table image of a search with the given heuristic and max_depth: max_depth 4 and 6 read the image's second variant (leaves
// averaged over six dice); NULL for a heuristic without images
static inline const void *fast_image(const void *tables, int S, int L, int max_depth, int heur = EWN_H_HYBRID)
{
    const int hi = fast_heur_image(heur);
    if (!tables || hi < 0) return nullptr;
    return (const int8_t *)tables + (size_t)(hi * 2 + ((max_depth == 4 || max_depth == 6) ? 1 : 0)) * fast_tables_bytes(S, L);
}

// Lanes of one wavefront that share a game in k_step_d3: enough to put several waves on every SIMD
// (1024 SIMDs x 64 lanes) at the given number of games.  EWN_D3_T=0 disables the kernel, 1 / 2 forces T.
static inline int d3_threads_per_game(int n_games)
{
    static const int forced = [] { const char *e = getenv("EWN_D3_T"); return e ? atoi(e) : -1; }();
    if (forced == 0 || forced == 1 || forced == 2) return forced;
    // measured on MI355X (tools/sweep_T.sh, us per step, T = 1 / 2 / 4): 16 384 games 14.9 / 10.9 / 10.0; 32 768: 15.1 / 11.3 / 12.6;
    // 65 536: 15.8 / 14.8 / 18.7; 131 072: 21.6 / 22.4 / 32.3; 262 144: 36.3 / 39.4 / 57.5; 1 048 576: 118 / 132 / 205.
    // The kernel is bound by integer VALU issue once the chip is full, so lanes added beyond what hides the LDS/global
    // latency only add redundant instructions.
    // Re-measured at the end of round 2 (table-driven setup, one-min pair selection): two lanes per game are now as fast as or faster
    // than four at every lane count below 131 072 (2 048 .. 24 576 games: one-step launch 9.9-10.4 us against 10.1-12.1), so the
    // four-lanes-per-game instances were dropped from the library, and later the T = 4 code of d3_search and its helpers with them.
    if (n_games >= 131072) return 1;
    return 2;
}

// the lean kernel's MT refill hand-off (ewn_core.hpp MtQueue): ctrl[4] | cnt[2][nb4] | list[2][nblk][2 * games per block] x 16 B.
// The layout depends on the lanes-per-game T the launch picks (games per block = 256 / T, nblk = ceil(N / games per block)), and
// the rounding-up of nblk makes T = 1 the LARGEST for a small N (64 lanes: one block of 512 slots), so take the maximum over T.
// (Sizing it for T = 4 only let a T = 1 launch on 64 lanes write 8 KB past the buffer -- into whatever tensor came next.)
static inline int64_t mtq_bytes(int64_t N)
{
    int64_t best = 0;
    for (int T = 1; T <= 4; T *= 2) {
        const int64_t gpb = D3_BS / T, nblk = (N + gpb - 1) / gpb, nb4 = (nblk + 3) / 4 * 4;
        const int64_t b = 16 + 2 * nb4 * 4 + 2 * nblk * (2 * gpb) * 16;
        if (b > best) best = b;
    }
    return best;
}


// the same choice for the K-step rollout kernel (ewn_rollout.hpp), whose per-step cost outside the search is much smaller
static inline int rollout_threads_per_game(int n_games)
{
    static const int forced = [] { const char *e = getenv("EWN_ROLLOUT_T"); return e ? atoi(e) : -1; }();
    if (forced == 1 || forced == 2) return forced;
    // measured (us per step with the trajectory, T = 2 / 4): 2 048 games 6.46 / 6.93, 8 192: 6.56 / 7.11, 24 576: 6.79 / 8.45
    if (n_games >= 131072) return 1;
    return 2;
}

// The MT19937-compat windows of an auto-resetting lane are rebuilt BETWEEN launches (ewn_core.hpp): ewn_step queues refills for
// them, and a launch that plays several episodes of a lane (every K-step kernel) cannot use the kind -- it is refused there.
// Without auto-reset (one episode per lane: evaluation) the kind is fine everywhere.
static inline bool mt_autoreset(const ewn_config *cfg) { return cfg->rng_kind == EWN_RNG_MT19937 && cfg->autoreset; }

// What ewn_step launches for a configuration: the ONE place that decides it.  ewn_step, ewn_step_scratch_bytes (which path needs
// which scratch), ewn_lanes_per_game(cfg, 0) (what the tests assert kernel families through) and the lean kernel's launcher
// (ewn_step_d3_tu.inc) all read it.
//   STEP_SPLIT        the opponent's policy runs as kernels of its own between two half steps (MCTS, minimax 'sim_winrate')
//   STEP_LEAN_TABLES  k_step_d3, T lanes per game, table-driven search (the 'two_min_dist' image: ewn_step_d3_h2.hip's instances)
//   STEP_LEAN_RANDOM  k_step_d3 against RandomAgent, one lane per game
//   STEP_TABLES       k_step<1, 0, S>: one thread per game, the search from a table image (EWN_D3_T=0)
//   STEP_GENERIC      k_step<NW, 0, 0>: any geometry, RandomAgent or the template-recursive search
// have_tables: the caller's state carries the table images (ewn_state.tables); a query without a state assumes it does.
enum StepPath { STEP_SPLIT, STEP_LEAN_TABLES, STEP_LEAN_RANDOM, STEP_TABLES, STEP_GENERIC };
struct StepPlan { StepPath path; int T; };   // T: lanes per game of the lean kernel, 0 on the other paths

static inline StepPlan step_plan(const ewn_config *cfg, const Geom &g, const KCfg &k, bool have_tables)
{
    if (cfg->opponent_kind == EWN_OPP_MCTS || (cfg->opponent_kind == EWN_OPP_MINIMAX && cfg->heuristic == EWN_H_SIM_WINRATE)) return { STEP_SPLIT, 0 };
    const bool tab = have_tables && fast_tables_bytes(g.S, g.L) > 0;
    // the one-thread-per-game kernel searches any table image; the lean kernel only those with instances of it (fast_heur_step)
    const bool fast = tab && cfg->opponent_kind == EWN_OPP_MINIMAX && cfg->max_depth <= 6 && fast_heur_image(cfg->heuristic) >= 0;
    const int T3 = d3_threads_per_game(k.N);
    if (T3 > 0 && tab && cfg->opponent_kind == EWN_OPP_RANDOM) return { STEP_LEAN_RANDOM, 1 };
    if (T3 > 0 && fast && fast_heur_step(cfg->heuristic)) {
        // leaves are shared among lanes at depth 3-4; depth 5-6 splits its inner dice over two lanes while the chip is not full
        const int T = cfg->max_depth < 3 ? 1 : (cfg->max_depth > 4 ? (k.N <= 131072 && T3 != 1 ? 2 : 1) : T3);
        return { STEP_LEAN_TABLES, T };
    }
    return { fast ? STEP_TABLES : STEP_GENERIC, 0 };
}

// what every entry point that plays games needs of the caller's state; with the table images; the shaped-reward columns
static inline bool state_ok(const ewn_state *st) { return st && st->board && st->dice && st->done && st->rng; }
static inline bool state_tables_ok(const ewn_state *st) { return state_ok(st) && st->tables; }
static inline bool shaped_ok(const ewn_config *cfg, const ewn_state *st) { return !cfg->shaped || (st->prev_score && st->tolerance); }

// ewn_step_d3.hip: the lean table-driven step kernel (one launch = one env step); plan: step_plan's STEP_LEAN_* answer
int ewn_launch_step_d3(const ewn_config *cfg, const Geom &g, const KCfg &k, const ewn_state *st, const void *tables, const int8_t *actions,
                       const ewn_step_out *out, void *scratch, const StepPlan &plan, bool fused_refill, hipStream_t s);
// ewn_step_d3_h2.hip: the same for the 'two_min_dist' table image
int ewn_launch_step_d3_h2(const ewn_config *cfg, const Geom &g, const KCfg &k, const ewn_state *st, const void *tables, const int8_t *actions,
                          const ewn_step_out *out, void *scratch, const StepPlan &plan, bool fused_refill, hipStream_t s);

// ewn_rollout_s<S>.hip: K env steps per launch (ewn_rollout.hpp), one unit per board size
struct RollCfg;
struct RollBuf;
int ewn_launch_rollout_s5(const RollCfg &rc, const RollBuf &rb, int T, int opp, int rngk, int agent, bool h2, hipStream_t s);
int ewn_launch_rollout_s6(const RollCfg &rc, const RollBuf &rb, int T, int opp, int rngk, int agent, bool h2, hipStream_t s);
int ewn_launch_rollout_s7(const RollCfg &rc, const RollBuf &rb, int T, int opp, int rngk, int agent, bool h2, hipStream_t s);
int ewn_launch_rollout_s8(const RollCfg &rc, const RollBuf &rb, int T, int opp, int rngk, int agent, bool h2, hipStream_t s);
// ewn_policy.hip: the policy-driven rollout (ewn_step_k_policy); EWN_OK when it serves the configuration
int ewn_policy_supported(const ewn_config *cfg, const Geom &g);
// ewn_policy_eval.hip: the evaluation instances of the policy-driven rollout (ewn_policy_eval); opp 0 minimax max_depth 1-4,
// 1 RandomAgent, 2 minimax max_depth 5 / 6; rngk EWN_RNG_*
struct PolCfg;
struct PolBuf;
int ewn_launch_policy_eval(const PolCfg &pc, const PolBuf &pb, int S, int opp, int rngk, hipStream_t s);
