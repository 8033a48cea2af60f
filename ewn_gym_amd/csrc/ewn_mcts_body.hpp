// ewn_mcts_body.hpp -- K env steps per launch with one thread per game for the rules: rollout_mcts_body (the loop of k_rollout_mcts,
// of ewn_step_k_agent's kernels and of ewn_policy_eval_mcts's), its playout phase, and what it shares with the generic kernels of
// ewn_kernels.hip: the per-lane rules (step_agent / step_opponent / policy_random / lane_auto_reset) and the one copy of the stand-in
// agent, the trajectory row and the write-back (stand_in_action / traj_columns_store / traj_blocks_store / rollout_write_back, also
// k_rollout_generic's).  A header because the body is instantiated in two translation units: ewn_kernels.hip (AG 0 / 1 / 2: the
// stand-in, minimax and MCTS agents) and ewn_policy_eval_mcts.hip (AG 3: the actor-critic, whose matrix code is built with
// -fno-slp-vectorize, a flag ewn_kernels.hip must not get).
#pragma once
#include "ewn_host.hpp"
#include "ewn_playout.hpp"

#include "ewn_lds.hpp"
#include "ewn_step_d3.hpp"
#include "ewn_rollout.hpp"
#include "ewn_mlp3.hpp"

// the auto-reset inside a step: next_seed becomes the episode seed (the freed window is rebuilt by k_mt_refill afterwards)
template <int NW>
EWN_DEV void lane_auto_reset(const Geom &g, const KCfg &c, u32 *rng, int lane, GState<NW> &s, int &dice, LaneRng &r)
{
    r.next_episode(rng, c.N, lane, c.seed_stride, c.key, nullptr);
    init_state<NW>(g, s);
    dice = r.first_dice(g.CN);
}

struct StepRes { double reward; int term, trunc, info; };

// Agent half of step(): envs/ewn.py:438-458 and training_ewn.py:44-66.
// Returns true when the opponent must still reply.
template <int NW>
EWN_DEV bool step_agent(const Geom &g, const KCfg &c, GState<NW> &s, int &dice, int flag, int dir, LaneRng &r,
                           int32_t *tol, StepRes &o)
{
    o.reward = 0.0; o.term = 0; o.trunc = 0; o.info = EWN_INFO_NONE;
    const CubeSel cs = select_cubes(s.aliveP, dice);
    const int k = cube_to_move(cs, flag == 1);
    const bool valid = k >= 0 && dir >= 0 && dir <= 2 && dir_ok<0>(g, pos_of<0>(s, k), dir);
    if (!valid) {
        if (c.shaped) {
            const int t = *tol - 1;
            *tol = t;
            if (t <= 0) { o.reward = -c.reward; o.term = 1; o.trunc = 1; o.info = EWN_INFO_INVALID_PLAYER; }
            else { o.reward = c.illegal_reward; o.info = EWN_INFO_TOLERANCE; }
        } else { o.reward = -c.reward; o.term = 1; o.trunc = 1; o.info = EWN_INFO_INVALID_PLAYER; }
        return false;
    }
    apply_move<0, NW>(g, s, k, dir);
    if (is_win<NW>(g, s)) { o.reward = c.reward; o.term = 1; o.info = EWN_INFO_WON; return false; }
    dice = r.randint(1, g.CN + 1); // the opponent's dice, :458
    return true;
}

// Opponent half: envs/ewn.py:464-486, training_ewn.py:75-99.
template <int NW>
EWN_DEV void step_opponent(const Geom &g, const KCfg &c, GState<NW> &s, int &dice, int oflag, int odir, LaneRng &r,
                              double *prev_score, StepRes &o)
{
    const CubeSel cs = select_cubes(s.aliveN, dice);
    const int k = cube_to_move(cs, oflag == 1);
    const bool valid = k >= 0 && odir >= 0 && odir <= 2 && dir_ok<1>(g, pos_of<1>(s, k), odir);
    if (!valid) { o.reward = 0.0; o.term = 1; o.trunc = 1; o.info = EWN_INFO_INVALID_OPP; return; }
    apply_move<1, NW>(g, s, k, odir);
    if (is_win<NW>(g, s)) { o.reward = -c.reward; o.term = 1; o.info = EWN_INFO_LOST; return; }
    dice = r.randint(1, g.CN + 1); // :483
    if (c.shaped) {
        const double cur = evaluate<NW>(g, s, EWN_H_HYBRID);
        o.reward = cur - *prev_score;
        *prev_score = cur;
    }
}

// RandomAgent.predict on the live env (classical_policies/random_policy.py:11-15):
// uniform index into BOTTOM_RIGHT's legal list, drawn from the lane's own stream.
template <int NW>
EWN_DEV void policy_random(const Geom &g, const GState<NW> &s, int dice, LaneRng &r, int &oflag, int &odir)
{
    const int pick = r.randint(0, legal_count<1, NW>(g, s, dice));   // drawn for an empty list too
    int k;
    oflag = 0; odir = 0;
    legal_nth<1, NW>(g, s, dice, pick, oflag, k, odir);
}

// The stand-in agent of ewn_step_k: RandomAgent.predict (the hash pick of ewn_step_out.random_action) or, with agent_sample,
// env.action_space.sample() (all six actions).  Draws nothing from the lane's stream.
template <int NW>
EWN_DEV void stand_in_action(const Geom &g, const KCfg &c, const GState<NW> &s, int dice, const LaneRng &r, int lane, int agent_sample,
                             int &aflag, int &adir)
{
    const u32 w = agent_hash(r.seed_mix(), r.draws(), (u32)(c.lane_offset + lane), c.key);
    if (agent_sample) { const int a6 = (int)__umulhi(w, 6u); aflag = a6 >= 3 ? 1 : 0; adir = a6 - 3 * aflag; }
    else {
        const int n = legal_count<0, NW>(g, s, dice);
        int k;
        if (n > 0) legal_nth<0, NW>(g, s, dice, (int)__umulhi(w, (u32)n), aflag, k, adir);
    }
}

// A lane's totals over the steps of a launch (ewn_rollout_out.return_sum / n_steps / n_episodes / n_wins)
struct LaneTotals {
    double ret = 0.0;
    int steps = 0, eps = 0, wins = 0;
    EWN_DEV void count(const StepRes &o) { ret += o.reward; steps++; eps += o.term; wins += o.info == EWN_INFO_WON ? 1 : 0; }
};

// One lane's entries of a trajectory row, index = step * N + lane: the columns of ewn_rollout_out that the caller asked for
EWN_DEV void traj_columns_store(const RollBuf &B, size_t index, int aflag, int adir, int dice, const StepRes &o)
{
    if (B.t_action) ((uint16_t *)B.t_action)[index] = pack_action(aflag, adir);
    if (B.t_dice) B.t_dice[index] = (int8_t)dice;
    if (B.t_reward) B.t_reward[index] = o.reward;
    if (B.t_term) B.t_term[index] = (uint8_t)o.term;
    if (B.t_trunc) B.t_trunc[index] = (uint8_t)o.trunc;
    if (B.t_info) B.t_info[index] = (uint8_t)o.info;
}

// A block's part of a trajectory row, row0 = step * N + the block's first lane, nl lanes: the boards, then the records, each staged in
// lds ([.][strd], one slot per thread that owns a game) and copied out in coalesced pieces.  Every thread of the block calls it
// (block barriers); lds holds nothing the caller still needs.
template <int NW>
EWN_DEV void traj_blocks_store(const Geom &g, const RollBuf &B, int8_t *lds, int strd, int tid, bool live, size_t row0, int nl,
                               const GState<NW> &s, int dice, int aflag, int adir, const StepRes &o)
{
    if (B.t_board) {
        if (live) encode_board<NW>(g, s, lds + tid * g.cells);
        __syncthreads();
        block_copy_out(B.t_board + row0 * g.cells, lds, nl * g.cells);
        __syncthreads();
    }
    if (B.t_rec) { // one aligned record per lane-step: board | dice | action | flags | padding (ewn_rollout_out.record)
        if (live) {
            int8_t *rec = lds + tid * strd;
            for (int i = g.cells; i < strd; i++) rec[i] = 0;
            encode_board<NW>(g, s, rec);
            rec[g.cells] = (int8_t)dice; rec[g.cells + 1] = (int8_t)aflag; rec[g.cells + 2] = (int8_t)adir;
            rec[g.cells + 3] = (int8_t)o.term; rec[g.cells + 4] = (int8_t)o.trunc; rec[g.cells + 5] = (int8_t)o.info;
        }
        __syncthreads();
        block_copy_out((int8_t *)B.t_rec + row0 * strd, lds, nl * strd);
        __syncthreads();
    }
}

// After the last step: the board through lds, the RNG header and the dice unless the lane was frozen when the launch began (its state
// is not the launch's to touch), the done flag, the totals added to the caller's.  Every thread of the block calls it (block barrier).
template <int NW>
EWN_DEV void rollout_write_back(const Geom &g, const KState &st, const RollBuf &B, int8_t *lds, int tid, bool live, int lane, int lane0,
                                int nl, const GState<NW> &s, int dice, const LaneRng &r, bool frozen0, bool frozen, const LaneTotals &tot)
{
    if (live) {
        encode_board<NW>(g, s, lds + tid * g.cells);
        if (!frozen0) { *rng_hdr_ptr(st.rng, lane) = r.header(); st.dice[lane] = (int8_t)dice; }
        st.done[lane] = frozen ? 1 : 0;
        if (B.ret_sum) B.ret_sum[lane] += tot.ret;
        if (B.n_steps) B.n_steps[lane] += tot.steps;
        if (B.n_episodes) B.n_episodes[lane] += tot.eps;
        if (B.n_wins) B.n_wins[lane] += tot.wins;
    }
    __syncthreads();
    block_copy_out(st.board + (size_t)lane0 * g.cells, lds, nl * g.cells);
}

// the canonical observation of a game as the playouts' byte-per-cube start position
EWN_DEV PState pstate_from_gstate(const Geom &g, const GState<1> &c)
{
    u32 w[4] = { 0x40404040u, 0x40404040u, 0x40404040u, 0x40404040u };   // every cube off the board (pstate_load's encoding)
    #pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32 cp = (u32)pos_get<1>(c.posP, k), rp = (cp * g.div_magic) >> 16, cn = (u32)pos_get<1>(c.posN, k), rn = (cn * g.div_magic) >> 16;
        if ((c.aliveP >> k) & 1u) w[k & 1] ^= (0x40u ^ (rp * 8u + (cp - rp * (u32)g.S))) << (8 * (k >> 1));
        if ((c.aliveN >> k) & 1u) w[2 + (k & 1)] ^= (0x40u ^ (rn * 8u + (cn - rn * (u32)g.S))) << (8 * (k >> 1));
    }
    const PState st = { w[0], w[1], w[2], w[3] };
    return st;
}

struct MctsRoll { int K, total, gl, agent_sample, strd, gpb; };   // strd: bytes per game of the dynamic LDS area (a record, or S*S)

// mr.gpb games per block of BS threads: the rules run one thread per game (the block's first lanes), the playouts on all BS lanes
// (the measurements behind the block size: k_rollout_mcts, ewn_kernels.hip).
#define MR_GPB 128        // the most games a block takes (LDS arrays); the launchers pick mr.gpb <= MR_GPB (8 or 4, doubled with N)

// the agent of k_rollout_mcts_agent (ewn_step_k_agent): minimax max_depth / heuristic, or MCTS with `total` playouts per root move in
// groups of 2^gl lanes on the playout stream of evaluation step t = step_base + kstep: obs_word(lane_offset + lane, 'MCTS', key_t),
// key_t = key + 0x9E3779B97F4A7C15 * (t + 1) -- what tournament.evaluate's per-step loop passes to predict_mcts
struct AgentRoll { int depth, heur, total, gl; u32 step_base; u64 key; };

// One flat Monte-Carlo decision (mcts.py:47-69) for every game of the block whose owner thread passes n_root > 0, its start position,
// dice and playout stream already in pb0 / pdice / pword[tid]: `total` playouts per (game, root move) cell, BOTTOM_RIGHT replying
// first, a group of 2^gl lanes per cell; a group that has finished its cell takes the next unplayed one (results do not depend on who
// plays what).  Leaves the wins per root move in wins[tid] (-1: no such move).  Every thread of the block calls it (block barriers).
EWN_DEV void mcts_playout_phase(const Geom &g, const PlayTab *T, const PState *pb0, const u32 *pword, const int8_t *pdice, int (*wins)[6],
                                uint16_t *livec, int *nlive_s, int *next_slot, int *nextc, int *myslot, int tid, bool owner, int n_root,
                                int total, int gl, int tc, int glane, int grp)
{
    if (owner) {
        #pragma unroll
        for (int i = 0; i < 6; i++) wins[tid][i] = i < n_root ? 0 : -1;
    }
    if (tid == 0) { *nlive_s = 0; *next_slot = BS >> gl; }
    __syncthreads();
    if (n_root > 0) { const int base = atomicAdd(nlive_s, n_root); for (int i = 0; i < n_root; i++) livec[base + i] = (uint16_t)(tid * 8 + i); }
    __syncthreads();
    const int nlive = *nlive_s;
    int slot = grp;
    while (slot < nlive) {
        const int cell = livec[slot], gi = cell >> 3, i = cell & 7;
        if (glane == 0) nextc[grp] = tc;   // same wave as the lanes that read it: LDS operations of a wave execute in order
        PState b0 = pb0[gi];
        int w;
        if (playout_root_move(T, b0, g.S, pdice[gi], i)) w = glane < total ? (total - glane + tc - 1) >> gl : 0;   // TOP_LEFT has won
        else w = run_playouts<1>(T, b0, g.S, pword[gi], (u32)(i * total), glane, total, &nextc[grp]);         // BOTTOM_RIGHT replies first
        for (int off = tc >> 1; off > 0; off >>= 1) w += __shfl_down(w, off, tc);
        if (glane == 0) { wins[gi][i] = w; myslot[grp] = atomicAdd(next_slot, 1); }
        __builtin_amdgcn_wave_barrier();
        slot = myslot[grp];
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
}

// np.argmax over the six win counters of an observation's root moves (first maximum, mcts.py:68); -1 for a row of six -1: no root
// move (a finished observation, an inactive lane), where the stateless policy answers (0, 0)
EWN_DEV int argmax_wins(const int *w6)
{
    int best = -1, bw = -1;
    #pragma unroll
    for (int i = 0; i < 6; i++) { const int w = w6[i]; if (w > bw) { bw = w; best = i; } }
    return best;
}

// MctsAgent's choice inside the K-step loop: that entry of the legal list of the observation.  Its owner has a root move, so it starts
// the maximum at entry 0; kept as its own loop because rebasing it on argmax_wins changes the code of the kernels around it.
EWN_DEV void mcts_pick(const Geom &g, const GState<1> &obs, int dice, const int *w6, int &flag, int &dir)
{
    int best = 0, bw = -1;
    #pragma unroll
    for (int i = 0; i < 6; i++) { const int w = w6[i]; if (w > bw) { bw = w; best = i; } }
    int k;
    flag = 0; dir = 0;
    legal_nth<0, 1>(g, obs, dice, best, flag, k, dir);
}

// The dynamic LDS of the AG 3 instances behind the boards area: the policy net's forward image (mlp3_pack_fwd), then per game of the
// block's 32-game network tiles eight floats of logits, a zero-padded observation slot (the board bytes, feature k at byte k: what
// k_rollout_mlp's slots hold) and the dice.
template <int S> struct MctsNet {
    static constexpr int OSTR = 16 * Mlp3Geo<S>::KB1;      // bytes per observation slot: the k-blocks of layer 1
    static_assert(OSTR >= S * S, "a slot holds the board");
    static constexpr int tiles(int gpb) { return (gpb + 31) / 32; }
    static constexpr size_t o_img(int gpb, int strd) { return ((size_t)gpb * strd + 15) & ~(size_t)15; }
    static constexpr size_t o_logits(int gpb, int strd) { return o_img(gpb, strd) + Mlp3Geo<S>::FWD_BYTES; }
    static constexpr size_t o_slots(int gpb, int strd) { return o_logits(gpb, strd) + (size_t)tiles(gpb) * 32 * 8 * 4; }
    static constexpr size_t o_dice(int gpb, int strd) { return o_slots(gpb, strd) + (size_t)tiles(gpb) * 32 * OSTR; }
    static constexpr size_t lds_bytes(int gpb, int strd) { return o_dice(gpb, strd) + (size_t)tiles(gpb) * 32; }
    static_assert(Mlp3Geo<S>::FWD_BYTES % 16 == 0, "image alignment");
};

// K env steps of mr.gpb games per block.  AG: 0 ewn_step_k's stand-in agent (mr.agent_sample; ar is not read), 1 minimax (ar.depth,
// ar.heur), 2 MCTS (a playout phase over the agent's observation before the agent half), 3 the actor-critic's argmax (below).  OPP: 0 RandomAgent,
// 1 minimax (c.depth, c.heur), 2 MCTS (its playout phase between the two halves).  The minimax searches (AG 1's agent, OPP 1's opponent: one of them per instance) are the table-driven fast_d3 of
// k_predict_minimax_fast / ewn_step's table path, on the rules thread, from an image of the search's table in LDS (S = board size;
// 0 = no search, no table).  k_rollout_mcts (ewn_kernels.hip: ewn_step_k against the MCTS opponent) is the instance <0, 2, 0>;
// DESIGN.md 4e has the measurement that let its own copy of this loop go.
//
// AG 3 (ewn_policy_eval_mcts): OPP 2 only, un-shaped, no auto-reset.  B.agent_tables = the actor-critic's flat fp32
// parameters; S = the board size of Mlp3Geo<S>, no table image.  The action row of a lane is written only for the steps it plays,
// and a block whose games are all over leaves the step loop.
template <int AG, int OPP, int S>
EWN_DEV void rollout_mcts_body(const Geom &g, const KCfg &c, const KState &st, const MctsRoll &mr, const RollBuf &B, const AgentRoll &ar)
{
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];   // [MR_GPB][strd]: packed boards in and out, trajectory rows in between
    __shared__ PlayTab T;
    __shared__ PState pb0[MR_GPB];
    __shared__ u32 pword[MR_GPB];
    __shared__ int8_t pdice[MR_GPB];
    __shared__ int wins[MR_GPB][6];
    __shared__ uint16_t livec[MR_GPB * 6];
    __shared__ int nlive_s, next_slot;
    __shared__ int nextc[BS / 8], myslot[BS / 8];
    constexpr int TS = S ? S : 5;
    [[maybe_unused]] const FastTab<TS> *ft = nullptr;
    if constexpr (S != 0 && AG != 3) {   // LDS-DMA behind the boards area, waited for at the first barrier
        int8_t *tb = lds + ((mr.gpb * mr.strd + 15) & ~15);
        tables_to_lds<FAST_TAB_BYTES(TS)>(tb, (const int8_t *)B.tables);
        ft = (const FastTab<TS> *)tb;
    }
    playtab_build(&T, g.S);
    const int tid = (int)threadIdx.x, lane0 = (int)blockIdx.x * mr.gpb, nl = min(mr.gpb, c.N - lane0), lane = lane0 + tid;
    const bool owner = tid < mr.gpb, live = owner && lane < c.N;
    using NG = MctsNet<TS>;
    [[maybe_unused]] int8_t *Wpi = nullptr, *oslot = nullptr, *odice = nullptr;
    [[maybe_unused]] float *LG = nullptr;
    if constexpr (AG == 3) {   // the policy net's image, packed once per launch; every slot zero (the padding stays zero), every dice 1
        static_assert(S == 5 || S == 7, "the actor-critic's geometries");
        static_assert(OPP == 2, "the other opponents are ewn_policy_eval's");
        Wpi = lds + NG::o_img(mr.gpb, mr.strd);
        LG = (float *)(lds + NG::o_logits(mr.gpb, mr.strd));
        oslot = lds + NG::o_slots(mr.gpb, mr.strd);
        odice = lds + NG::o_dice(mr.gpb, mr.strd);
        mlp3_pack_fwd<TS>(Wpi, (const float *)B.agent_tables, 0, tid, BS);
        const int ngt = NG::tiles(mr.gpb) * 32;
        for (int i = tid; i < ngt * (NG::OSTR / 4); i += BS) ((u32 *)oslot)[i] = 0u;
        for (int i = tid; i < ngt; i += BS) odice[i] = 1;
    }
    uint4 hdr = make_uint4(0u, 0u, 0u, 0u);
    int dice = 1;
    bool frozen = true;
    if (live) { hdr = *rng_hdr_ptr(st.rng, lane); dice = st.dice[lane]; frozen = st.done[lane] != 0; }
    const bool frozen0 = frozen;
    block_copy_in(lds, st.board + (size_t)lane0 * g.cells, nl * g.cells);
    if constexpr (S != 0 && AG != 3) lds_dma_wait();
    __syncthreads();
    GState<1> s;
    decode_board<1>(g, lds + (live ? tid : 0) * g.cells, s);
    LaneRng r; r.load(c.rng_kind, hdr, rng_win_ptr(st.rng, c.N, c.W, live ? lane : 0, RNGF_CUR(hdr.w)), c.W, c.key);
    r.begin_kernel();
    LaneTotals tot;
    const int tc = 1 << mr.gl, glane = tid & (tc - 1), grp = tid >> mr.gl;
    const int atc = 1 << ar.gl, aglane = tid & (atc - 1), agrp = tid >> ar.gl;   // the agent's playout groups (AG 2)

    for (int kstep = 0; kstep < mr.K; kstep++) {
        const bool active = live && !frozen;
        StepRes o; o.reward = 0.0; o.term = (live && frozen) ? 1 : 0; o.trunc = 0; o.info = EWN_INFO_NONE;
        int aflag = 0, adir = 0, n_root = 0;
        bool reply = false;
        GState<1> cst = s;
        if constexpr (AG == 0) {
            if (active) stand_in_action<1>(g, c, s, dice, r, lane, mr.agent_sample, aflag, adir);
        }
        if constexpr (AG == 2) {
            // MctsAgent.predict(env.board, env.dice): the agent's observation as it stands, its root moves, its playout stream
            int a_root = 0;
            if (active) {
                pb0[tid] = pstate_from_gstate(g, s);
                pdice[tid] = (int8_t)dice;
                const u64 key_t = ar.key + 0x9E3779B97F4A7C15ull * ((u64)ar.step_base + (u64)kstep + 1ull);
                pword[tid] = PlayoutRng::obs_word((u32)(c.lane_offset + lane), 0x4D435453u, key_t);
                a_root = legal_count<0, 1>(g, s, dice);
            }
            mcts_playout_phase(g, &T, pb0, pword, pdice, wins, livec, &nlive_s, &next_slot, nextc, myslot, tid, owner, a_root, ar.total,
                               ar.gl, atc, aglane, agrp);
            if (active) mcts_pick(g, s, dice, wins[tid], aflag, adir);
        }
        if constexpr (AG == 3) {
            // model.predict(deterministic=True) on (env.board, env.dice): the owners publish their observations, the block's first
            // ceil(gpb / 32) waves each run one 32-game tile of the policy net on the matrix pipe (whole waves enter or skip: the MFMA
            // operands come from every lane), the owners take the argmax.  The features are built as k_rollout_mlp builds them.
            if (active) { encode_board<1>(g, s, oslot + tid * NG::OSTR); odice[tid] = (int8_t)dice; }
            if (!__syncthreads_or(active ? 1 : 0)) break;   // block-uniform: every game of the block is over, nothing is left to write
            const int wave = tid >> 6, wl = tid & 63;
            if (wave < NG::tiles(mr.gpb)) {
                const int j = wl & 31, h = wl >> 5, dj = odice[wave * 32 + j];
                const int8_t *sj = oslot + (wave * 32 + j) * NG::OSTR + 8 * h;
                auto xb = [&](int kb) { return pol_obs_operand<TS>(sj, kb, h, dj); };
                f32x16 h1[2], h2[2];
                float lo[MLP_NA];
                mlp3_forward<TS, MLP_NA>(Wpi, wl, xb, h1, h2, lo);
                if (wl < 32) { float *q = LG + (wave * 32 + wl) * 8; *(float4 *)q = make_float4(lo[0], lo[1], lo[2], lo[3]); q[4] = lo[4]; }
            }
            __syncthreads();
            if (active) {   // k_rollout_mlp's deterministic pick: strict comparisons, so ties break the same way
                const float4 lg = *(const float4 *)(LG + tid * 8);
                const float lg4 = LG[tid * 8 + 4];
                aflag = pol_pick_flag(lg.x, lg.y);
                adir = pol_pick_dir(lg.z, lg.w, lg4);
            }
        }
        if (active) {
            if constexpr (AG == 1) {   // ExpectiMinimaxAgent.predict on the agent's observation (TOP_LEFT to move): k_predict_minimax_fast
                aflag = -1; adir = -1;
                if (ar.heur == EWN_H_TWO_MIN_DIST) fast_d3<TS, true>(ft, s, dice, ar.depth, aflag, adir);
                else fast_d3<TS, false>(ft, s, dice, ar.depth, aflag, adir);
            }
            r.prefetch();
            r.begin_step();
            reply = step_agent<1>(g, c, s, dice, aflag, adir, r, nullptr, o);      // envs/ewn.py:438-458
            if constexpr (OPP == 2) {
                if (reply) { // MctsAgent.predict's input: the canonical observation (envs/ewn.py:289-296), its root moves, its playout stream
                    cst = canonicalize<1>(g, s);
                    pb0[tid] = pstate_from_gstate(g, cst);
                    pdice[tid] = (int8_t)dice;
                    pword[tid] = PlayoutRng::obs_word(r.seed_mix() * 0x9E3779B1u + r.draws(), 0x4D435453u, c.key);
                    n_root = legal_count<0, 1>(g, cst, dice);
                }
            } else if (reply) {
                int oflag = 0, odir = 0;
                if constexpr (OPP == 0) policy_random<1>(g, s, dice, r, oflag, odir);
                else {   // the minimax opponent on its canonical observation, as ewn_step's table path searches it
                    cst = canonicalize<1>(g, s);
                    if (c.heur == EWN_H_TWO_MIN_DIST) fast_d3<TS, true>(ft, cst, dice, c.depth, oflag, odir);
                    else fast_d3<TS, false>(ft, cst, dice, c.depth, oflag, odir);
                }
                step_opponent<1>(g, c, s, dice, oflag, odir, r, nullptr, o);              // envs/ewn.py:464-486
            }
        }
        if constexpr (OPP == 2) {
            // ---- the playouts of the block's (game, root move) cells, then the opponent's half (envs/ewn.py:464-486)
            mcts_playout_phase(g, &T, pb0, pword, pdice, wins, livec, &nlive_s, &next_slot, nextc, myslot, tid, owner, n_root, mr.total,
                               mr.gl, tc, glane, grp);
            if (reply) {
                int oflag = 0, odir = 0;
                mcts_pick(g, cst, dice, wins[tid], oflag, odir);
                step_opponent<1>(g, c, s, dice, oflag, odir, r, nullptr, o);
            }
        }
        if (active) {
            tot.count(o);
            if (o.term) { if (c.autoreset) lane_auto_reset<1>(g, c, st.rng, lane, s, dice, r); else frozen = true; }
        }
        // ---- this step's trajectory row (AG 3, as ewn_policy_eval: the action of a lane that played this step, nothing else)
        if constexpr (AG == 3) {
            if (active && B.t_action)
                ((uint16_t *)B.t_action)[(size_t)kstep * c.N + lane] = (uint16_t)((uint8_t)aflag | ((uint16_t)(uint8_t)adir << 8));
        } else if (live) traj_columns_store(B, (size_t)kstep * c.N + lane, aflag, adir, dice, o);
        traj_blocks_store<1>(g, B, lds, mr.strd, tid, live, (size_t)kstep * c.N + lane0, nl, s, dice, aflag, adir, o);
    }
    rollout_write_back<1>(g, st, B, lds, tid, live, lane, lane0, nl, s, dice, r, frozen0, frozen, tot);
}
