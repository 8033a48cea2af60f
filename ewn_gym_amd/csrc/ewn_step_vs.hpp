// ewn_step_vs.hpp -- the env step against a TRAINED policy for any agent (C ABI: ewn_step_vs, ewn_step_k_vs): the reference's
// `opponent_policy=<path>` env (envs/ewn.py:265-296, 464-486) as eval_random.py / eval_minimax.py / play_gym.py and the SB3 adapter meet
// it.  ewn_policy_body.inc plays this opponent only where the agent is a network too; here the agent's action comes from the caller
// (one step per launch: ewn_step's contract) or from one of the classical agents (K steps per launch: ewn_step_k's contract).
//
// One kernel text.  Two lanes per game and 32 games per wave, as in ewn_policy_body.inc, because the opponent's network is evaluated
// for a whole wave of games at once: the wave's 32 games are the 32 columns of the MFMA tiles (ewn_mlp3.hpp).
//   per launch   table image -> LDS (LDS-DMA); ONE forward image of the opponent's parameters (mlp3_pack_fwd, net 0);
//                boards -> registers (d3_decode) and per-game LDS slots (rec_slot_build)
//   per env step the agent's action; agent half (plain or shaped: tolerance, prev_score); the opponent's dice; the opponent's network
//                on np.rot90(-board, 2) read straight out of the slots (pol_opp_operand, ewn_mlp3.hpp); argmax or Gumbel-max;
//                opponent half (an impossible move ends the game: EWN_INFO_INVALID_OPP, reward 0); shaped reward; auto-reset or freeze;
//                this step's outputs
//   after the last step the state goes back once
// Stream contract: per step the lane's dice stream gives the opponent's dice and then the next dice, nothing else (the network draws
// nothing); the opponent's sampling noise is the word k_rollout_mlp_vs uses, taken before the step moves the stream, so a step here is a
// step there, bit for bit (tests/test_gpu_step_vs.py).  The stand-in agents use ewn_step_k's hash stream.
#pragma once
#include "ewn_policy.hpp"

struct VsCfg {
    int N, autoreset, lane_offset, agent_depth, K;
    int agent_sample;                      // AG 1: 1 = env.action_space.sample() instead of RandomAgent
    int shaped, refresh, opp_deterministic;
    u32 seed_stride, W;
    double reward, illegal_reward;
    u64 key, opp_noise_key;
};

struct VsBuf {
    int8_t *board; int8_t *dice; uint8_t *done; u32 *rng; double *prev_score; int32_t *tolerance;
    const void *tables;                    // AG 3 / 4: the image of the agent's search; else any image (geometry and selectors only)
    const float *opp_params;
    const int8_t *actions;                 // AG 0: [N][2]
    int8_t *tboard; int8_t *tdice;         // AG 0: the observation before the auto-reset (ewn_step_out.terminal_*), each may be NULL
    // this step's row, [K][N]...: the columns of ewn_rollout_out (AG 0, K = 1: reward / terminated / truncated / info of ewn_step_out)
    int8_t *t_board; int8_t *t_dice; int8_t *t_action; double *t_reward; uint8_t *t_term; uint8_t *t_trunc; uint8_t *t_info; uint8_t *t_rec;
    double *ret_sum; int32_t *n_steps; int32_t *n_episodes; int32_t *n_wins;
    int8_t *o_action;                      // [K][N][3] {dice, flag, dir} of the opponent's move, {0, 0, 0} when it did not move; may be NULL
};

// AG: where the agent's action comes from.  0: the caller's int8 [N][2], one step (ewn_step's contract: a direction outside {0, 1, 2} is
// an illegal move); 1: RandomAgent / action_space.sample() (roll_stand_in_action: ewn_step_k's hash stream); 3: ExpectiMinimaxAgent
// 'hybrid' of max_depth 1-4 (d3_search on the rs_flip-ed position, as k_rollout_d3 runs it); 4: of max_depth 5 / 6 (d5_dispatch).
// RNGK: the dice, 1 Philox, 0 MT19937-compat (no auto-reset: host check).
template <int S, int NT, int AG, int RNGK>
__global__ __launch_bounds__(NT, 2) void k_step_vs(VsCfg c, VsBuf B)
{
    static_assert(AG == 0 || AG == 1 || AG == 3 || AG == 4, "caller, stand-in, minimax 1-4, minimax 5 / 6");
    constexpr int T = 2, GPB = NT / T, CELLS = S * S, STR = RecGeo<S>::STR;
    using Q3 = Mlp3Geo<S>;
    static_assert(Q3::FWD_BYTES % 16 == 0, "image alignment");
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *tb = lds;
    int8_t *Wop = lds + FAST_TAB_BYTES(S);
    float *lx_all = (float *)(Wop + Q3::FWD_BYTES);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *LX = lx_all + wave * 32 * 8;                    // this wave's 8 floats per game of head outputs
    int8_t *slots = (int8_t *)(lx_all + GPB * 8);
    uint8_t *garr = (uint8_t *)(slots + GPB * STR);
    tables_to_lds_nt<FAST_TAB_BYTES(S), NT>(tb, (const int8_t *)B.tables);
    const FastTab<S> *Tb = (const FastTab<S> *)tb;
    mlp3_pack_fwd<S>(Wop, B.opp_params, 0, threadIdx.x, NT);

    const int g0 = (int)blockIdx.x * GPB, ng = min(GPB, c.N - g0);
    const int gl = threadIdx.x / T, sub = threadIdx.x % T, game = g0 + gl;
    const int jw = lane >> 1;                              // my game's column inside the wave's tile
    const bool live = game < c.N, writer = live && sub == 0;
    const int K = AG == 0 ? 1 : c.K;

    uint4 hdr = make_uint4(0u, 0u, 0u, 0u);
    int dice = 1, tol = 0, aflag = 0, adir = 0;
    double prev = 0.0;
    bool frozen = true;
    if (live) {
        hdr = *rng_hdr_ptr(B.rng, game);
        dice = B.dice[game];
        frozen = B.done[game] != 0;
        if (c.shaped) { tol = B.tolerance[game]; prev = B.prev_score[game]; }
        if constexpr (AG == 0) {
            const uint16_t a2 = ((const uint16_t *)B.actions)[game];
            aflag = (int8_t)(a2 & 0xff); adir = (int8_t)(a2 >> 8);
        }
    }
    const bool frozen0 = frozen;
    block_copy_in(slots, B.board + (size_t)g0 * CELLS, ng * CELLS);      // packed boards, decoded from there
    LaneRng r; r.load(RNGK, hdr, RNGK == 0 ? rng_win_ptr(B.rng, c.N, c.W, live ? game : 0, RNGF_CUR(hdr.w)) : nullptr, c.W, c.key);
    r.begin_kernel();
    lds_dma_wait();
    __syncthreads();
    RState<S> s;
    d3_decode<S, T>(live ? slots + gl * CELLS : slots, sub, garr + gl * 16, s);
    __syncthreads();                                       // every game is in registers: the board area becomes the per-game slots
    int8_t *slot = slots + gl * STR;
    rec_slot_build<S, T>(Tb, s, sub, slot);
    double ret_acc = 0.0;
    int n_steps = 0, n_eps = 0, n_wins = 0;
    [[maybe_unused]] RollCfg rc;                           // what roll_stand_in_action reads
    rc.agent_sample = c.agent_sample; rc.lane_offset = c.lane_offset; rc.key = c.key;

    #pragma unroll 1
    for (int kstep = 0; kstep < K; kstep++) {
        const bool active = live && !frozen;
        double reward = 0.0;
        int term = 0, trunc = 0, info = EWN_INFO_NONE;
        if (live && frozen) term = 1;                      // a finished, un-reset game stays put (as in ewn_step)
        // ---- the agent's action for the current observation (the agent is the canonical BOTTOM_RIGHT side)
        if constexpr (AG == 1) {
            aflag = 0; adir = 0;
            roll_stand_in_action<S>(Tb, s, pk_sel<S>(Tb, s.posN, dice), r, rc, game, aflag, adir);
        }
        if constexpr (AG == 3 || AG == 4) {
            // ExpectiMinimaxAgent.predict(canonical observation): the agent's own position IS canonical for it once flipped
            aflag = 0; adir = 0;
            const RState<S> f = rs_flip<S>(Tb, s);
            if constexpr (AG == 3) d3_search<S, T>(Tb, f, dice, sub, c.agent_depth, aflag, adir);
            else d5_dispatch<S, T>(Tb, f, dice, sub, aflag, adir);
        }
        // the opponent's noise: k_rollout_mlp_vs's word (ewn_policy_body.inc), taken here, before the step moves the stream
        const u32 w0o = pol_opp_noise_word(r.seed_mix(), tol, r.draws(), c.lane_offset + game, c.key, c.opp_noise_key);
        // ---- agent half, envs/ewn.py:438-458 / envs/training_ewn.py:44-66
        bool reply = false;
        if (active) {
            if constexpr (RNGK == 0) r.prefetch();
            r.begin_step();
            if constexpr (RNGK == 1) r.ps.prime();
            const int k = pk_cube(pk_sel<S>(Tb, s.posN, dice), aflag == 1);
            const int pb = pk_get(s.posN, k);
            const int q = (adir >= 0 && adir <= 2) ? Tb->nbn[adir][pb] : 255;   // no cube at all: byte 6 -> 255
            if (q == 255) {
                if (c.shaped) { // an illegal move costs tolerance; the game goes on until it is used up (training_ewn.py:48-56)
                    tol -= 1;
                    if (tol <= 0) { reward = -c.reward; term = 1; trunc = 1; info = EWN_INFO_INVALID_PLAYER; }
                    else { reward = c.illegal_reward; info = EWN_INFO_TOLERANCE; }
                } else { reward = -c.reward; term = 1; trunc = 1; info = EWN_INFO_INVALID_PLAYER; }
            } else {
                const int cp = Tb->real_of_ring[pb & 63], cq = Tb->real_of_ring[q];
                slot[cp] = 0; slot[cq] = (int8_t)(k + 1);
                rs_move<S, false>(s, k, q);
                if (q == Tb->ri_origin || s.P == 0) { reward = c.reward; term = 1; info = EWN_INFO_WON; }
                else { dice = r.randint(1, 7); reply = true; }
            }
        }
        const int odice = dice;                            // the opponent's dice where it replies
        // ---- the opponent's network on its canonical view (pol_opp_operand, ewn_mlp3.hpp), run by every lane of the wave (its 32 games
        // are the tile's 32 columns)
        __builtin_amdgcn_wave_barrier();                   // the agent's moves are in the slots
        {
            const int j = lane & 31, h = lane >> 5;
            const int dj = __builtin_amdgcn_ds_bpermute((2 * j) << 2, dice);          // game j's dice (its lanes are 2 j, 2 j + 1)
            const int8_t *sj = slots + (wave * 32 + j) * STR;
            auto xo = [&](int kb) { return pol_opp_operand<S>(sj, kb, h, dj); };
            f32x16 h1[2], h2[2];
            float lo[MLP_NA];
            mlp3_forward<S, MLP_NA>(Wop, lane, xo, h1, h2, lo);
            if (lane < 32) { *(float4 *)(LX + lane * 8) = make_float4(lo[0], lo[1], lo[2], lo[3]); LX[lane * 8 + 4] = lo[4]; }
        }
        __builtin_amdgcn_wave_barrier();
        const float4 og = *(const float4 *)(LX + jw * 8);
        const float og4 = LX[jw * 8 + 4];
        __builtin_amdgcn_wave_barrier();
        float on[5];
        #pragma unroll
        for (int i = 0; i < 5; i++) on[i] = c.opp_deterministic ? 0.0f : pol_gumbel(pol_uniform(w0o, i));
        const float y0 = og.x + on[0], y1 = og.y + on[1], y2 = og.z + on[2], y3 = og.w + on[3], y4 = og4 + on[4];
        const int oflag = pol_pick_flag(y0, y1);
        const int odir = pol_pick_dir(y2, y3, y4);
        // ---- opponent half, envs/ewn.py:464-486
        if (reply) {
            const int k = pk_cube(pk_sel<S>(Tb, s.posP, dice), oflag == 1);
            const int pb = pk_get(s.posP, k);
            const int q = Tb->nbp[odir][pb];
            // a network may pick a move that leaves the board or a cube that is gone: envs/ewn.py:469-473
            if (q == 255) { reward = 0.0; term = 1; trunc = 1; info = EWN_INFO_INVALID_OPP; }
            else roll_opponent_move<S>(Tb, s, k, pb, q, dice, r, c.reward, reward, term, info, slot);
            if (c.shaped && !term) { // reward = evaluate() - prev_score (training_ewn.py:94-96)
                const double cur = d3_shaped_score<S>(Tb, s);
                reward = cur - prev;
                prev = cur;
            }
        }
        if constexpr (AG == 0) {                           // the observation before the auto-reset (a frozen lane: the one it holds)
            if (writer && B.tdice) B.tdice[game] = (int8_t)dice;
            if (writer && B.tboard) { int8_t *dst = B.tboard + (size_t)game * CELLS; for (int i = 0; i < CELLS; i++) dst[i] = slot[i]; }
        }
        if (active) {
            ret_acc += reward; n_steps++; n_eps += term; n_wins += info == EWN_INFO_WON ? 1 : 0;
            if (term) {
                if (c.autoreset) {                         // Philox kind only (host check)
                    r.next_episode(B.rng, c.N, game, c.seed_stride, c.key, nullptr);
                    d3_init_state<S>(Tb, s);
                    rec_slot_init<S>(slot);
                    dice = r.first_dice(6);
                    if (c.shaped && c.refresh) prev = d3_shaped_score<S>(Tb, s);
                } else frozen = true;
            }
        }
        // ---- this step's outputs
        __builtin_amdgcn_wave_barrier();
        if (live) {
            const size_t o = (size_t)kstep * c.N + game;
            if (sub == 0) {
                if (B.o_action) {
                    int8_t *p = B.o_action + o * 3;
                    p[0] = (int8_t)(reply ? odice : 0); p[1] = (int8_t)(reply ? oflag : 0); p[2] = (int8_t)(reply ? odir : 0);
                }
                if constexpr (AG == 0) {                   // ewn_step_out: the four columns are required (host check), nothing else exists
                    B.t_reward[o] = reward; B.t_term[o] = (uint8_t)term; B.t_trunc[o] = (uint8_t)trunc; B.t_info[o] = (uint8_t)info;
                } else {
                    if (B.t_action) ((uint16_t *)B.t_action)[o] = (uint16_t)((uint8_t)aflag | ((uint16_t)(uint8_t)adir << 8));
                    if (B.t_dice) B.t_dice[o] = (int8_t)dice;
                    if (B.t_reward) B.t_reward[o] = reward;
                    if (B.t_term) B.t_term[o] = (uint8_t)term;
                    if (B.t_trunc) B.t_trunc[o] = (uint8_t)trunc;
                    if (B.t_info) B.t_info[o] = (uint8_t)info;
                }
            }
            if constexpr (AG != 0) {
                if (B.t_rec) rec_store<S, T>(slot, sub, dice, aflag, adir, term, trunc, info, B.t_rec + o * STR);
                if (B.t_board && sub == 0) { int8_t *dst = B.t_board + o * CELLS; for (int i = 0; i < CELLS; i++) dst[i] = slot[i]; }
            }
        }
    }
    // ---- the state goes back to HBM once, through the packed board area
    __syncthreads();
    if (live) d3_encode<S, T>(Tb, s, sub, slots + gl * CELLS);
    if (writer) {
        if (!frozen0) { *rng_hdr_ptr(B.rng, game) = r.header(); B.dice[game] = (int8_t)dice; }
        B.done[game] = frozen ? 1 : 0;
        if (c.shaped) { B.tolerance[game] = tol; B.prev_score[game] = prev; }
        if constexpr (AG != 0) {
            if (B.ret_sum) B.ret_sum[game] += ret_acc;
            if (B.n_steps) B.n_steps[game] += n_steps;
            if (B.n_episodes) B.n_episodes[game] += n_eps;
            if (B.n_wins) B.n_wins[game] += n_wins;
        }
    }
    __syncthreads();
    block_copy_out(B.board + (size_t)g0 * CELLS, slots, ng * CELLS);
}
