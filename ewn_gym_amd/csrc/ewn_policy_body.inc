// ewn_policy_body.inc -- the text of k_rollout_mlp / k_rollout_mlp_vs (ewn_policy.hpp), included into both kernels: in scope are the
// template parameters S, OPP, NT, TRJ, RNGK and the arguments PolCfg c, PolBuf B, PolOpp O.  One text, so that the policy opponent is
// the same env step as every other opponent; included, not called, so that k_rollout_mlp stays the kernel it was, instruction for
// instruction (a wrapper around an inlined body compiles to a different register allocation).  With k_step_vs and k_predict_mlp it
// shares small value-returning helpers only (pol_obs_operand, pol_opp_operand, pol_pick_*, pol_gumbel, pol_opp_noise_word): those compile
// to the instructions of the text written out (diff the units' device assembly against the parent's after touching one); the whole
// opponent-network block as a helper, or a pick through reference parameters, do not.
    constexpr bool FIX = TRJ == 1, EV = TRJ == 2;
    static_assert(EV || (OPP != 2 && RNGK == 1), "the depth-5 opponent and the MT19937-compat dice are evaluation-only");
    const bool want_value = !FIX && !EV && c.want_value, deterministic = EV || (!FIX && c.deterministic), rec0 = FIX || (!EV && c.rec0);
    constexpr int T = 2, GPB = NT / T, CELLS = S * S, STR = RecGeo<S>::STR, NCH = RecGeo<S>::NCH;
    using G = MlpGeo<S>;
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    using Q3 = Mlp3Geo<S>;
    static_assert(Q3::FWD_BYTES % 16 == 0, "image alignment");
    int8_t *tb = lds;
    int8_t *Wpi = lds + FAST_TAB_BYTES(S);
    int8_t *Wvf = Wpi + Q3::FWD_BYTES;
    int8_t *Wop = Wpi + (want_value ? 2 : 1) * Q3::FWD_BYTES;   // OPP 3 only
    float *lx_all = (float *)(Wpi + ((want_value ? 2 : 1) + (OPP == 3 ? 1 : 0)) * Q3::FWD_BYTES);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *LX = lx_all + wave * 32 * 8;                    // this wave's 8 floats per game of head outputs
    int8_t *slots = (int8_t *)(lx_all + GPB * 8);
    uint8_t *garr = (uint8_t *)(slots + GPB * STR);
    tables_to_lds_nt<FAST_TAB_BYTES(S), NT>(tb, (const int8_t *)B.tables);
    const FastTab<S> *Tb = (const FastTab<S> *)tb;
    mlp3_pack_fwd<S>(Wpi, B.params, 0, threadIdx.x, NT);
    if (want_value) mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, NT);
    if constexpr (OPP == 3) mlp3_pack_fwd<S>(Wop, O.params, 0, threadIdx.x, NT);

    const int g0 = (int)blockIdx.x * GPB, ng = min(GPB, c.N - g0);
    const int gl = threadIdx.x / T, sub = threadIdx.x % T, game = g0 + gl;
    const int jw = lane >> 1;                              // my game's sample column inside the wave's tile
    const bool live = game < c.N, writer = live && sub == 0;

    uint4 hdr = make_uint4(0u, 0u, 0u, 0u);
    int dice = 1, tol = 0;
    double prev = 0.0;
    bool frozen = true;
    if (live) {
        hdr = *rng_hdr_ptr(B.rng, game);
        dice = B.dice[game];
        frozen = B.done[game] != 0;
        if (!EV && c.shaped) { tol = B.tolerance[game]; prev = B.prev_score[game]; }
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
    if ((FIX || B.t_rec) && rec0 && live) rec_store<S, T>(slot, sub, dice, 0, 0, 0, 0, 0, B.t_rec + (size_t)game * STR);
    double ret_acc = 0.0;
    int n_steps = 0, n_eps = 0, n_wins = 0;

    #pragma unroll 1
    for (int kstep = 0; kstep < c.K; kstep++) {
        if constexpr (EV) { if (__ballot(live && !frozen) == 0) break; }   // wave-uniform: every game of this wave is over
        const bool active = live && !frozen;
        double reward = 0.0;
        int term = 0, trunc = 0, info = EWN_INFO_NONE;
        if (live && frozen) term = 1;
        // ---- the network(s): this wave's 32 games are the 32 columns of the MFMA tiles (game j of the wave = column j, both lane halves);
        // the features come straight out of the games' slots: lane (j, h) turns bytes 16 kb + 8 h .. + 7 of game j's board into the eight
        // bf16 of its k-block operand (the slot's bytes past the board are zero) and sets the dice one-hot (features CELLS .. CELLS + 6)
        __builtin_amdgcn_wave_barrier();
        {
            const int j = lane & 31, h = lane >> 5;
            const int dj = __builtin_amdgcn_ds_bpermute((2 * j) << 2, dice);          // game j's dice (its lanes are 2 j, 2 j + 1)
            const int8_t *sj = slots + (wave * 32 + j) * STR + 8 * h;
            auto xb = [&](int kb) { return pol_obs_operand<S>(sj, kb, h, dj); };
            f32x16 h1[2], h2[2];
            float lo[MLP_NA];
            mlp3_forward<S, MLP_NA>(Wpi, lane, xb, h1, h2, lo);
            if (lane < 32) { *(float4 *)(LX + lane * 8) = make_float4(lo[0], lo[1], lo[2], lo[3]); LX[lane * 8 + 4] = lo[4]; }
            if (want_value) {
                float vo[1];
                mlp3_forward<S, 1>(Wvf, lane, xb, h1, h2, vo);
                if (lane < 32) LX[lane * 8 + 5] = vo[0];
            }
        }
        __builtin_amdgcn_wave_barrier();
        const float4 lg = *(const float4 *)(LX + jw * 8);
        const float lg4 = LX[jw * 8 + 4], val = LX[jw * 8 + 5];
        __builtin_amdgcn_wave_barrier();
        // ---- Gumbel-max sample (argmax of logits when deterministic): a[0] ~ softmax(l0, l1), a[1] ~ softmax(l2, l3, l4)
        // keyed by (episode, draws so far, lane) like the stand-in agents' hash, and by the tolerance left: an illegal move of the shaped
        // env (training_ewn.py:48-56) changes neither the observation nor the dice stream, and must not replay the same noise
        const u32 w0 = agent_hash(r.seed_mix() ^ ((u32)tol * 0x632BE5ABu), r.draws(), (u32)(c.lane_offset + game), c.key ^ c.noise_key);
        // the policy opponent's noise: the same hash under its own key, taken here, before the step moves the stream
        u32 w0o = 0u;
        if constexpr (OPP == 3)
            w0o = pol_opp_noise_word(r.seed_mix(), tol, r.draws(), c.lane_offset + game, c.key, O.noise_key);
        float u[5], gn[5];
        #pragma unroll
        for (int i = 0; i < 5; i++) { u[i] = pol_uniform(w0, i); gn[i] = deterministic ? 0.0f : pol_gumbel(u[i]); }
        const float z0 = lg.x + gn[0], z1 = lg.y + gn[1], z2 = lg.z + gn[2], z3 = lg.w + gn[3], z4 = lg4 + gn[4];
        const int aflag = pol_pick_flag(z0, z1);
        const int adir = pol_pick_dir(z2, z3, z4);
        if (!FIX && !EV && writer) {
            const size_t o = (size_t)kstep * c.N + game;
            if (B.t_logits) { float *p = B.t_logits + o * 5; p[0] = lg.x; p[1] = lg.y; p[2] = lg.z; p[3] = lg.w; p[4] = lg4; }
            if (B.t_value) B.t_value[o] = val;
            if (B.t_noise) { float *p = B.t_noise + o * 5; for (int i = 0; i < 5; i++) p[i] = u[i]; }
        }
        // ---- agent half, envs/ewn.py:438-458 / envs/training_ewn.py:44-66 (the agent is the canonical BOTTOM_RIGHT side)
        bool reply = false;
        if (active) {
            if constexpr (RNGK == 0) r.prefetch();
            r.begin_step();
            if constexpr (RNGK == 1) r.ps.prime();
            const int k = pk_cube(pk_sel<S>(Tb, s.posN, dice), aflag == 1);
            const int pb = pk_get(s.posN, k);
            const int q = Tb->nbn[adir][pb];
            if (q == 255) {
                if (!EV && c.shaped) { // an illegal move costs tolerance; the game goes on until it is used up (training_ewn.py:48-56)
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
        // ---- the opponent's search: run by every lane (lanes without a pending reply compute on a harmless state)
        int oflag = 0, odir = 0;
        if constexpr (OPP == 0) d3_search<S, T>(Tb, s, dice, sub, c.depth, oflag, odir);
        if constexpr (OPP == 2) d5_dispatch<S, T>(Tb, s, dice, sub, oflag, odir);
        const int odice = dice;                            // the opponent's dice where it replies
        if constexpr (OPP == 3) {
            // ---- the opponent's network on its canonical view of the same slots (pol_opp_operand, ewn_mlp3.hpp)
            __builtin_amdgcn_wave_barrier();               // the agent's moves are in the slots
            {
                const int j = lane & 31, h = lane >> 5;
                const int dj = __builtin_amdgcn_ds_bpermute((2 * j) << 2, dice);
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
            for (int i = 0; i < 5; i++) on[i] = O.deterministic ? 0.0f : pol_gumbel(pol_uniform(w0o, i));
            const float y0 = og.x + on[0], y1 = og.y + on[1], y2 = og.z + on[2], y3 = og.w + on[3], y4 = og4 + on[4];
            oflag = pol_pick_flag(y0, y1);
            odir = pol_pick_dir(y2, y3, y4);
        }
        if (reply) {
            const u32 e = pk_sel<S>(Tb, s.posP, dice);
            if constexpr (OPP == 1) {
                const u32 pp = pk_pair(s.posP, e);
                const u32 okm = (u32)Tb->lgp[pp & 0xFFu] | ((u32)Tb->lgp[pp >> 8] << 3);
                const int sl = Tb->nth[okm * 8u + (u32)r.randint(0, __popc(okm))];
                oflag = sl < 3 ? (int)(e >> 15) : 0;
                odir = sl < 3 ? sl : sl - 3;
            }
            if constexpr (OPP == 3) {   // a network may pick a move that leaves the board or a cube that is gone: envs/ewn.py:469-473
                const int k = pk_cube(e, oflag == 1);
                const int pb = pk_get(s.posP, k);
                const int q = Tb->nbp[odir][pb];
                if (q == 255) { reward = 0.0; term = 1; trunc = 1; info = EWN_INFO_INVALID_OPP; }
                else roll_opponent_move<S>(Tb, s, k, pb, q, dice, r, c.reward, reward, term, info, slot);
            } else
            roll_opponent_half<S>(Tb, s, e, oflag, odir, dice, r, c.reward, reward, term, info, slot);
            if (!EV && c.shaped && !term) { // reward = evaluate() - prev_score (training_ewn.py:94-96)
                const double cur = d3_shaped_score<S>(Tb, s);
                reward = cur - prev;
                prev = cur;
            }
        }
        if (active) {
            ret_acc += reward; n_steps++; n_eps += term; n_wins += info == EWN_INFO_WON ? 1 : 0;
            if (term) {
                if (!EV && c.autoreset) {
                    r.next_episode(B.rng, c.N, game, c.seed_stride, c.key, nullptr);
                    d3_init_state<S>(Tb, s);
                    rec_slot_init<S>(slot);
                    dice = r.first_dice(6);
                    if (!EV && c.shaped && c.refresh) prev = d3_shaped_score<S>(Tb, s);
                } else frozen = true;
            }
        }
        // ---- this step's trajectory row
        __builtin_amdgcn_wave_barrier();
        if constexpr (OPP == 3 && !FIX) {
            if ((EV ? active : live) && sub == 0 && O.t_action) {
                int8_t *p = O.t_action + ((size_t)kstep * c.N + game) * 3;
                p[0] = (int8_t)(reply ? odice : 0); p[1] = (int8_t)(reply ? oflag : 0); p[2] = (int8_t)(reply ? odir : 0);
            }
        }
        if constexpr (EV) {
            if (active && sub == 0 && B.t_action)
                ((uint16_t *)B.t_action)[(size_t)kstep * c.N + game] = (uint16_t)((uint8_t)aflag | ((uint16_t)(uint8_t)adir << 8));
        } else if (live) {
            const size_t o = (size_t)kstep * c.N + game;
            if constexpr (FIX) {
                if (sub == 0) B.t_reward[o] = reward;
            } else if (sub == 0) {
                if (B.t_action) ((uint16_t *)B.t_action)[o] = (uint16_t)((uint8_t)aflag | ((uint16_t)(uint8_t)adir << 8));
                if (B.t_dice) B.t_dice[o] = (int8_t)dice;
                if (B.t_reward) B.t_reward[o] = reward;
                if (B.t_term) B.t_term[o] = (uint8_t)term;
                if (B.t_trunc) B.t_trunc[o] = (uint8_t)trunc;
                if (B.t_info) B.t_info[o] = (uint8_t)info;
            }
            if (FIX || B.t_rec) rec_store<S, T>(slot, sub, dice, aflag, adir, term, trunc, info, B.t_rec + (o + (rec0 ? (size_t)c.N : 0)) * STR);
            if (!FIX && B.t_board && sub == 0) { int8_t *dst = B.t_board + o * CELLS; for (int i = 0; i < CELLS; i++) dst[i] = slot[i]; }
        }
    }
    // ---- the state goes back to HBM once, through the packed board area
    __syncthreads();
    if (live) d3_encode<S, T>(Tb, s, sub, slots + gl * CELLS);
    if (writer) {
        if (!frozen0) { *rng_hdr_ptr(B.rng, game) = r.header(); B.dice[game] = (int8_t)dice; }
        B.done[game] = frozen ? 1 : 0;
        if (!EV && c.shaped) { B.tolerance[game] = tol; B.prev_score[game] = prev; }
        if (B.ret_sum) B.ret_sum[game] += ret_acc;
        if (B.n_steps) B.n_steps[game] += n_steps;
        if (B.n_episodes) B.n_episodes[game] += n_eps;
        if (B.n_wins) B.n_wins[game] += n_wins;
    }
    __syncthreads();
    block_copy_out(B.board + (size_t)g0 * CELLS, slots, ng * CELLS);
