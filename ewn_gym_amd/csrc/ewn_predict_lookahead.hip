// ewn_predict_lookahead.hip -- one-ply lookahead on the trained critic (C ABI: ewn_predict_lookahead): what the actor-critic plays when
// it searches one agent move and one reply ahead and asks its own value net at the next agent-to-move state.  Plain expectiminimax, NO
// alpha-beta window: Q is a continuous function of the leaf values.  Per observation (b, d), agent = TOP_LEFT:
//   Q[f][r]   = -inf                              the move of cube find_cube_to_move(f) in direction r leaves the board
//             = +terminal_value                   b1 (the board after it) has the agent on the far corner or no opposing cube
//             = 1/6 sum_{d1} R(b1, d1)            otherwise
//   R(b1, d1) = min over BOTTOM_RIGHT's replies under d1 (cubes find_cube_to_move(True / False), directions that stay on the board) of
//   W(reply)  = -terminal_value                   b2 (the board after the reply) has the opponent on (0, 0) or no agent cube
//             = 1/6 sum_{d2} V(b2, d2)            otherwise; V = the value net, ewn_predict_policy's `value` for that observation
//   action    = the first maximum of Q in (f, r) order (strict >, as pol_pick_*)
// The dice only SELECTS among replies: a root has at most 6 cubes x 3 directions = 18 distinct replies, an observation 6 x 18 = 108 distinct
// b2, each evaluated under six d2: at most 648 columns of the value net, 21 MFMA tiles.  The leaf arithmetic is ewn_predict_policy's
// (mlp3_pack_fwd's image of net 1, pol_obs_operand on a zero-padded slot, mlp3_forward<S, 1>).  The observation in LDS, the roots
// and the fold of W into Q and the action are ewn_lookahead.hpp's helpers, the ones ewn_lookahead_stages.hip calls.
// ewn_predict_lookahead_eg is the same tree with W = terminal_value * E(b2) wherever an endgame table covers b2: the
// second instance of the one kernel below, k_predict_lookahead<S, true>.
#include "ewn_endgame.hpp"

#define LA_NT 256            // threads per block: four waves, one observation each per trip
#define LA_MAX_BLOCKS 256    // one block per CU (PRED_MAX_BLOCKS' reasoning); more observations than that are walked grid-stride
#define LA_NONE (-1)         // a tuple's meta byte: no such reply (or a root that is not searched) ...
#define LA_LOST (-2)         // ... a reply that wins for the opponent; >= 0: the b2's leaf slot
#define LA_EXACT (-3)        // k_predict_lookahead<S, true> only: a b2 the endgame table covers -- no leaf slot, no columns, W from the table

// LDS of k_predict_lookahead<S>: the value net's image | per wave: the observation as a slot | cube positions | tuple meta | W | R | Q |
// V [648] | 108 leaf slots of RecGeo<S>::STR bytes
template <int S> struct LaGeo {
    static constexpr int CELLS = S * S, STR = RecGeo<S>::STR, NW = LA_NT / 64;
    static constexpr int O_BASE = 0;                          // the observation's board, zero past the board (a slot: copied whole)
    static constexpr int O_POS = O_BASE + STR;                // [16] cell of agent cube k at k, of opposing cube k at 8 + k; 0xFF: absent
    static constexpr int O_META = O_POS + 16;                 // [108] int8, padded to 112
    static constexpr int O_W = O_META + 112;                  // [108] float: W(reply), +inf where there is none
    static constexpr int O_R = O_W + LA_TUPLES * 4;           // [36] float: R(root, d1)
    static constexpr int O_Q = O_R + 36 * 4;                  // [6] float, padded to 8
    static constexpr int O_V = O_Q + 8 * 4;                   // [648] float: V(leaf slot, d2) at 6 slot + d2 - 1
    static constexpr int O_SLOTS = O_V + LA_TUPLES * 6 * 4;
    static constexpr int WAVE_BYTES = O_SLOTS + LA_TUPLES * STR;
    static_assert(CELLS <= 64, "one lane per cell");
    static_assert(STR % 16 == 0 && WAVE_BYTES % 16 == 0, "every region starts on a 16-byte boundary");
    static constexpr size_t lds_bytes() { return (size_t)Mlp3Geo<S>::FWD_BYTES + (size_t)NW * WAVE_BYTES; }
};

struct LaBuf { const int8_t *boards; const int8_t *dice; const float *params; int8_t *actions; float *q; };
// a kernel's buffers: the plain instance's are LaBuf and nothing else; the instance with a table adds the table (layout 1), its
// max_cubes and max_total, and leaf_counts [M][2] or NULL: {leaves valued by the table, by the critic}
template <bool EG> struct LaArgs : LaBuf {};
template <> struct LaArgs<true> : LaBuf { int K, T; const float *table; int16_t *counts; };

// Everything is per wave; nothing after the pack crosses a wave, so there is no block barrier in the loop.  Phases per observation:
// (a) lanes enumerate the 108 tuples (two per lane) and write each distinct non-terminal b2 into the next free leaf slot (ballot
// ranks); (b) the value net over tiles of 32 columns, column = 6 slot + d2 - 1; (c) W per tuple, then la_fold: R per (root, d1), Q per
// root, the pick, the stores.
// EG: in (a) the lane of a tuple whose b2 the table covers -- 1 .. K cubes a side, at most T in all; a leaf never has an
// agent cube on C - 1 (that root wins, or the row is over) nor an opposing cube on 0 (that reply is LA_LOST, or the row is over) --
// forms the table index from its registers and the 16-byte position table and issues the gather; it takes no leaf slot, so the ranks
// and ncol count the critic's leaves only, and (c) consumes the loaded E behind (b)'s tiles.  Every index lies inside the table: a
// move never adds a cube and the coverage test comes first (eg_move's argument).  A root with a cube number twice on a side, or a
// cell outside -6 .. 6, is no position of the table's: its cells outnumber its presence masks, and every leaf goes to the critic.
template <int S, bool EG>
__global__ __launch_bounds__(LA_NT, 1) void k_predict_lookahead(int M, float tv, LaArgs<EG> B)
{
    using P = LaGeo<S>;
    using Q3 = Mlp3Geo<S>;
    constexpr int CELLS = P::CELLS, STR = P::STR;
    static_assert(Q3::FWD_BYTES % 16 == 0, "image alignment");
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t *Wvf = lds;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *mine = lds + Q3::FWD_BYTES + wave * P::WAVE_BYTES;
    int8_t *base = mine + P::O_BASE, *meta = mine + P::O_META, *slots = mine + P::O_SLOTS;
    uint8_t *pos = (uint8_t *)(mine + P::O_POS);
    float *Wt = (float *)(mine + P::O_W), *Rt = (float *)(mine + P::O_R), *Qt = (float *)(mine + P::O_Q), *Vt = (float *)(mine + P::O_V);
    mlp3_pack_fwd<S>(Wvf, B.params, 1, threadIdx.x, LA_NT);
    __syncthreads();

    const float inf = __builtin_inff();
    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * P::NW + wave; m0 < M; m0 += (int)gridDim.x * P::NW) {   // wave-uniform
        const size_t m = (size_t)m0;
        int PA, PO;
        const int d = la_dice((int)B.dice[m]);
        const bool live = la_observation<S, STR>(B.boards + m * CELLS, lane, base, pos, PA, PO);
        if (!live) {
            if constexpr (EG) { if (B.counts && lane < 2) B.counts[m * 2 + lane] = 0; }
            la_row_over(B.actions, B.q, m, lane);
            continue;
        }
        const int c0 = la_find(0, d, PA), c1 = la_find(1, d, PA);
        bool eg_row = false;                                   // wave-uniform
        float ev[2] = {0.0f, 0.0f};                            // E(b2) of this lane's covered tuples: loaded in (a), read in (c)
        if constexpr (EG) {
            const int ncell = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < CELLS && base[lane < CELLS ? lane : 0] != 0));
            eg_row = ncell == __builtin_popcount((unsigned)PA) + __builtin_popcount((unsigned)PO);
        }

        // ---- (a) tuple t = lane + 64 half: the reply of cube k in direction e to root `root`
        int mt[2];
        int src0[2], dst0[2], cub0[2], src1[2], dst1[2], cub1[2];
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            const int t = lane + 64 * half, root = t / LA_REPLIES, k = (t % LA_REPLIES) / 3 + 1, e = t % 3;
            mt[half] = LA_NONE; src0[half] = dst0[half] = cub0[half] = src1[half] = dst1[half] = cub1[half] = 0;
            if (t < LA_TUPLES && la_searched(root, c0, c1) == root) {
                const LaRoot R = la_root<S>(base, pos, PA, PO, c0, c1, root);
                if (R.code == 2 && ((R.PO1 >> k) & 1)) {
                    const int s1 = pos[8 + k], x1 = s1 / S, y1 = s1 % S;
                    if ((e == 1 || y1 > 0) && (e == 0 || x1 > 0)) {
                        const int t1 = s1 - (e == 0 ? 1 : e == 1 ? S : S + 1);
                        const int v1 = t1 == R.dst ? R.cube : t1 == R.src ? 0 : (int)base[t1];   // b1[t1]: what the reply captures
                        const int PA2 = R.PA1 & ~(v1 > 0 ? 1 << (v1 & 7) : 0);
                        mt[half] = (t1 == 0 || PA2 == 0) ? LA_LOST : 0;
                        src0[half] = R.src; dst0[half] = R.dst; cub0[half] = R.cube; src1[half] = s1; dst1[half] = t1; cub1[half] = -k;
                        if constexpr (EG) {
                            const int PO2 = R.PO1 & ~(v1 < 0 ? 1 << (-v1 & 7) : 0);   // a reply captures its own side's cubes too
                            const int na = __builtin_popcount((unsigned)PA2), no = __builtin_popcount((unsigned)PO2);   // both >= 1 on a leaf
                            if (eg_row && mt[half] == 0 && na <= B.K && no <= B.K && na + no <= B.T) {
                                // cube k's cell in byte k - 1 (eg_cell): pos[1 .. 6] and pos[9 .. 14], the two moved cubes at their targets
                                const int sa = 8 * (R.cube - 1), so = 8 * (k - 1);
                                const u64 pa = ((*(const u64 *)pos >> 8) & ~(0xFFull << sa)) | ((u64)R.dst << sa);
                                const u64 po = ((*(const u64 *)(pos + 8) >> 8) & ~(0xFFull << so)) | ((u64)t1 << so);
                                // no load but the gather itself (eg_rank, eg_off): nothing waits on it before (c)
                                ev[half] = B.table[eg_off<S>(B.K, B.T, na, no) + (long long)eg_side_of<S>(eg_rank(PA2), PA2, pa, false) * (long long)eg_n<S>(no)
                                                   + (long long)eg_side_of<S>(eg_rank(PO2), PO2, po, false)];
                                mt[half] = LA_EXACT;
                            }
                        }
                    }
                }
            }
        }
        const u64 leaf0 = __builtin_amdgcn_ballot_w64(mt[0] == 0), leaf1 = __builtin_amdgcn_ballot_w64(mt[1] == 0);
        const int n0 = __builtin_popcountll(leaf0), nleaf = n0 + __builtin_popcountll(leaf1);   // <= 108
        if constexpr (EG) {
            const int nex = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mt[0] == LA_EXACT)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(mt[1] == LA_EXACT));
            if (B.counts && lane < 2) B.counts[m * 2 + lane] = (int16_t)(lane == 0 ? nex : nleaf);
        }
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            const u64 bal = half ? leaf1 : leaf0;
            const int rank = (half ? n0 : 0) + (int)__builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
            const int t = lane + 64 * half;
            if (mt[half] == 0) {                               // b2 = the observation with the two moves applied, in their order
                int8_t *sl = slots + rank * STR;
                #pragma unroll
                for (int w = 0; w < STR / 4; w++) ((u32 *)sl)[w] = ((const u32 *)base)[w];
                sl[src0[half]] = 0; sl[dst0[half]] = (int8_t)cub0[half];
                sl[src1[half]] = 0; sl[dst1[half]] = (int8_t)cub1[half];
                mt[half] = rank;
            }
            if (t < LA_TUPLES) meta[t] = (int8_t)mt[half];
        }
        __builtin_amdgcn_wave_barrier();

        // ---- (b) the value net: 32 columns per tile (both lane halves hold column lane & 31), column c = leaf slot c / 6 under d2 = c % 6 + 1
        const int ncol = 6 * nleaf, j = lane & 31, h = lane >> 5;
        #pragma unroll 1
        for (int c00 = 0; c00 < ncol; c00 += 32) {             // wave-uniform
            const int c = c00 + j;
            const bool live = c < ncol;
            const int slot = live ? c / 6 : 0, dj = live ? c % 6 + 1 : 0;   // a column past the last: slot 0 (written: nleaf >= 1), no dice
            const int8_t *sj = slots + slot * STR + 8 * h;
            auto xb = [&](int kb) { return pol_obs_operand<S>(sj, kb, h, dj); };
            f32x16 h1[2], h2[2];
            float vo[1];
            mlp3_forward<S, 1>(Wvf, lane, xb, h1, h2, vo);
            if (live && h == 0) Vt[c] = vo[0];
        }
        __builtin_amdgcn_wave_barrier();

        // ---- (c) W per tuple: the mean over d2, in d2 order
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            const int t = lane + 64 * half;
            if (t < LA_TUPLES) {
                const int mm = meta[t];
                float w = mm == LA_NONE ? inf : -tv;
                if (mm >= 0) {
                    const float *v = Vt + 6 * mm;
                    w = (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) * (1.0f / 6.0f);
                }
                if constexpr (EG) { if (mm == LA_EXACT) w = tv * ev[half]; }
                Wt[t] = w;
            }
        }
        __builtin_amdgcn_wave_barrier();
        la_fold<S>(base, pos, PA, PO, c0, c1, Wt, Rt, Qt, tv, B.actions, B.q, m, lane);
    }
}

template <int S>
static int la_launch(int M, float tv, const LaBuf &lb, hipStream_t s)
{
    constexpr size_t lds = LaGeo<S>::lds_bytes();
    static_assert(lds <= POL_LDS_MAX, "the value net's image + four waves' slots and tables must fit the CU's LDS");
    return pol_launch_kernel(k_predict_lookahead<S, false>, la_blocks(M, LaGeo<S>::NW, LA_MAX_BLOCKS), LA_NT, lds, 64 * 1024, POL_LDS_MAX, s, M, tv,
                             LaArgs<false>{lb});
}

template <int S>
static int la_launch_eg(int M, float tv, const LaArgs<true> &a, hipStream_t s)
{
    return pol_launch_kernel(k_predict_lookahead<S, true>, la_blocks(M, LaGeo<S>::NW, LA_MAX_BLOCKS), LA_NT, LaGeo<S>::lds_bytes(), 64 * 1024, POL_LDS_MAX,
                             s, M, tv, a);
}

// ewn_predict_policy's order of refusals: arguments, geometry, the empty batch, pointers; then the terminal value -- all before the launch
int ewn_predict_lookahead(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const float *params,
                          float terminal_value, int8_t *actions, float *q, void *stream)
{
    if (M < 0) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (M == 0) return EWN_OK;
    if (!boards || !dice || !params || !actions) return EWN_ENULL;
    if (!std::isfinite(terminal_value)) return EWN_EINVAL;
    LaBuf lb = { boards, dice, params, actions, q };
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? la_launch<5>(M, terminal_value, lb, s) : la_launch<7>(M, terminal_value, lb, s);
}

// ewn_predict_lookahead's order with the table's parameters after the geometry (ewn_endgame_table_bytes' refusal)
int ewn_predict_lookahead_eg(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const float *params,
                             float terminal_value, int max_cubes, int max_total, const float *table, int8_t *actions, float *q,
                             int16_t *leaf_counts, void *stream)
{
    if (M < 0) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (M == 0) return EWN_OK;
    if (!boards || !dice || !params || !table || !actions) return EWN_ENULL;
    if (!std::isfinite(terminal_value)) return EWN_EINVAL;
    LaBuf lb = { boards, dice, params, actions, q };
    LaArgs<true> a = { lb, max_cubes, max_total, table, leaf_counts };
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? la_launch_eg<5>(M, terminal_value, a, s) : la_launch_eg<7>(M, terminal_value, a, s);
}
