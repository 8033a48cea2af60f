// ewn_lookahead_stages.hip -- the two ends of ewn_predict_lookahead's tree as kernels of their own (C ABI: ewn_lookahead_expand,
// ewn_lookahead_reduce).  expand writes every (agent move, reply) tuple's b2 under the six d2 out as observations, with a
// kind byte per tuple; reduce folds a value per such observation back into Q and the action.  Both read the tree through the helpers
// k_predict_lookahead reads it through (ewn_lookahead.hpp: la_observation, la_root, la_fold), so the chain is that kernel's arithmetic.
// Between them the caller evaluates the leaves with what it likes: the plain critic (ewn_predict_policy's value: the chain then IS
// ewn_predict_lookahead) or ewn_predict_lookahead itself (its q rows: a two-move lookahead).  No network runs here.
#include "ewn_lookahead.hpp"
#include <climits>

#define LS_NT 256            // threads per block: four waves, one observation each per trip
#define LS_MAX_BLOCKS 1024   // four blocks per CU (both kernels are light on registers and LDS); more observations are walked grid-stride
#define LS_ROWS (LA_TUPLES * 6)   // leaf rows per observation: row = 6 t + d2 - 1

// per wave: the observation's board (64 bytes, zero past the board) | cube positions [16] | then the kernel's own tables
#define LS_O_POS 64
#define LS_O_OWN 80
#define LS_EXPAND_WAVE (LS_O_OWN + LA_TUPLES * 8)                    // [108] tuple records of 8 bytes
#define LS_REDUCE_WAVE (LS_O_OWN + LA_TUPLES * 4 + 36 * 4 + 8 * 4)   // W [108] | R [36] | Q [6], padded to 8

struct LsExpandBuf { const int8_t *boards; const int8_t *dice; int8_t *leaf_boards; int8_t *leaf_dice; int8_t *kind; };
struct LsReduceBuf { const int8_t *boards; const int8_t *dice; const int8_t *kind; const float *leaf; int8_t *actions; float *q; };

// A tuple's record: lo = kind | src0 << 8 | dst0 << 16 | cube0 << 24 (the agent's move), hi = src1 | dst1 << 8 | cube1 << 16 (the reply,
// cube1 = -k as a byte); all zero unless kind == 2.  Every one of the 648 rows of the observation is stored on every trip.
template <int S>
__global__ __launch_bounds__(LS_NT) void k_lookahead_expand(int M, LsExpandBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(LS_NT / 64) * LS_EXPAND_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * LS_EXPAND_WAVE;
    uint8_t *pos = (uint8_t *)(base + LS_O_POS);
    uint2 *rec = (uint2 *)(base + LS_O_OWN);

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (LS_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (LS_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        int PA, PO;
        const bool live = la_observation<S, 64>(B.boards + m * CELLS, lane, base, pos, PA, PO);
        const int d = la_dice((int)B.dice[m]);
        const int c0 = live ? la_find(0, d, PA) : 0, c1 = live ? la_find(1, d, PA) : 0;
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            const int t = lane + 64 * half, root = t / LA_REPLIES, k = (t % LA_REPLIES) / 3 + 1, e = t % 3;
            u32 lo = 0, hi = 0;
            if (live && t < LA_TUPLES && !(root >= 3 && c1 == c0)) {   // both flags name one cube: roots 3 .. 5 are roots 0 .. 2
                const LaRoot R = la_root<S>(base, pos, PA, PO, c0, c1, root);
                if (R.code == 2 && ((R.PO1 >> k) & 1)) {
                    const int s1 = pos[8 + k], x1 = s1 / S, y1 = s1 % S;
                    if ((e == 1 || y1 > 0) && (e == 0 || x1 > 0)) {
                        const int t1 = s1 - (e == 0 ? 1 : e == 1 ? S : S + 1);
                        const int v1 = t1 == R.dst ? R.cube : t1 == R.src ? 0 : (int)base[t1];   // b1[t1]: what the reply captures
                        const int PA2 = R.PA1 & ~(v1 > 0 ? 1 << (v1 & 7) : 0);
                        if (t1 == 0 || PA2 == 0) lo = 1u;
                        else {
                            lo = 2u | (u32)R.src << 8 | (u32)R.dst << 16 | (u32)R.cube << 24;
                            hi = (u32)s1 | (u32)t1 << 8 | ((u32)(-k) & 0xFFu) << 16;
                        }
                    }
                }
            }
            if (t < LA_TUPLES) {
                rec[t] = make_uint2(lo, hi);
                B.kind[m * LA_TUPLES + t] = (int8_t)(lo & 0xFFu);
            }
        }
        __builtin_amdgcn_wave_barrier();
        // the rows: byte i of the observation's 648 boards is cell i % CELLS of row i / CELLS, b2 = the observation with the two moves
        // applied in their order (so the later store wins: dst1, src1, dst0, src0), zero where the tuple is no leaf
        int8_t *out = B.leaf_boards + m * (size_t)(LS_ROWS * CELLS);
        #pragma unroll 1
        for (int i = lane; i < LS_ROWS * CELLS; i += 64) {
            const int row = i / CELLS, c = i - row * CELLS;
            const uint2 r = rec[row / 6];
            const int s0 = (int)(r.x >> 8 & 0xFFu), t0 = (int)(r.x >> 16 & 0xFFu), s1 = (int)(r.y & 0xFFu), t1 = (int)(r.y >> 8 & 0xFFu);
            int v = base[c];
            v = c == s0 ? 0 : v;
            v = c == t0 ? (int)(r.x >> 24) : v;
            v = c == s1 ? 0 : v;
            v = c == t1 ? (int)(int8_t)(r.y >> 16 & 0xFFu) : v;
            out[i] = (int8_t)((r.x & 0xFFu) == 2u ? v : 0);
        }
        int8_t *od = B.leaf_dice + m * (size_t)LS_ROWS;
        #pragma unroll 1
        for (int i = lane; i < LS_ROWS; i += 64) od[i] = (int8_t)(i % 6 + 1);
        __builtin_amdgcn_wave_barrier();                       // this trip's LDS is read: the next may overwrite it
    }
}

// 4k's phase (c) on leaf values handed in: W per tuple, then la_fold (R per (root, d1), Q per root, the pick).  WIDTH entries per leaf
// row, the row's value their maximum.  The roots are read off the observation again; `kind` only selects among values, it never indexes.
template <int S, int WIDTH>
__global__ __launch_bounds__(LS_NT) void k_lookahead_reduce(int M, float tv, LsReduceBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(LS_NT / 64) * LS_REDUCE_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * LS_REDUCE_WAVE;
    uint8_t *pos = (uint8_t *)(base + LS_O_POS);
    float *Wt = (float *)(base + LS_O_OWN), *Rt = Wt + LA_TUPLES, *Qt = Rt + 36;

    const float inf = __builtin_inff();
    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (LS_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (LS_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        int PA, PO;
        const bool live = la_observation<S, 64>(B.boards + m * CELLS, lane, base, pos, PA, PO);
        const int d = la_dice((int)B.dice[m]);
        if (!live) { la_row_over(B.actions, B.q, m, lane); continue; }
        const int c0 = la_find(0, d, PA), c1 = la_find(1, d, PA);

        // W per tuple: the mean over d2 of the row's value, in d2 order
        #pragma unroll
        for (int half = 0; half < 2; half++) {
            const int t = lane + 64 * half;
            if (t < LA_TUPLES) {
                const int kd = B.kind[m * LA_TUPLES + t];
                float w = kd == 0 ? inf : -tv;
                if (kd == 2) {
                    const float *lf = B.leaf + (m * LA_TUPLES + t) * (size_t)(6 * WIDTH);
                    float v[6];
                    #pragma unroll
                    for (int j = 0; j < 6; j++) {
                        float x = lf[j * WIDTH];
                        #pragma unroll
                        for (int i = 1; i < WIDTH; i++) { const float y = lf[j * WIDTH + i]; x = y > x ? y : x; }
                        v[j] = x;
                    }
                    w = (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) * (1.0f / 6.0f);
                }
                Wt[t] = w;
            }
        }
        __builtin_amdgcn_wave_barrier();
        la_fold<S>(base, pos, PA, PO, c0, c1, Wt, Rt, Qt, tv, B.actions, B.q, m, lane);
    }
}

template <class Kern, class... Args>
static int ls_launch(Kern kern, int M, hipStream_t s, const Args &...args)
{
    return pol_launch_kernel(kern, la_blocks(M, LS_NT / 64, LS_MAX_BLOCKS), LS_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, args...);
}

// ewn_predict_lookahead's order of refusals: arguments, geometry, the empty batch, pointers; then the values -- all before the launch
int ewn_lookahead_expand(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, int8_t *leaf_boards,
                         int8_t *leaf_dice, int8_t *kind, void *stream)
{
    if (M < 0 || (long long)M * LS_ROWS > INT_MAX) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (M == 0) return EWN_OK;
    if (!boards || !dice || !leaf_boards || !leaf_dice || !kind) return EWN_ENULL;
    LsExpandBuf eb = { boards, dice, leaf_boards, leaf_dice, kind };
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? ls_launch(k_lookahead_expand<5>, M, s, eb) : ls_launch(k_lookahead_expand<7>, M, s, eb);
}

int ewn_lookahead_reduce(int board_size, int cube_layer, int M, const int8_t *boards, const int8_t *dice, const int8_t *kind,
                         const float *leaf, int leaf_width, float terminal_value, int8_t *actions, float *q, void *stream)
{
    if (M < 0 || (long long)M * LS_ROWS > INT_MAX) return EWN_EINVAL;
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (M == 0) return EWN_OK;
    if (!boards || !dice || !kind || !leaf || !actions) return EWN_ENULL;
    if (!std::isfinite(terminal_value) || (leaf_width != 1 && leaf_width != 6)) return EWN_EINVAL;
    LsReduceBuf rb = { boards, dice, kind, leaf, actions, q };
    hipStream_t s = (hipStream_t)stream;
    const float tv = terminal_value;
    if (board_size == 5)
        return leaf_width == 1 ? ls_launch(k_lookahead_reduce<5, 1>, M, s, tv, rb) : ls_launch(k_lookahead_reduce<5, 6>, M, s, tv, rb);
    return leaf_width == 1 ? ls_launch(k_lookahead_reduce<7, 1>, M, s, tv, rb) : ls_launch(k_lookahead_reduce<7, 6>, M, s, tv, rb);
}
