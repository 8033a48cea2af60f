// ewn_endgame.hip -- exact endgame values (C ABI: ewn_endgame_table_bytes, ewn_endgame_build, ewn_endgame_lookup).
// A position is seen from the side to move, before its dice: the mover is TOP_LEFT (positive cubes, goal cell C - 1, C = S * S).
//   E(b) = fl((m_1 + ... + m_6) * fl(1/6))            fp32, summed in dice order
//   m_d  = max over f in {0, 1}, r in {0, 1, 2} whose move stays on the board of G(b, d, f, r)
//   G    = +1 if the move wins (it reaches C - 1 or leaves the other side without a cube), else -E(flip(b1)), b1 the board after it;
//          flip turns the board by 180 degrees and swaps the sides.  The cube is find_cube_to_move(f) under d (la_find), and the move
//          captures whatever stands on its target, own cubes included (la_root's rules).
// Every ply lowers Phi(b) = the sum over all cubes of the Manhattan distance to the cube's own corner by at least 1, so the table is
// filled level by level in Phi: a launch reads only entries of lower levels, which earlier launches on the same stream wrote.  No
// atomics, no flag, no entry read in the launch that writes it.
//
// Table layout (version 1, EndgameTable.LAYOUT in ewn_gym_amd/endgame.py): a block per (ka, ko), ka-major, over 1 <= ka, ko <= K with
// ka + ko <= T; inside it entry = side(agent) * n_ko + side(opponent), n_k = binom(6, k) * C^k;
// side = rank of the 6-bit presence mask among the masks of its popcount (ascending) * C^k + the cells in cube-number order as a
// base-C number, lowest cube number most significant.  Slots of positions that are not live (cubes sharing a cell, an agent cube on
// C - 1, an opposing cube on 0) are never read; the build writes 0 there (the whole table is cleared first).
#define EG_MASKS_LINKAGE    // EG_MASKS is this unit's own symbol; every other unit's copy is static
#include "ewn_endgame.hpp"

#define EG_NT 256            // threads per block of both kernels
#define EG_MAX_BLOCKS 9      // (ka, ko) blocks of a table: K <= 3
#define EG_MAX_GRID (1u << 22)   // workgroups per launch: a launch's grid is 32 bits of THREADS (2^24 workgroups of EG_NT), see eg_build

// E from the best move of each cube: m_d = max(best[cube of flag 0], best[cube of flag 1]); max is exact, so this is the definition's
// maximum over (f, r) bit for bit
template <int S>
EWN_DEV float eg_value(const float *tbl, const EgGeo &g, int Ma, int Mo, u64 pa, u64 po)
{
    float best[3] = {0.0f, 0.0f, 0.0f};                            // per cube of Ma, in cube-number order (K <= 3)
    int m = Ma;
    #pragma unroll 1
    for (int j = 0; j < 3 && m; j++, m &= m - 1) {
        const int k = __builtin_ctz(m);
        float b = -__builtin_inff();
        #pragma unroll
        for (int r = 0; r < 3; r++) { const float q = eg_move<S>(tbl, g, Ma, Mo, pa, po, k, r); b = q > b ? q : b; }
        best[0] = j == 0 ? b : best[0]; best[1] = j == 1 ? b : best[1]; best[2] = j == 2 ? b : best[2];
    }
    float sum = 0.0f;
    #pragma unroll
    for (int d = 1; d <= 6; d++) {
        const int j0 = __builtin_popcount((unsigned)(Ma & ((1 << la_find(0, d, Ma)) - 1))), j1 = __builtin_popcount((unsigned)(Ma & ((1 << la_find(1, d, Ma)) - 1)));
        const float m0 = j0 == 0 ? best[0] : j0 == 1 ? best[1] : best[2], m1 = j1 == 0 ? best[0] : j1 == 1 ? best[1] : best[2];
        const float md = m1 > m0 ? m1 : m0;
        sum = d == 1 ? md : sum + md;
    }
    return sum * (1.0f / 6.0f);
}

// a side index decoded: false where two of its cubes share a cell or a cell of `occ` (the other side's), or a cube stands on `bad`.
// phi: the sum of the cubes' Manhattan distances to their corner (far_goal: cell C - 1, else cell 0)
template <int S>
EWN_DEV bool eg_decode(u32 i, int k, int bad, bool far_goal, u64 &occ0, u64 &occ1, int &M, u64 &pos, int &phi)
{
    constexpr int C = S * S;
    const u32 pw = eg_pw<S>(k);
    u32 rem = i % pw;
    M = (int)EG_MASKS.unrank[k][i / pw] << 1;
    pos = 0; phi = 0;
    bool ok = true;
    int m = M;
    #pragma unroll
    for (int j = 0; j < 3; j++) {
        if (j < k) {
            const int cube = 31 - __builtin_clz((unsigned)m);    // the highest cube number holds the least significant digit
            m &= ~(1 << cube);
            const int c = (int)(rem % (u32)C);
            rem /= (u32)C;
            const int x = c / S, y = c % S;
            phi += far_goal ? (S - 1 - x) + (S - 1 - y) : x + y;
            const u64 bit = 1ull << (c & 63);
            const bool hi = c >= 64;
            ok = ok && c != bad && !((hi ? occ1 : occ0) & bit);
            occ0 |= hi ? 0ull : bit; occ1 |= hi ? bit : 0ull;
            pos |= (u64)c << (8 * (cube - 1));
        }
    }
    return ok;
}

struct EgLevel {
    int level, nblk;
    u32 first;                                                  // the level's workgroup that this launch's blockIdx.x = 0 is
    struct { int ka, ko; u32 wg0, chunks; } b[EG_MAX_BLOCKS];   // workgroups wg0 .. : chunks per agent side index, EG_NT opposing side indices per chunk
};

// One Phi level.  A workgroup holds one agent side and EG_NT consecutive opposing sides, so the agent half of the decode is uniform
// and an agent side that is invalid or already too far for this level retires the whole workgroup.
template <int S>
__global__ __launch_bounds__(EG_NT) void k_endgame_level(float *tbl, EgGeo g, EgLevel L)
{
    constexpr int C = S * S;
    const u32 wg = L.first + blockIdx.x;
    int bi = 0;
    #pragma unroll 1
    for (int i = 1; i < L.nblk; i++) if (wg >= L.b[i].wg0) bi = i;
    const int ka = L.b[bi].ka, ko = L.b[bi].ko;
    const u32 local = wg - L.b[bi].wg0, chunks = L.b[bi].chunks;
    const u32 ia = local / chunks, io = (local % chunks) * EG_NT + threadIdx.x;
    u64 occ0 = 0ull, occ1 = 0ull;
    int Ma, Mo, phia, phio;
    u64 pa, po;
    if (!eg_decode<S>(ia, ka, C - 1, true, occ0, occ1, Ma, pa, phia)) return;
    const int want = L.level - phia;
    if (want < ko || want > ko * 2 * (S - 1) || io >= eg_n<S>(ko)) return;
    if (!eg_decode<S>(io, ko, 0, false, occ0, occ1, Mo, po, phio) || phio != want) return;
    tbl[g.off[ka][ko] + (long long)ia * (long long)eg_n<S>(ko) + (long long)io] = eg_value<S>(tbl, g, Ma, Mo, pa, po);
}

// The build's clear.  A kernel and not hipMemsetAsync: captured into a hipGraph, a memset node of value 0 is not replayed faithfully
// by the ROCm 7.0 runtime (from the second replay on it writes an 8-byte pattern that is not zero; tests/test_gpu_stream_contract.py).
// A table is 4-byte aligned only: `head` entries (0 .. 3) up to the first 16-byte boundary, n4 groups of four, `tail` entries (0 .. 3).
#define EG_CLEAR_BLOCKS 2048
__global__ __launch_bounds__(EG_NT) void k_endgame_clear(float *tbl, int head, long long n4, int tail)
{
    const long long id = (long long)blockIdx.x * EG_NT + threadIdx.x, stride = (long long)gridDim.x * EG_NT;
    float4 *body = (float4 *)(tbl + head);
    for (long long i = id; i < n4; i += stride) body[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (id < head) tbl[id] = 0.0f;
    if (id < tail) tbl[head + 4 * n4 + id] = 0.0f;
}

struct EgLookBuf { const float *tbl; const int8_t *boards; const int8_t *dice; int8_t *actions; float *q; float *value; uint8_t *covered; };

// a lane per observation: the work is a handful of dependent gathers, nothing a wave could share
template <int S>
__global__ __launch_bounds__(EG_NT) void k_endgame_lookup(int M, EgGeo g, EgLookBuf B)
{
    constexpr int C = S * S;
    const long long m = (long long)blockIdx.x * EG_NT + threadIdx.x;
    if (m >= M) return;
    const int8_t *b = B.boards + m * C;
    int Ma, Mo, na, no;
    u64 pa, po;
    const bool ok = eg_position<S>(b, g.K, g.T, Ma, Mo, na, no, pa, po);
    const int d = la_dice((int)B.dice[m]);
    const float ninf = -__builtin_inff();
    float q[6] = {ninf, ninf, ninf, ninf, ninf, ninf}, val = 0.0f;
    int best = 0;
    if (ok) {
        const int c0 = la_find(0, d, Ma), c1 = la_find(1, d, Ma);
        #pragma unroll
        for (int r = 0; r < 3; r++) q[r] = eg_move<S>(B.tbl, g, Ma, Mo, pa, po, c0, r);
        #pragma unroll
        for (int r = 0; r < 3; r++) q[3 + r] = c1 == c0 ? q[r] : eg_move<S>(B.tbl, g, Ma, Mo, pa, po, c1, r);
        float qb = q[0];
        #pragma unroll
        for (int i = 1; i < 6; i++) if (q[i] > qb) { qb = q[i]; best = i; }
        if (B.value) val = B.tbl[g.off[na][no] + (long long)eg_side<S>(Ma, pa, false) * (long long)eg_n<S>(no) + (long long)eg_side<S>(Mo, po, false)];
    }
    B.actions[m * 2] = (int8_t)(best / 3); B.actions[m * 2 + 1] = (int8_t)(best % 3);
    if (B.q) {
        #pragma unroll
        for (int i = 0; i < 6; i++) B.q[m * 6 + i] = q[i];
    }
    if (B.value) B.value[m] = val;
    if (B.covered) B.covered[m] = ok ? 1 : 0;
}

// ---------------------------------------------------------------- host
// the active (ka, ko) blocks of a level and its grid: EG_NT entries a workgroup, rounded up per agent side.  0: nothing at this level
static unsigned long long eg_level(int S, int K, int T, int level, EgLevel &L)
{
    memset(&L, 0, sizeof(L));
    L.level = level;
    unsigned long long wg = 0;
    for (int a = 1; a <= K; a++)
        for (int o = 1; o <= K; o++) {
            if (a + o > T || level < a + o || level > (a + o) * 2 * (S - 1)) continue;
            const unsigned long long chunks = (unsigned long long)(eg_n_host(S, o) + EG_NT - 1) / EG_NT;
            if (wg > 0x7FFFFFFFull) return wg;
            L.b[L.nblk].ka = a; L.b[L.nblk].ko = o; L.b[L.nblk].wg0 = (u32)wg; L.b[L.nblk].chunks = (u32)chunks;
            L.nblk++;
            wg += chunks * (unsigned long long)eg_n_host(S, a);
        }
    return wg;
}

template <int S>
static int eg_build(int K, int T, float *table, long long entries, const EgGeo &g, hipStream_t s)
{
    EgLevel L;
    for (int level = 2; level <= 2 * T * (S - 1); level++)       // every level's grid must fit before anything is launched
        if (eg_level(S, K, T, level, L) > 0x7FFFFFFFull) return EWN_EUNSUPPORTED;
    {
        const long long to16 = (long long)(((16 - ((uintptr_t)table & 15)) & 15) / sizeof(float));
        const long long head = to16 < entries ? to16 : entries, n4 = (entries - head) / 4, tail = entries - head - 4 * n4;
        const long long need = (n4 + EG_NT - 1) / EG_NT;
        k_endgame_clear<<<dim3((unsigned)(need < 1 ? 1 : (need < EG_CLEAR_BLOCKS ? need : EG_CLEAR_BLOCKS))), dim3(EG_NT), 0, s>>>(table, (int)head, n4, (int)tail);
        const int rc = launch_status();
        if (rc != EWN_OK) return rc;
    }
    for (int level = 2; level <= 2 * T * (S - 1); level++) {     // Phi >= 2: a live position has a cube a side, neither on its corner
        const unsigned long long wg = eg_level(S, K, T, level, L);
        // A level goes out in launches of at most EG_MAX_GRID workgroups.  The runtime takes a grid of 2^24 workgroups of 256 threads
        // or more without an error and runs its thread count modulo 2^32: levels 5 to 16 of (5, 3, 5) have 23 866 975 workgroups, of which
        // one launch ran the first 7 089 759 and left blocks (3, 1), (3, 2) and 43 % of (2, 3) at the cleared 0.  The launches of a
        // level write disjoint entries and read lower levels only, so their order on the stream is all they need.
        for (unsigned long long first = 0; first < wg; first += EG_MAX_GRID) {
            const unsigned long long n = wg - first < EG_MAX_GRID ? wg - first : EG_MAX_GRID;
            L.first = (u32)first;
            k_endgame_level<S><<<dim3((unsigned)n), dim3(EG_NT), 0, s>>>(table, g, L);
            const int rc = launch_status();
            if (rc != EWN_OK) return rc;
        }
    }
    return EWN_OK;
}

template <int S>
static int eg_lookup(int M, const EgGeo &g, const EgLookBuf &B, hipStream_t s)
{
    k_endgame_lookup<S><<<dim3((unsigned)((M - 1) / EG_NT + 1)), dim3(EG_NT), 0, s>>>(M, g, B);
    return launch_status();
}

#define EG_BY_SIZE(S_, CALL)                                                                                          \
    switch (S_) {                                                                                                     \
    case 3: return CALL(3); case 4: return CALL(4); case 5: return CALL(5); case 6: return CALL(6); case 7: return CALL(7);   \
    case 8: return CALL(8); case 9: return CALL(9); case 10: return CALL(10); default: return CALL(11);               \
    }

int64_t ewn_endgame_table_bytes(int board_size, int max_cubes, int max_total)
{
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    EgGeo g;
    return (int64_t)eg_geo(board_size, max_cubes, max_total, g) * (int64_t)sizeof(float);
}

int ewn_endgame_build(int board_size, int max_cubes, int max_total, float *table, int64_t table_bytes, void *stream)
{
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (!table) return EWN_ENULL;
    EgGeo g;
    const long long entries = eg_geo(board_size, max_cubes, max_total, g);
    if (table_bytes != (int64_t)entries * (int64_t)sizeof(float) || ((uintptr_t)table & 3u)) return EWN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define EG_CALL(S_) eg_build<S_>(max_cubes, max_total, table, entries, g, s)
    EG_BY_SIZE(board_size, EG_CALL)
#undef EG_CALL
}

int ewn_endgame_lookup(int board_size, int max_cubes, int max_total, const float *table, int M, const int8_t *boards, const int8_t *dice,
                       int8_t *actions, float *q, float *value, uint8_t *covered, void *stream)
{
    if (M < 0 || !eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (M == 0) return EWN_OK;
    if (!table || !boards || !dice || !actions) return EWN_ENULL;
    if ((uintptr_t)table & 3u) return EWN_EINVAL;
    EgGeo g;
    eg_geo(board_size, max_cubes, max_total, g);
    EgLookBuf B = { table, boards, dice, actions, q, value, covered };
    hipStream_t s = (hipStream_t)stream;
#define EG_CALL(S_) eg_lookup<S_>(M, g, B, s)
    EG_BY_SIZE(board_size, EG_CALL)
#undef EG_CALL
}
