// ewn_endgame.hpp -- the one copy of how an endgame table (layout version 1, ewn_endgame.hip's header comment) is indexed, for the
// units that read one: ewn_endgame.hip (the build and the lookup), ewn_predict_lookahead.hip (covered leaves),
// ewn_playout_search.hip (covered leaves of the playout tree search), ewn_puct_fused.hip (covered leaves of the
// one-launch PUCT search) and ewn_puct_games.hip (the same leaves in whole self-play games).
#pragma once
#include "ewn_lookahead.hpp"

struct EgMasks { uint8_t rank[64]; uint8_t unrank[4][20]; };   // rank[mask of cubes 1..6 >> 1]; unrank[popcount][rank]
static constexpr EgMasks eg_make_masks()
{
    EgMasks t{};
    int cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int m = 0; m < 64; m++) {
        const int k = __builtin_popcount((unsigned)m);
        t.rank[m] = (uint8_t)cnt[k];
        if (k <= 3) t.unrank[k][cnt[k]] = (uint8_t)m;
        cnt[k]++;
    }
    return t;
}
// a copy per unit that includes this: internal, except in ewn_endgame.hip, whose symbol keeps the name and linkage it had there
#ifndef EG_MASKS_LINKAGE
#define EG_MASKS_LINKAGE static
#endif
EG_MASKS_LINKAGE __constant__ EgMasks EG_MASKS = eg_make_masks();

// EG_MASKS.rank without the load, for masks of at most three cubes (K <= 3): the combinatorial number system -- the i-th lowest set
// bit at position p (cube p + 1) adds binom(p, i), which ranks the masks of one popcount in ascending order
static constexpr u32 eg_rank(int M)
{
    u32 r = 0;
    int i = 1;
    for (int m = (M >> 1) & 63; m; m &= m - 1, i++) {
        const u32 p = (u32)__builtin_ctz((unsigned)m);
        r += i == 1 ? p : i == 2 ? p * (p - 1) / 2 : p * (p - 1) * (p - 2) / 6;
    }
    return r;
}
static constexpr bool eg_rank_is_the_table()
{
    const EgMasks t = eg_make_masks();
    for (int m = 0; m < 64; m++)
        if (__builtin_popcount((unsigned)m) <= 3 && eg_rank(m << 1) != t.rank[m]) return false;
    return true;
}
static_assert(eg_rank_is_the_table(), "eg_rank is EG_MASKS.rank on every mask of at most three cubes");

struct EgGeo { int K, T; long long off[4][4]; };             // off[ka][ko]: the block's first entry (in floats); -1: not in the table

template <int S> struct EgDim {
    static constexpr int C = S * S;
    static constexpr u32 pw(int k) { return k == 0 ? 1u : k == 1 ? (u32)C : k == 2 ? (u32)C * C : (u32)C * C * C; }
    static constexpr u32 n(int k) { return (k == 1 ? 6u : k == 2 ? 15u : 20u) * pw(k); }
};
template <int S> EWN_DEV u32 eg_pw(int k) { return k == 1 ? EgDim<S>::pw(1) : k == 2 ? EgDim<S>::pw(2) : EgDim<S>::pw(3); }
template <int S> EWN_DEV u32 eg_n(int k) { return k == 1 ? EgDim<S>::n(1) : k == 2 ? EgDim<S>::n(2) : EgDim<S>::n(3); }

// eg_geo's off[ka][ko] of the (S, K, T) table for a lane's own counts (the block must be in the table) without a load: the block rows
// above it (row a holds the blocks ko = 1 .. min(K, T - a)), then the blocks to its left.  Indexing EgGeo.off with a lane's counts is
// a load from the kernel's arguments, and selects among its nine entries are turned back into one by the compiler
template <int S>
static constexpr long long eg_off(int K, int T, int ka, int ko)
{
    constexpr u32 N1 = EgDim<S>::n(1), N2 = N1 + EgDim<S>::n(2), N3 = N2 + EgDim<S>::n(3);   // the entries of 1 .. k opposing cubes
    const auto row = [&](int a) { const int w = T - a < K ? T - a : K; return w <= 0 ? 0u : w == 1 ? N1 : w == 2 ? N2 : N3; };   // of block row a
    const long long r1 = (long long)EgDim<S>::n(1) * row(1), r2 = (long long)EgDim<S>::n(2) * row(2);                         // uniform
    const u32 n = ka == 1 ? EgDim<S>::n(1) : ka == 2 ? EgDim<S>::n(2) : EgDim<S>::n(3), left = ko == 1 ? 0u : ko == 2 ? N1 : N2;
    return (ka > 1 ? r1 : 0ll) + (ka > 2 ? r2 : 0ll) + (long long)n * (long long)left;
}
template <int S>
static constexpr bool eg_off_is_eg_geo()                        // against eg_geo's running total, every table and every block of it
{
    for (int K = 1; K <= 3; K++)
        for (int T = 2; T <= 2 * K; T++) {
            long long total = 0;
            for (int a = 1; a <= K; a++)
                for (int o = 1; o <= K; o++)
                    if (a + o <= T) {
                        if (eg_off<S>(K, T, a, o) != total) return false;
                        total += (long long)EgDim<S>::n(a) * (long long)EgDim<S>::n(o);
                    }
        }
    return true;
}
static_assert(eg_off_is_eg_geo<5>() && eg_off_is_eg_geo<7>() && eg_off_is_eg_geo<11>(), "eg_off is eg_geo's off on every block");

// a side as registers: M the presence mask (bit k: cube k, k = 1 .. 6), pos the cell of cube k in byte k - 1 (read only where M has k)
EWN_DEV int eg_cell(u64 pos, int k) { return (int)((pos >> (8 * (k - 1))) & 0xFFull); }

// the side's index from its mask's rank; turned: as flip() shows it to the other side (cell c -> C - 1 - c)
template <int S>
EWN_DEV u32 eg_side_of(u32 rank, int M, u64 pos, bool turned)
{
    constexpr int C = S * S;
    u32 v = rank;
    for (int m = M; m; m &= m - 1) {
        const int c = eg_cell(pos, __builtin_ctz(m));
        v = v * (u32)C + (u32)(turned ? C - 1 - c : c);
    }
    return v;
}
template <int S> EWN_DEV u32 eg_side(int M, u64 pos, bool turned) { return eg_side_of<S>(EG_MASKS.rank[(M >> 1) & 63], M, pos, turned); }

// A board row of C cells (global memory or LDS) as a table position, and whether the (S, K, T) table covers it: cell values within
// -6 .. 6, no cube number twice on a side (that is not a position), no agent cube on C - 1, no opposing cube on 0, 1 .. K cubes a
// side and at most T in all.  The one copy of the test: k_endgame_lookup's `covered` and the searches that value covered leaves
// (k_playout_search<S, true>) call it, so they agree on every board, malformed ones included.  Ma, Mo, pa, po: the sides as
// registers (above); na, no: the cubes counted, a repeated number counted twice
template <int S>
EWN_DEV bool eg_position(const int8_t *b, int K, int T, int &Ma, int &Mo, int &na, int &no, u64 &pa, u64 &po)
{
    constexpr int C = S * S;
    Ma = 0; Mo = 0; na = 0; no = 0; pa = 0; po = 0;
    bool ok = true;
    #pragma unroll 1
    for (int x = 0; x < S; x++) {
        int v[S];                                                  // a board row at a time: S independent loads, so the latency of
        #pragma unroll                                             // the memory (LDS or global) is paid once a row and not once a cell
        for (int y = 0; y < S; y++) v[y] = b[x * S + y];
        #pragma unroll
        for (int y = 0; y < S; y++) {
            const int c = x * S + y, k = v[y] > 0 ? v[y] : -v[y];
            if (k == 0) continue;
            if (k > 6) { ok = false; continue; }
            // the two sides by selects, not by two branches over one body: the compiler merges such branches into one that indexes
            // the sides' registers as an array in scratch memory
            const bool own = v[y] > 0;
            const int bit = 1 << k;
            const u64 at = (u64)c << (8 * (k - 1));
            ok = ok && !((own ? Ma : Mo) & bit) && c != (own ? C - 1 : 0);
            Ma |= own ? bit : 0; Mo |= own ? 0 : bit;
            na += own ? 1 : 0; no += own ? 0 : 1;
            pa |= own ? at : 0ull; po |= own ? 0ull : at;
        }
    }
    return ok && na >= 1 && no >= 1 && na <= K && no <= K && na + no <= T;
}

// G of the agent's cube `cube` (in Ma) in direction r; -inf where the move leaves the board.  Every index it forms is inside the table:
// a move never adds a cube and never empties the mover's side, so 1 <= popcounts <= K, their sum <= T, and each side index < n_k.
template <int S>
EWN_DEV float eg_move(const float *tbl, const EgGeo &g, int Ma, int Mo, u64 pa, u64 po, int cube, int r)
{
    constexpr int C = S * S;
    const int src = eg_cell(pa, cube), x = src / S, y = src % S;
    if (!((r == 1 || y < S - 1) && (r == 0 || x < S - 1))) return -__builtin_inff();
    const int dst = src + (r == 0 ? 1 : r == 1 ? S : S + 1);
    int Ma1 = Ma, Mo1 = Mo;
    #pragma unroll
    for (int k = 1; k <= 6; k++) {
        if (((Ma >> k) & 1) && eg_cell(pa, k) == dst) Ma1 &= ~(1 << k);
        if (((Mo >> k) & 1) && eg_cell(po, k) == dst) Mo1 &= ~(1 << k);
    }
    if (dst == C - 1 || Mo1 == 0) return 1.0f;
    const int sh = 8 * (cube - 1);
    const u64 pa1 = (pa & ~(0xFFull << sh)) | ((u64)dst << sh);
    const int ka1 = __builtin_popcount((unsigned)Mo1), ko1 = __builtin_popcount((unsigned)Ma1);   // of flip(b1): the sides swap
    const long long idx = g.off[ka1][ko1] + (long long)eg_side<S>(Mo1, po, true) * (long long)eg_n<S>(ko1) + (long long)eg_side<S>(Ma1, pa1, true);
    return -tbl[idx];
}

// ---------------------------------------------------------------- host
static inline bool eg_params_ok(int S, int K, int T) { return S >= 3 && S <= 11 && K >= 1 && K <= 3 && T >= 2 && T <= 2 * K; }

static inline long long eg_n_host(int S, int k)
{
    long long n = k == 1 ? 6 : k == 2 ? 15 : 20;
    for (int i = 0; i < k; i++) n *= S * S;
    return n;
}

// the block offsets, ka-major; returns the table's entries
static inline long long eg_geo(int S, int K, int T, EgGeo &g)
{
    g.K = K; g.T = T;
    long long total = 0;
    for (int a = 0; a < 4; a++) for (int o = 0; o < 4; o++) g.off[a][o] = -1;
    for (int a = 1; a <= K; a++)
        for (int o = 1; o <= K; o++)
            if (a + o <= T) { g.off[a][o] = total; total += eg_n_host(S, a) * eg_n_host(S, o); }
    return total;
}
