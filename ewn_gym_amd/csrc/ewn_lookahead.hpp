// ewn_lookahead.hpp -- the one copy of what the units on the (agent move, reply) tree share (ewn_predict_lookahead.hip,
// ewn_lookahead_stages.hip, ewn_puct.hip; ewn_endgame.hip takes la_dice and la_find): the tuple numbering, the observation loaded into
// LDS, a root read off it, and the fold of W per tuple into R, Q and the action.
#pragma once
#include "ewn_policy_host.hpp"

#define LA_REPLIES 18        // (reply cube 1 .. 6, direction 0 .. 2) per root
#define LA_TUPLES 108        // (root 0 .. 5 = 3 f + r, reply): tuple t = 18 root + 3 (cube - 1) + direction

// the dice as every unit reads it: outside 1 .. 6 it is clamped
EWN_DEV int la_dice(int d) { return d < 1 ? 1 : d > 6 ? 6 : d; }

// find_cube_to_move (envs/ewn.py:178-215) on a presence mask (bit k: cube k is on the board, k = 1 .. 6; P != 0), d = 1 .. 6: the dice's
// cube, else the nearest larger / smaller one as asked for, else the other.  The same for both players: "larger" is the larger number
EWN_DEV int la_find(int larger, int d, int P)
{
    if ((P >> d) & 1) return d;
    const int up = P & ~((2 << d) - 1), dn = P & ((1 << d) - 1);
    const int hi = up ? __builtin_ctz(up) : 0, lo = dn ? 31 - __builtin_clz(dn) : 0;
    return larger ? (hi ? hi : lo) : (lo ? lo : hi);
}

// An observation into LDS: the board at `row` -> base, zero past the board; the cell of agent cube k -> pos[k], of opposing cube k ->
// pos[8 + k], 0xFF for a cube that is gone; PA / PO the presence masks (all wave-uniform).  Returns whether the row is searched: not
// already over (check_win) and a cube on either side.  EXTENT is how many bytes of base there are to write: the stage and PUCT
// kernels keep 64, a byte per lane, but k_predict_lookahead's base is a leaf slot of RecGeo<S>::STR bytes (32 at 5x5) with pos
// directly behind it, so a lane past EXTENT must not store
template <int S, int EXTENT>
EWN_DEV bool la_observation(const int8_t *row, int lane, int8_t *base, uint8_t *pos, int &PA, int &PO)
{
    constexpr int CELLS = S * S;
    static_assert(CELLS <= EXTENT && EXTENT <= 64, "one lane per cell, and no store past base");
    const int cell = lane < CELLS ? (int)row[lane] : 0;
    if (EXTENT == 64 || lane < EXTENT) base[lane] = (int8_t)cell;
    if (lane < 16) pos[lane] = 0xFFu;
    __builtin_amdgcn_wave_barrier();
    if (cell != 0 && cell >= -6 && cell <= 6) pos[cell > 0 ? cell : 8 - cell] = (uint8_t)lane;
    __builtin_amdgcn_wave_barrier();
    const u32 have = (u32)__builtin_amdgcn_ballot_w64(lane < 16 && pos[lane & 15] != 0xFFu);
    PA = (int)(have & 0x7Eu); PO = (int)((have >> 8) & 0x7Eu);
    return !(PA == 0 || PO == 0 || base[0] < 0 || base[CELLS - 1] > 0);
}

// a row that is not searched: action (0, 0), every Q -inf
EWN_DEV void la_row_over(int8_t *actions, float *q, size_t m, int lane)
{
    if (lane < 2) actions[m * 2 + lane] = 0;
    if (q && lane < 6) q[m * 6 + lane] = -__builtin_inff();
    __builtin_amdgcn_wave_barrier();                           // base and pos are read: the next trip may overwrite them
}

// the root that is searched for `root`: both flags name one cube (c1 == c0) unless the dice's cube is gone, and roots 3 .. 5 are then roots 0 .. 2
EWN_DEV int la_searched(int root, int c0, int c1) { return root >= 3 && c1 == c0 ? root - 3 : root; }

// the agent's move of root `root` (= 3 f + r): code 0 it leaves the board, 1 it wins, 2 it is searched
struct LaRoot { int code, cube, src, dst, PA1, PO1; };     // PA1 / PO1: the presence masks of b1

template <int S>
EWN_DEV LaRoot la_root(const int8_t *base, const uint8_t *pos, int PA, int PO, int c0, int c1, int root)
{
    const int f = root >= 3, r = root - 3 * f;
    LaRoot o;
    o.cube = f ? c1 : c0;
    o.src = pos[o.cube];
    const int x = o.src / S, y = o.src % S;
    const bool on = (r == 1 || y < S - 1) && (r == 0 || x < S - 1);
    o.dst = on ? o.src + (r == 0 ? 1 : r == 1 ? S : S + 1) : o.src;
    const int v0 = base[o.dst];                                // what the move captures, own cubes included (envs/ewn.py:252-260)
    o.PA1 = PA & ~(v0 > 0 ? 1 << (v0 & 7) : 0);
    o.PO1 = PO & ~(v0 < 0 ? 1 << (-v0 & 7) : 0);
    o.code = !on ? 0 : (o.dst == S * S - 1 || o.PO1 == 0) ? 1 : 2;
    return o;
}

// The fold of a searched row, W(reply) per tuple in Wt (+inf where there is none; written, and a wave barrier passed): R per (root,
// d1) into Rt [36], Q per root into Qt [6] and q, the first maximum of Q (strict >, as pol_pick_*) into actions.  Sums in dice order
template <int S>
EWN_DEV void la_fold(const int8_t *base, const uint8_t *pos, int PA, int PO, int c0, int c1, const float *Wt, float *Rt, float *Qt, float tv,
                     int8_t *actions, float *q, size_t m, int lane)
{
    // R per (root, d1): the minimum over the replies of the (at most two) cubes d1 selects; a non-terminal b1 always has a reply
    if (lane < 36) {
        const int root = la_searched(lane / 6, c0, c1), d1 = lane % 6 + 1;
        const LaRoot R = la_root<S>(base, pos, PA, PO, c0, c1, root);
        float r = 0.0f;
        if (R.code == 2) {
            const float *wa = Wt + root * LA_REPLIES + 3 * (la_find(0, d1, R.PO1) - 1), *wb = Wt + root * LA_REPLIES + 3 * (la_find(1, d1, R.PO1) - 1);
            r = wa[0];
            r = wa[1] < r ? wa[1] : r; r = wa[2] < r ? wa[2] : r;
            r = wb[0] < r ? wb[0] : r; r = wb[1] < r ? wb[1] : r; r = wb[2] < r ? wb[2] : r;
        }
        Rt[lane] = r;
    }
    __builtin_amdgcn_wave_barrier();
    // Q per root: the mean over d1, in d1 order
    if (lane < 6) {
        const int root = la_searched(lane, c0, c1);
        const LaRoot R = la_root<S>(base, pos, PA, PO, c0, c1, root);
        const float *r = Rt + 6 * lane;
        float qv = (((((r[0] + r[1]) + r[2]) + r[3]) + r[4]) + r[5]) * (1.0f / 6.0f);
        qv = R.code == 0 ? -__builtin_inff() : R.code == 1 ? tv : qv;
        Qt[lane] = qv;
        if (q) q[m * 6 + lane] = qv;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        int best = 0;
        float qb = Qt[0];
        #pragma unroll
        for (int i = 1; i < 6; i++) { const float qi = Qt[i]; if (qi > qb) { qb = qi; best = i; } }
        actions[m * 2] = (int8_t)(best / 3); actions[m * 2 + 1] = (int8_t)(best % 3);
    }
    __builtin_amdgcn_wave_barrier();                           // this trip's LDS is read: the next may overwrite it
}

// the grid of a kernel that walks M rows grid-stride, per_block of them per block and trip (M >= 1)
static inline unsigned la_blocks(int M, int per_block, int max_blocks)
{
    const int need = (M - 1) / per_block + 1;
    return (unsigned)(need < max_blocks ? need : max_blocks);
}
