// ewn_lookahead.hpp -- what the lookahead units share (ewn_predict_lookahead.hip, ewn_lookahead_stages.hip): the tuple numbering of the
// (agent move, reply) tree and the device helpers that read a root off an observation held in LDS.
#pragma once
#include "ewn_policy_host.hpp"

#define LA_REPLIES 18        // (reply cube 1 .. 6, direction 0 .. 2) per root
#define LA_TUPLES 108        // (root 0 .. 5 = 3 f + r, reply): tuple t = 18 root + 3 (cube - 1) + direction

// find_cube_to_move (envs/ewn.py:178-215) on a presence mask (bit k: cube k is on the board, k = 1 .. 6; P != 0), d = 1 .. 6: the dice's
// cube, else the nearest larger / smaller one as asked for, else the other.  The same for both players: "larger" is the larger number
EWN_DEV int la_find(int larger, int d, int P)
{
    if ((P >> d) & 1) return d;
    const int up = P & ~((2 << d) - 1), dn = P & ((1 << d) - 1);
    const int hi = up ? __builtin_ctz(up) : 0, lo = dn ? 31 - __builtin_clz(dn) : 0;
    return larger ? (hi ? hi : lo) : (lo ? lo : hi);
}

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
