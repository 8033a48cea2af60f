// ewn_puct_wide.hpp -- several leaves of one tree per round under a virtual loss: the marks beside a tree, their
// removal along a parent chain and the wide walk, which is ewn_puct.hpp's pu_walk on n + vn, w - (float)vn and cn + vcn.  The root,
// the evaluation, the backup and the layout are ewn_puct.hpp's, called as they are; ewn_puct_wide.hip is the one user.
//
// A mark on (p, a, d) says that a leaf collected in this round and not yet evaluated lies below edge a of node p under dice d:
// vn[p][a] and vcn[p][a][d - 1] count them.  They are per-edge words: lane a alone reads and writes the marks of edge a, as it does
// the edge's n, w, p, child and cn (ewn_puct.hpp's rule).  A node's marks are zeroed by their own lanes when the node is created
// (pw_clear), which is before any walk enters it, so what the buffer held cannot matter; all are zero again when a search ends.
//
// Within one walk half nothing is read that another lane wrote in the same half: a later walk reads the per-edge words earlier
// walks wrote, boards, dice and parent triples of nodes created in EARLIER rounds only -- a node created in this round is never
// entered, the collision test looks at its index alone -- and the chains that pw_unmark climbs start at such older nodes.
#pragma once
#include "ewn_puct.hpp"

#define PW_MAX_LEAVES 32     // the columns of an MFMA tile
#define PW_NODE_BYTES 96     // a node's marks: vn int32 [6] in one section, vcn int16 [6][6] in the next

// one tree's marks inside the 4-byte aligned scratch: vn int32 [nodes][6] | vcn int16 [nodes][6][6]
struct PwMarks { int *vn; int16_t *vcn; };

EWN_DEV PwMarks pw_marks(uint8_t *scratch, size_t m, int nodes)
{
    uint8_t *s = scratch + m * ((size_t)PW_NODE_BYTES * (size_t)nodes);   // 64-bit byte offsets
    PwMarks V;
    V.vn = (int *)s; V.vcn = (int16_t *)(s + (size_t)24 * (size_t)nodes);
    return V;
}

// node idx has no marks: lane a writes edge a's seven counts
EWN_DEV void pw_clear(const PwMarks &V, int idx, int lane)
{
    if (lane < 6) {
        V.vn[6 * idx + lane] = 0;
        int16_t *c = V.vcn + 36 * idx + 6 * lane;
        #pragma unroll
        for (int i = 0; i < 6; i++) c[i] = 0;
    }
}

// The marks of the path from the root to node j are removed: pu_backup's climb and range checks, lane a takes one off edge a
EWN_DEV void pw_unmark(const PuTree &T, const PwMarks &V, int j, int lane, int nodes)
{
    #pragma unroll 1
    for (int guard = 0; guard < nodes; guard++) {
        const int p = T.parent[4 * j], a = T.parent[4 * j + 1], d = T.parent[4 * j + 2];
        if (p < 0 || p >= j || a < 0 || a > 5 || d < 1 || d > 6) break;   // the root (or a buffer that is no tree)
        if (lane == a) {
            V.vn[6 * p + a] -= 1;
            V.vcn[36 * p + 6 * a + d - 1] -= 1;
        }
        j = p;
    }
}

enum { PW_BEGUN = 0, PW_LEAF = 1, PW_COLLISION = 2 };

// One walk of a round's walk half: pu_walk, operation for operation, on the marked counts.  count0: the tree's nodes when the half
// began.  -> PW_LEAF: a new node, marked down to it, its observation in leaf_row / leaf_dice; PW_BEGUN: the simulation ended on a
// winning edge (backed up at once) or where pu_walk breaks off, its marks removed; PW_COLLISION: the selected child was created in
// this round and is not evaluated yet -- the marks are removed, no simulation has begun and the round collects no further leaf
template <int S>
EWN_DEV int pw_walk(const PuTree &T, const PwMarks &V, int &count, int count0, int nodes, float c_puct, int8_t *leaf_row, int8_t *leaf_dice,
                    int lane, int8_t *base)
{
    constexpr int CELLS = S * S;
    uint8_t *pos = (uint8_t *)(base + PU_O_POS);
    float *sc = (float *)(base + PU_O_OWN);
    int *isc = (int *)(base + PU_O_OWN) + 8;
    int j = 0;
    #pragma unroll 1
    for (int step = 0; step < nodes; step++) {                 // a path holds at most `count` nodes
        int PA, PO;
        __builtin_amdgcn_wave_barrier();                       // what was there is read
        la_observation<S, 64>(T.board + (size_t)j * CELLS, lane, base, pos, PA, PO);
        if (PA == 0 || PO == 0) break;
        const PuEdge E = pu_edge<S>(base, pos, PA, PO, (int)T.dice[j], lane);
        const int vn = lane < 6 ? V.vn[6 * j + lane] : 0;
        const int nn = (lane < 6 ? T.n[6 * j + lane] : 0) + vn;
        const float ww = (lane < 6 ? T.w[6 * j + lane] : 0.0f) - (float)vn, pp = lane < 6 ? T.p[6 * j + lane] : 0.0f;
        if (lane < 8) isc[lane] = nn;
        __builtin_amdgcn_wave_barrier();
        const int Ns = isc[0] + isc[1] + isc[2] + isc[3] + isc[4] + isc[5];
        const float rs = (float)sqrt((double)(Ns + 1));        // the correctly rounded fp32 root of an integer
        const float qa = nn > 0 ? ww / (float)nn : 0.0f;
        const float score = qa + ((c_puct * pp) * rs) / (float)(1 + nn);
        if (lane < 8) sc[lane] = score;
        const u32 valid = (u32)__builtin_amdgcn_ballot_w64(E.kind != 0) & 0x3Fu;
        __builtin_amdgcn_wave_barrier();
        int best = -1;
        float sb = 0.0f;
        #pragma unroll
        for (int i = 0; i < 6; i++) {
            const float si = sc[i];
            if (((valid >> i) & 1u) && (best < 0 || si > sb)) { best = i; sb = si; }
        }
        if (best < 0) break;
        const int bk = __shfl(E.kind, best), bsrc = __shfl(E.src, best), bdst = __shfl(E.dst, best), bcube = __shfl(E.cube, best);
        if (bk == 1) {                                         // the move wins: +1 from this node, no network call
            pw_unmark(T, V, j, lane, nodes);
            if (lane == best) { T.w[6 * j + best] += 1.0f; T.n[6 * j + best] += 1; }
            pu_backup(T, j, 1.0f, lane, nodes);
            return PW_BEGUN;
        }
        int dsel = 1, c = -1;                                  // chance: the least visited dice, the first of them
        if (lane == best) {
            const int16_t *cn = T.cn + 36 * j + 6 * best, *vc = V.vcn + 36 * j + 6 * best;
            int mn = cn[0] + vc[0];
            #pragma unroll
            for (int i = 1; i < 6; i++) { const int x = cn[i] + vc[i]; if (x < mn) { mn = x; dsel = i + 1; } }
            c = T.child[36 * j + 6 * best + dsel - 1];
        }
        dsel = __shfl(dsel, best); c = __shfl(c, best);
        if (c >= 0) {
            if (c >= count || c <= j) break;                   // no tree
            if (c >= count0) {                                 // created in this round: not entered
                pw_unmark(T, V, j, lane, nodes);
                return PW_COLLISION;
            }
        } else if (count >= nodes) break;
        if (lane == best) {                                    // the mark on (j, best, dsel)
            V.vn[6 * j + best] += 1;
            V.vcn[36 * j + 6 * best + dsel - 1] += 1;
        }
        if (c >= 0) { j = c; continue; }
        const int idx = count++;                               // a new node: flip(b1) under dsel, a pending leaf
        if (lane == best) T.child[36 * j + 6 * best + dsel - 1] = (int16_t)idx;
        pw_clear(V, idx, lane);
        if (lane < CELLS) {
            const int rc = CELLS - 1 - lane;
            int v = base[rc];
            v = rc == bsrc ? 0 : v;
            v = rc == bdst ? bcube : v;
            const int8_t nb = (int8_t)(-v);
            T.board[(size_t)idx * CELLS + lane] = nb;
            leaf_row[lane] = nb;
        }
        if (lane == 0) {
            T.dice[idx] = (int8_t)dsel;
            T.parent[4 * idx] = (int16_t)j; T.parent[4 * idx + 1] = (int16_t)best; T.parent[4 * idx + 2] = (int16_t)dsel;
            leaf_dice[0] = (int8_t)dsel;
        }
        return PW_LEAF;
    }
    pw_unmark(T, V, j, lane, nodes);                           // broken off where pu_walk breaks off: begun, and unmarked
    return PW_BEGUN;
}
