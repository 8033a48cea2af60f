// ewn_puct.hpp -- the one copy of the PUCT tree's device code: the layout, a node's edges, the backup, the
// root written by begin, the evaluation of a pending node, one simulation's walk and the move of a self-play game (pu_play).
// ewn_puct.hip (the staged kernels: the network's outputs come and the leaf rows go through global memory, a launch per step),
// ewn_puct_fused.hip (the whole search in one launch: both come and go through LDS) and ewn_puct_games.hip (whole games in one
// launch: that search with the move and a game loop round it) call the same functions, so the paths agree byte for byte by construction.
//
// A wave per tree.  Per-edge state (N, W, P, kind, child[.][d'], cn[.][d']) of edge a is read and written by lane a alone, in every
// kernel.  What one lane writes and ANOTHER reads through global memory -- a node's dice and parent triple and the header (lane 0
// writes, every lane reads), begin's fill (any lane writes a word that another lane's root or edge lies in) -- is handed over in one
// of two ways, and a kernel that calls these functions must provide one of them:
//   staged:  the write and the read are in different launches (boards, dice and parent triples are written one launch before they
//            are read);
//   fused:   a tree stays on ONE wave from the fill to the end of the search, and between the write and the read lies a block
//            barrier (__syncthreads: a workgroup-scope release / acquire), the barriers of the round structure.  Whole games: the
//            same, with the board, dice and game state that pu_play writes for the next ply's pu_root among the values handed over.
// Within one call of pu_round nothing is read that another lane wrote in the same call: a board cell is read by the lane that wrote
// it, the nodes of a backup chain and of a walk were created in earlier rounds, and the node created now is not entered again.
// The node's board goes to LDS by ewn_lookahead.hpp's la_observation, so that la_find and la_root apply unchanged.
#pragma once
#include "ewn_lookahead.hpp"
#include <climits>

#define PU_MAX_SIMS 4096
#define PU_LAYOUT 1          // hdr[5]: the version of the layout below (ewn_gym_amd.vec_env.PUCT_LAYOUT)

// per wave: the node's board (64 bytes, zero past the board) | cube positions [16] | 16 words of the kernel's own
#define PU_O_POS 64
#define PU_O_OWN 80
#define PU_WAVE (PU_O_OWN + 16 * 4)
#define PU_SUM_MIN 0x1p-60f   // pu_evaluate: below this sum of the legal softmax products the priors are formed relative to the legal edges

// One tree, sections of structure-of-arrays inside one 4-byte aligned buffer; `nodes` = sims + 1.  Offsets in bytes:
//   hdr    int32 [8]            node count | simulations begun | pending node (-1: none) | degenerate | sims | PU_LAYOUT | 0 | 0
//   n      int32 [nodes][6]     visits per edge a = 3 f + r
//   w      float [nodes][6]     sum of the values backed up through the edge
//   p      float [nodes][6]     prior
//   child  int16 [nodes][6][6]  the node under (edge, dice d' - 1), -1 for none
//   cn     int16 [nodes][6][6]  its visits
//   parent int16 [nodes][4]     node, edge, dice d', 0; the root: -1, 0, 0, 0
//   kind   int8  [nodes][6]     0 not an action | 1 wins | 2 searched (written when the node is evaluated)
//   dice   int8  [nodes]
//   board  int8  [nodes][S*S]   seen from the node's side to move
// kind, dice and board are each padded to a multiple of 4 bytes.
struct PuLayout { int nodes; u32 n, w, p, child, cn, parent, kind, dice, board; long long bytes; };

__host__ __device__ static inline PuLayout pu_layout(int S, int sims)
{
    PuLayout L;
    const u32 N = (u32)sims + 1u, C = (u32)(S * S);
    u32 o = 32;
    L.nodes = (int)N;
    L.n = o; o += 24 * N;
    L.w = o; o += 24 * N;
    L.p = o; o += 24 * N;
    L.child = o; o += 72 * N;
    L.cn = o; o += 72 * N;
    L.parent = o; o += 8 * N;
    L.kind = o; o += (6 * N + 3) & ~3u;
    L.dice = o; o += (N + 3) & ~3u;
    L.board = o; o += (N * C + 3) & ~3u;
    L.bytes = (long long)o;
    return L;
}

struct PuTree { int *hdr; int *n; float *w; float *p; int16_t *child, *cn, *parent; int8_t *kind, *dice, *board; };

EWN_DEV PuTree pu_tree(uint8_t *trees, size_t m, const PuLayout &L)
{
    uint8_t *t = trees + m * (size_t)L.bytes;                  // 64-bit byte offsets
    PuTree T;
    T.hdr = (int *)t; T.n = (int *)(t + L.n); T.w = (float *)(t + L.w); T.p = (float *)(t + L.p);
    T.child = (int16_t *)(t + L.child); T.cn = (int16_t *)(t + L.cn); T.parent = (int16_t *)(t + L.parent);
    T.kind = (int8_t *)(t + L.kind); T.dice = (int8_t *)(t + L.dice); T.board = (int8_t *)(t + L.board);
    return T;
}

// lane a's edge of the node in LDS under dice d: kind and the move (lanes 6 .. 63: kind 0)
struct PuEdge { int kind, src, dst, cube; bool one; };         // one: both flags name one cube

template <int S>
EWN_DEV PuEdge pu_edge(const int8_t *base, const uint8_t *pos, int PA, int PO, int d, int lane)
{
    const int c0 = la_find(0, d, PA), c1 = la_find(1, d, PA);
    const LaRoot R = la_root<S>(base, pos, PA, PO, c0, c1, lane < 6 ? lane : 0);
    PuEdge E;
    E.one = c1 == c0;
    E.kind = lane >= 6 || (lane >= 3 && E.one) ? 0 : R.code;
    E.src = R.src; E.dst = R.dst; E.cube = R.cube;
    return E;
}

// Backup of v from node j: every lane walks the parent chain, lane a adds to edge a
EWN_DEV void pu_backup(const PuTree &T, int j, float v, int lane, int nodes)
{
    #pragma unroll 1
    for (int guard = 0; guard < nodes; guard++) {
        const int p = T.parent[4 * j], a = T.parent[4 * j + 1], d = T.parent[4 * j + 2];
        if (p < 0 || p >= j || a < 0 || a > 5 || d < 1 || d > 6) break;   // the root (or a buffer that is no tree)
        v = -v;
        if (lane == a) {
            T.w[6 * p + a] += v;
            T.n[6 * p + a] += 1;
            T.cn[36 * p + 6 * a + d - 1] += 1;
        }
        j = p;
    }
}

// The root of a tree whose every byte is filled (zeros, child -1), by one wave: the header, node 0 and the leaf row -- the root's
// observation, or a zero board with dice 1 where the observation is over or a side has no cube (a degenerate tree).  `lds` is the
// wave's PU_WAVE bytes; leaf_row [CELLS] and leaf_dice [1] may lie in global memory or in LDS
template <int S>
EWN_DEV void pu_root(const PuTree &T, const int8_t *row, const int8_t *dice, int sims, int8_t *leaf_row, int8_t *leaf_dice, int lane, int8_t *lds)
{
    constexpr int CELLS = S * S;
    uint8_t *pos = (uint8_t *)(lds + PU_O_POS);
    int PA, PO;
    __builtin_amdgcn_wave_barrier();                           // what was there is read
    const bool live = la_observation<S, 64>(row, lane, lds, pos, PA, PO);
    const int d = la_dice((int)dice[0]);
    if (lane < CELLS) {
        T.board[lane] = lds[lane];
        leaf_row[lane] = live ? lds[lane] : (int8_t)0;
    }
    if (lane == 0) {
        T.hdr[0] = 1; T.hdr[1] = 0; T.hdr[2] = live ? 0 : -1; T.hdr[3] = live ? 0 : 1; T.hdr[4] = sims; T.hdr[5] = PU_LAYOUT;
        T.dice[0] = (int8_t)d;
        T.parent[0] = -1;
        leaf_dice[0] = (int8_t)(live ? d : 1);
    }
}

// the noise instance's own (ewn_puct_advance_noise): the tree's six weights, eps and keep = 1 - eps formed once on the host
struct PuNoise { const float *row; float eps, keep; };

// The evaluation of the pending node: priors from the five logits at lg (softmax over the flags times softmax over the directions,
// normalised over the legal edges), kind, then the backup of v = *vp * inv_tv clamped to [-1, 1].  Both softmaxes are taken relative
// to the maximum of ALL their entries, so a network that puts its mass on illegal moves leaves the legal products, and their sum,
// in the denormals or at zero.  Where the sum is below PU_SUM_MIN (wave-uniform: every lane reads the same six words) the same
// priors are formed again relative to the legal edges alone: b the first legal edge of the largest logit sum, e_a = expf of the
// DIFFERENCES (l_f[a] - l_f[b]) + (l_r[a] - l_r[b]) (the direction term alone where both flags name one cube), P_a = e_a / sum e.
// e_b is 1, so that sum lies in [1, 6]; the differences are taken before anything is added, so an offset common to all logits
// cancels exactly.  At and above PU_SUM_MIN the arithmetic is the product's, bit for bit as it always was: an edge whose product has
// left the normal numbers (below 2^-126) has a prior below 2^-126 / PU_SUM_MIN = 2^-66, far inside the priors' tolerance of 2^-19
// (DESIGN.md 4o).  Finite logits and a value that is not a NaN are the contract.  NOISE: when the node is the root,
// its priors are mixed with the caller's weights, normalised over the legal edges, before the backup and before the first
// simulation selects on them.  lg and vp may lie in global memory or in LDS
template <int S, bool NOISE>
EWN_DEV void pu_evaluate(const PuTree &T, int pending, const float *lg, const float *vp, float inv_tv, const PuNoise &Z, int nodes, int lane,
                         int8_t *base)
{
    constexpr int CELLS = S * S;
    uint8_t *pos = (uint8_t *)(base + PU_O_POS);
    float *sc = (float *)(base + PU_O_OWN);
    int PA, PO;
    __builtin_amdgcn_wave_barrier();                           // what was there is read
    la_observation<S, 64>(T.board + (size_t)pending * CELLS, lane, base, pos, PA, PO);
    if (PA != 0 && PO != 0) {
        const PuEdge E = pu_edge<S>(base, pos, PA, PO, (int)T.dice[pending], lane);
        const float l0 = lg[0], l1 = lg[1], l2 = lg[2], l3 = lg[3], l4 = lg[4];
        const float mf = l1 > l0 ? l1 : l0;
        const float f0 = expf(l0 - mf), f1 = expf(l1 - mf), sf = f0 + f1;
        float mr = l3 > l2 ? l3 : l2;
        mr = l4 > mr ? l4 : mr;
        const float r0 = expf(l2 - mr), r1 = expf(l3 - mr), r2 = expf(l4 - mr), sr = (r0 + r1) + r2;
        const int f = lane >= 3, r = lane - 3 * f;
        const float pf = (f ? f1 : f0) / sf, pr = (r == 0 ? r0 : r == 1 ? r1 : r2) / sr;
        float raw = E.kind == 0 ? 0.0f : E.one ? pr : pf * pr;
        if (lane < 8) sc[lane] = raw;
        __builtin_amdgcn_wave_barrier();
        float sum = ((((sc[0] + sc[1]) + sc[2]) + sc[3]) + sc[4]) + sc[5];
        if (!(sum >= PU_SUM_MIN)) {                            // the legal products ran out of fp32: relative to the legal edges
            const u32 legal = (u32)__builtin_amdgcn_ballot_w64(E.kind != 0) & 0x3Fu;
            int b = -1;
            float tb = 0.0f;
            #pragma unroll
            for (int i = 0; i < 6; i++) {
                const float tf = i >= 3 ? l1 - mf : l0 - mf, tr = (i % 3 == 0 ? l2 : i % 3 == 1 ? l3 : l4) - mr;
                const float ti = E.one ? tr : tf + tr;
                if (((legal >> i) & 1u) && (b < 0 || ti > tb)) { b = i; tb = ti; }
            }
            if (b >= 0) {
                const float lfb = b >= 3 ? l1 : l0, lrb = b % 3 == 0 ? l2 : b % 3 == 1 ? l3 : l4;
                const float lf = f ? l1 : l0, lr = r == 0 ? l2 : r == 1 ? l3 : l4;
                const float df = lf - lfb, dr = lr - lrb;
                raw = E.kind == 0 ? 0.0f : expf(E.one ? dr : df + dr);
                __builtin_amdgcn_wave_barrier();               // the products are read
                if (lane < 8) sc[lane] = raw;
                __builtin_amdgcn_wave_barrier();
                sum = ((((sc[0] + sc[1]) + sc[2]) + sc[3]) + sc[4]) + sc[5];
            }
        }
        if constexpr (NOISE) {
            float prior = E.kind == 0 ? 0.0f : raw / sum;
            if (pending == 0) {
                float eta = 0.0f;
                if (lane < 6 && E.kind != 0) {
                    const float x = Z.row[lane];
                    eta = x > 0.0f && x < __builtin_inff() ? x : 0.0f;   // NaN, inf, zero and negative numbers: no weight
                }
                __builtin_amdgcn_wave_barrier();               // the raw priors are read
                if (lane < 8) sc[lane] = eta;
                __builtin_amdgcn_wave_barrier();
                const float es = ((((sc[0] + sc[1]) + sc[2]) + sc[3]) + sc[4]) + sc[5];
                if (es > 0.0f && E.kind != 0) prior = Z.keep * prior + Z.eps * (eta / es);
            }
            if (lane < 6) {
                T.kind[6 * pending + lane] = (int8_t)E.kind;
                T.p[6 * pending + lane] = prior;
            }
        } else if (lane < 6) {
            T.kind[6 * pending + lane] = (int8_t)E.kind;
            T.p[6 * pending + lane] = E.kind == 0 ? 0.0f : raw / sum;
        }
        float v = vp[0] * inv_tv;
        v = v > -1.0f ? v : -1.0f;
        v = v < 1.0f ? v : 1.0f;
        pu_backup(T, pending, v, lane, nodes);
    }
}

// One simulation from the root: down to a new node, which becomes the pending leaf (its observation goes to leaf_row / leaf_dice,
// global memory or LDS; returns true), or to a winning edge, which is backed up at once.  count: the tree's nodes, one more with a leaf
template <int S>
EWN_DEV bool pu_walk(const PuTree &T, int &count, int &pending, int nodes, float c_puct, int8_t *leaf_row, int8_t *leaf_dice, int lane,
                     int8_t *base)
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
        const int nn = lane < 6 ? T.n[6 * j + lane] : 0;
        const float ww = lane < 6 ? T.w[6 * j + lane] : 0.0f, pp = lane < 6 ? T.p[6 * j + lane] : 0.0f;
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
            if (lane == best) { T.w[6 * j + best] += 1.0f; T.n[6 * j + best] += 1; }
            pu_backup(T, j, 1.0f, lane, nodes);
            break;
        }
        int dsel = 1, c = -1;                                  // chance: the least visited dice, the first of them
        if (lane == best) {
            const int16_t *cn = T.cn + 36 * j + 6 * best;
            int mn = cn[0];
            #pragma unroll
            for (int i = 1; i < 6; i++) { const int x = cn[i]; if (x < mn) { mn = x; dsel = i + 1; } }
            c = T.child[36 * j + 6 * best + dsel - 1];
        }
        dsel = __shfl(dsel, best); c = __shfl(c, best);
        if (c >= 0) {
            if (c >= count || c <= j) break;                   // no tree
            j = c;
            continue;
        }
        if (count >= nodes) break;
        const int idx = count++;                               // a new node: flip(b1) under dsel, the pending leaf
        if (lane == best) T.child[36 * j + 6 * best + dsel - 1] = (int16_t)idx;
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
        pending = idx;
        return true;
    }
    return false;
}

// One round of one tree, by one wave (ewn_puct_advance's definition): the pending node is evaluated and backed up; while fewer than
// `sims` simulations have begun, one more walks down; the header; the leaf row of a tree without a new leaf is a zero board with
// dice 1.  A tree of another budget or layout, or no tree at all, is left alone.  base: the wave's PU_WAVE bytes of LDS
template <int S, bool NOISE>
EWN_DEV void pu_round(const PuTree &T, int sims, float c_puct, float inv_tv, int nodes, const float *lg, const float *vp, const PuNoise &Z,
                      int8_t *leaf_row, int8_t *leaf_dice, int lane, int8_t *base)
{
    constexpr int CELLS = S * S;
    int count = T.hdr[0], done = T.hdr[1], pending = T.hdr[2];
    const bool ok = T.hdr[3] == 0 && T.hdr[4] == sims && T.hdr[5] == PU_LAYOUT && count >= 1 && count <= nodes && pending < count;
    bool leaf = false;                                         // a new node's observation went to the leaf row
    if (ok) {
        if (pending >= 0) {                                    // ---- evaluation: priors from the logits, then backup of v
            pu_evaluate<S, NOISE>(T, pending, lg, vp, inv_tv, Z, nodes, lane, base);
            pending = -1;
        }
        if (done < sims) {                                     // ---- one simulation: down to a new node or a winning edge
            done++;
            leaf = pu_walk<S>(T, count, pending, nodes, c_puct, leaf_row, leaf_dice, lane, base);
        }
        if (lane == 0) { T.hdr[0] = count; T.hdr[1] = done; T.hdr[2] = pending; }
    }
    if (!leaf) {
        if (lane < CELLS) leaf_row[lane] = 0;
        if (lane == 0) leaf_dice[0] = 1;
    }
    __builtin_amdgcn_wave_barrier();                           // this trip's LDS is read: the next may overwrite it
}

// the record buffers of ewn_puct_play: rows of board [CELLS], dice, visits [6], value, action [2], live; each pointer may be NULL
struct PuRecord { int8_t *board; int8_t *dice; int *visits; float *value; int8_t *action; int8_t *live; };

// The move of one self-play game off its finished tree, by one wave (ewn_puct_play's definition): the position played
// is the tree's root.  The edge is the first winning one, else drawn in proportion to the root's visits while ply < temp_plies
// (integer arithmetic on a Philox word of ply and gid), else k_puct_result's first maximum; the record row, the board after the move
// seen from the other side (board [CELLS]), the next dice (dice [1], a second Philox word) and the game's state g = {ply, over,
// winner, 0} are written; the record row is row r of R's buffers.  known: the budget is one a tree can have; T is only read.  Returns whether the game goes on.
// base: the wave's PU_WAVE bytes of LDS
template <int S>
EWN_DEV bool pu_play(const PuTree &T, bool known, int sims, int nodes, int8_t *board, int8_t *dice, int *g, int temp_plies, u32 k0, u32 k1,
                     unsigned long long gid, const PuRecord &R, size_t r, int lane, int8_t *base)
{
    constexpr int CELLS = S * S;
    uint8_t *pos = (uint8_t *)(base + PU_O_POS);
    float *sw = (float *)(base + PU_O_OWN);
    int *sn = (int *)(base + PU_O_OWN) + 8;
    const int ply = g[0], over = g[1];
    bool tree = false, live = false, goes_on = false;
    int kd = 0, nn = 0, PA = 0, PO = 0;
    float ww = 0.0f;
    PuEdge E = { 0, 0, 0, 0, false };
    if (known) {
        const int count = T.hdr[0], pending = T.hdr[2];
        tree = T.hdr[4] == sims && T.hdr[5] == PU_LAYOUT && count >= 1 && count <= nodes && pending < count;
    }
    if (tree && over == 0 && T.hdr[3] == 0) {
        __builtin_amdgcn_wave_barrier();                       // what was there is read
        if (la_observation<S, 64>(T.board, lane, base, pos, PA, PO)) {
            E = pu_edge<S>(base, pos, PA, PO, la_dice((int)T.dice[0]), lane);
            if (lane < 6) {
                kd = T.kind[lane]; nn = T.n[lane]; ww = T.w[lane];
                kd = kd == E.kind ? kd : 0;                    // an edge the rules do not know is no edge
            }
        }
    }
    if (lane < 8) { sw[lane] = ww; sn[lane] = nn; }
    const u32 wins = (u32)__builtin_amdgcn_ballot_w64(kd == 1) & 0x3Fu, searched = (u32)__builtin_amdgcn_ballot_w64(kd == 2) & 0x3Fu;
    __builtin_amdgcn_wave_barrier();
    live = (wins | searched) != 0;
    if (!live) {                                               // over, degenerate, without a move, or no tree: nothing is played
        if (lane < CELLS && R.board) R.board[r * CELLS + lane] = 0;
        if (lane < 6 && R.visits) R.visits[r * 6 + lane] = 0;
        if (lane < 2 && R.action) R.action[r * 2 + lane] = 0;
        if (lane == 0) {
            if (R.dice) R.dice[r] = 0;
            if (R.value) R.value[r] = 0.0f;
            if (R.live) R.live[r] = 0;
            if (tree && over == 0) g[1] = 1;                   // a game that cannot go on is over, without a winner
        }
    } else {
        u32 o[4];
        philox4x32_10((u32)ply, (u32)gid, (u32)(gid >> 32), 0x50555350u, k0, k1, o);
        const int tn = sn[0] + sn[1] + sn[2] + sn[3] + sn[4] + sn[5];
        int best;
        if (wins) best = __builtin_ctz(wins);                  // a win on the board is played
        else {
            u32 ts = 0;                                        // the visits of the searched edges
            #pragma unroll
            for (int i = 0; i < 6; i++) ts += ((searched >> i) & 1u) ? (u32)sn[i] : 0u;
            best = __builtin_ctz(searched);
            if (ply < temp_plies && ts > 0) {                  // in proportion to the visits: the first edge whose running sum passes r
                const u32 r = __umulhi(o[0], ts);
                u32 run = 0;
                bool found = false;
                #pragma unroll
                for (int i = 0; i < 6; i++) {
                    run += ((searched >> i) & 1u) ? (u32)sn[i] : 0u;
                    if (!found && ((searched >> i) & 1u) && run > r) { best = i; found = true; }
                }
            } else {
                int nb = sn[best];
                #pragma unroll
                for (int i = 1; i < 6; i++) if (((searched >> i) & 1u) && sn[i] > nb) { nb = sn[i]; best = i; }
            }
        }
        const int bk = (wins >> best) & 1u ? 1 : 2;
        const int bsrc = __shfl(E.src, best), bdst = __shfl(E.dst, best), bcube = __shfl(E.cube, best);
        if (lane < CELLS) {
            if (R.board) R.board[r * CELLS + lane] = base[lane];
            const int rc = CELLS - 1 - lane;                   // flip(b1)
            int v = base[rc];
            v = rc == bsrc ? 0 : v;
            v = rc == bdst ? bcube : v;
            board[lane] = (int8_t)(-v);
        }
        if (lane < 6 && R.visits) R.visits[r * 6 + lane] = nn;
        if (lane == 0) {
            const float tw = ((((sw[0] + sw[1]) + sw[2]) + sw[3]) + sw[4]) + sw[5];
            if (R.dice) R.dice[r] = T.dice[0];
            if (R.value) R.value[r] = tn > 0 ? tw / (float)tn : 0.0f;
            if (R.action) { R.action[r * 2] = (int8_t)(best / 3); R.action[r * 2 + 1] = (int8_t)(best % 3); }
            if (R.live) R.live[r] = 1;
            dice[0] = (int8_t)(1 + (int)__umulhi(o[1], 6u));
            g[0] = ply + 1;
            if (bk == 1) { g[1] = 1; g[2] = (ply & 1) ? -1 : 1; }
        }
        goes_on = bk != 1;
    }
    __builtin_amdgcn_wave_barrier();                           // this trip's LDS is read: the next may overwrite it
    return goes_on;
}

// ewn_lookahead_expand's order of refusals: arguments, geometry, the empty batch, pointers; then the values -- all before the launch
static inline int pu_refuse(int board_size, int cube_layer, int M)
{
    if (M < 0 || M > INT_MAX / 64) return EWN_EINVAL;          // rows of at most 64 cells are counted in 32 bits
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    return EWN_OK;
}
