// ewn_puct.hip -- a PUCT search on the trained actor-critic as tree kernels (C ABI: ewn_puct_tree_bytes, ewn_puct_begin,
// ewn_puct_advance, ewn_puct_result).  The staged shape of 4l: begin lays M trees out and hands their roots over as
// observations, the caller evaluates a row per tree with ewn_predict_policy, advance folds that evaluation into the tree (priors,
// backup) and walks one more simulation down to the next observation to evaluate, result reads the root.  No network runs here and
// no random number enters: the chance nodes are a stratified sample of the dice (the least visited dice first).
// Self-play on these trees (ewn_puct_advance_noise, ewn_puct_play): a second instance of advance mixes the caller's
// weights into the root's priors, and play takes a game's move off its finished tree -- the only kernel here that draws (Philox).
//
// A wave per tree.  Per-edge state (N, W, P, kind, child[.][d'], cn[.][d']) of edge a is read and written by lane a alone, in every
// kernel: a tree's values never travel between lanes through global memory, only through LDS and cross-lane reads.  The node's board
// goes to LDS by ewn_lookahead.hpp's la_observation, so that la_find and la_root apply unchanged.
#include "ewn_lookahead.hpp"
#include <climits>

#define PU_NT 256            // threads per block: four waves, one tree each per trip
#define PU_MAX_BLOCKS 1024   // more trees are walked grid-stride
#define PU_MAX_SIMS 4096
#define PU_LAYOUT 1          // hdr[5]: the version of the layout below (ewn_gym_amd.vec_env.PUCT_LAYOUT)

// per wave: the node's board (64 bytes, zero past the board) | cube positions [16] | 16 words of the kernel's own
#define PU_O_POS 64
#define PU_O_OWN 80
#define PU_WAVE (PU_O_OWN + 16 * 4)

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

struct PuBeginBuf { const int8_t *boards; const int8_t *dice; uint8_t *tree; int8_t *leaf_boards; int8_t *leaf_dice; };
struct PuAdvanceBuf { uint8_t *tree; const float *logits; const float *value; int8_t *leaf_boards; int8_t *leaf_dice; };
struct PuResultBuf { uint8_t *tree; int8_t *actions; int *visits; float *q; float *value; };
// the noise instance's buffers: PuAdvanceBuf first, so that the plain instance's kernel arguments are what they were
struct PuNoiseBuf : PuAdvanceBuf { const float *noise; float eps, keep; };   // noise [M][6]; keep = 1 - eps, formed once on the host
template <bool NOISE> struct PuAdvanceArg { typedef PuAdvanceBuf type; };
template <> struct PuAdvanceArg<true> { typedef PuNoiseBuf type; };
struct PuPlayBuf {
    const uint8_t *tree; int8_t *boards; int8_t *dice; int *game;
    int8_t *rec_board; int8_t *rec_dice; int *rec_visits; float *rec_value; int8_t *rec_action; int8_t *rec_live;
};

// A block per tree: every byte of the tree (zeros, child -1), then wave 0 writes the header, the root and the leaf row
template <int S>
__global__ __launch_bounds__(PU_NT) void k_puct_begin(int M, int sims, PuLayout L, PuBeginBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[PU_WAVE];
    const int lane = threadIdx.x & 63;
    uint8_t *pos = (uint8_t *)(lds + PU_O_POS);
    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x; m0 < M; m0 += (int)gridDim.x) {   // block-uniform
        const size_t m = (size_t)m0;
        u32 *t = (u32 *)(B.tree + m * (size_t)L.bytes);
        #pragma unroll 1
        for (u32 i = threadIdx.x; i < words; i += PU_NT) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        __syncthreads();                                       // the fill is done before the root goes over it
        if (threadIdx.x < 64) {
            const PuTree T = pu_tree(B.tree, m, L);
            int PA, PO;
            __builtin_amdgcn_wave_barrier();                   // what was there is read
            const bool live = la_observation<S, 64>(B.boards + m * CELLS, lane, lds, pos, PA, PO);
            const int d = la_dice((int)B.dice[m]);
            if (lane < CELLS) {
                T.board[lane] = lds[lane];
                B.leaf_boards[m * CELLS + lane] = live ? lds[lane] : (int8_t)0;
            }
            if (lane == 0) {
                T.hdr[0] = 1; T.hdr[1] = 0; T.hdr[2] = live ? 0 : -1; T.hdr[3] = live ? 0 : 1; T.hdr[4] = sims; T.hdr[5] = PU_LAYOUT;
                T.dice[0] = (int8_t)d;
                T.parent[0] = -1;
                B.leaf_dice[m] = (int8_t)(live ? d : 1);
            }
        }
        __syncthreads();                                       // the LDS is read: the next trip may overwrite it
    }
}

// NOISE (ewn_puct_advance_noise): when the node evaluated is the root, its priors are mixed with the caller's
// weights, normalised over the legal edges, before the backup and before the first simulation selects on them
template <int S, bool NOISE>
__global__ __launch_bounds__(PU_NT) void k_puct_advance(int M, int sims, float c_puct, float inv_tv, PuLayout L, typename PuAdvanceArg<NOISE>::type B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(PU_NT / 64) * PU_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * PU_WAVE;
    uint8_t *pos = (uint8_t *)(base + PU_O_POS);
    float *sc = (float *)(base + PU_O_OWN);
    int *isc = (int *)(base + PU_O_OWN) + 8;

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        const PuTree T = pu_tree(B.tree, m, L);
        int count = T.hdr[0], done = T.hdr[1], pending = T.hdr[2];
        // a tree of another budget or layout, or no tree at all, is left alone
        const bool ok = T.hdr[3] == 0 && T.hdr[4] == sims && T.hdr[5] == PU_LAYOUT && count >= 1 && count <= L.nodes && pending < count;
        bool leaf = false;                                     // a new node's observation went to the leaf row
        if (ok) {
            if (pending >= 0) {                                // ---- evaluation: priors from the logits, then backup of v
                int PA, PO;
                __builtin_amdgcn_wave_barrier();               // what was there is read
                la_observation<S, 64>(T.board + (size_t)pending * CELLS, lane, base, pos, PA, PO);
                if (PA != 0 && PO != 0) {
                    const PuEdge E = pu_edge<S>(base, pos, PA, PO, (int)T.dice[pending], lane);
                    const float *lg = B.logits + m * 5;
                    const float l0 = lg[0], l1 = lg[1], l2 = lg[2], l3 = lg[3], l4 = lg[4];
                    const float mf = l1 > l0 ? l1 : l0;
                    const float f0 = expf(l0 - mf), f1 = expf(l1 - mf), sf = f0 + f1;
                    float mr = l3 > l2 ? l3 : l2;
                    mr = l4 > mr ? l4 : mr;
                    const float r0 = expf(l2 - mr), r1 = expf(l3 - mr), r2 = expf(l4 - mr), sr = (r0 + r1) + r2;
                    const int f = lane >= 3, r = lane - 3 * f;
                    const float pf = (f ? f1 : f0) / sf, pr = (r == 0 ? r0 : r == 1 ? r1 : r2) / sr;
                    const float raw = E.kind == 0 ? 0.0f : E.one ? pr : pf * pr;
                    if (lane < 8) sc[lane] = raw;
                    __builtin_amdgcn_wave_barrier();
                    const float sum = ((((sc[0] + sc[1]) + sc[2]) + sc[3]) + sc[4]) + sc[5];
                    if constexpr (NOISE) {
                        float prior = E.kind == 0 ? 0.0f : raw / sum;
                        if (pending == 0) {
                            float eta = 0.0f;
                            if (lane < 6 && E.kind != 0) {
                                const float x = B.noise[m * 6 + lane];
                                eta = x > 0.0f && x < __builtin_inff() ? x : 0.0f;   // NaN, inf, zero and negative numbers: no weight
                            }
                            __builtin_amdgcn_wave_barrier();   // the raw priors are read
                            if (lane < 8) sc[lane] = eta;
                            __builtin_amdgcn_wave_barrier();
                            const float es = ((((sc[0] + sc[1]) + sc[2]) + sc[3]) + sc[4]) + sc[5];
                            if (es > 0.0f && E.kind != 0) prior = B.keep * prior + B.eps * (eta / es);
                        }
                        if (lane < 6) {
                            T.kind[6 * pending + lane] = (int8_t)E.kind;
                            T.p[6 * pending + lane] = prior;
                        }
                    } else if (lane < 6) {
                        T.kind[6 * pending + lane] = (int8_t)E.kind;
                        T.p[6 * pending + lane] = E.kind == 0 ? 0.0f : raw / sum;
                    }
                    float v = B.value[m] * inv_tv;
                    v = v > -1.0f ? v : -1.0f;
                    v = v < 1.0f ? v : 1.0f;
                    pu_backup(T, pending, v, lane, L.nodes);
                }
                pending = -1;
            }
            if (done < sims) {                                 // ---- one simulation: down to a new node or a winning edge
                done++;
                int j = 0;
                #pragma unroll 1
                for (int step = 0; step < L.nodes; step++) {   // a path holds at most `count` nodes
                    int PA, PO;
                    __builtin_amdgcn_wave_barrier();           // what was there is read
                    la_observation<S, 64>(T.board + (size_t)j * CELLS, lane, base, pos, PA, PO);
                    if (PA == 0 || PO == 0) break;
                    const PuEdge E = pu_edge<S>(base, pos, PA, PO, (int)T.dice[j], lane);
                    const int nn = lane < 6 ? T.n[6 * j + lane] : 0;
                    const float ww = lane < 6 ? T.w[6 * j + lane] : 0.0f, pp = lane < 6 ? T.p[6 * j + lane] : 0.0f;
                    if (lane < 8) isc[lane] = nn;
                    __builtin_amdgcn_wave_barrier();
                    const int Ns = isc[0] + isc[1] + isc[2] + isc[3] + isc[4] + isc[5];
                    const float rs = (float)sqrt((double)(Ns + 1));   // the correctly rounded fp32 root of an integer
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
                    if (bk == 1) {                             // the move wins: +1 from this node, no network call
                        if (lane == best) { T.w[6 * j + best] += 1.0f; T.n[6 * j + best] += 1; }
                        pu_backup(T, j, 1.0f, lane, L.nodes);
                        break;
                    }
                    int dsel = 1, c = -1;                      // chance: the least visited dice, the first of them
                    if (lane == best) {
                        const int16_t *cn = T.cn + 36 * j + 6 * best;
                        int mn = cn[0];
                        #pragma unroll
                        for (int i = 1; i < 6; i++) { const int x = cn[i]; if (x < mn) { mn = x; dsel = i + 1; } }
                        c = T.child[36 * j + 6 * best + dsel - 1];
                    }
                    dsel = __shfl(dsel, best); c = __shfl(c, best);
                    if (c >= 0) {
                        if (c >= count || c <= j) break;       // no tree
                        j = c;
                        continue;
                    }
                    if (count >= L.nodes) break;
                    const int idx = count++;                   // a new node: flip(b1) under dsel, the pending leaf
                    if (lane == best) T.child[36 * j + 6 * best + dsel - 1] = (int16_t)idx;
                    if (lane < CELLS) {
                        const int rc = CELLS - 1 - lane;
                        int v = base[rc];
                        v = rc == bsrc ? 0 : v;
                        v = rc == bdst ? bcube : v;
                        const int8_t nb = (int8_t)(-v);
                        T.board[(size_t)idx * CELLS + lane] = nb;
                        B.leaf_boards[m * CELLS + lane] = nb;
                    }
                    if (lane == 0) {
                        T.dice[idx] = (int8_t)dsel;
                        T.parent[4 * idx] = (int16_t)j; T.parent[4 * idx + 1] = (int16_t)best; T.parent[4 * idx + 2] = (int16_t)dsel;
                        B.leaf_dice[m] = (int8_t)dsel;
                    }
                    pending = idx;
                    leaf = true;
                    break;
                }
            }
            if (lane == 0) { T.hdr[0] = count; T.hdr[1] = done; T.hdr[2] = pending; }
        }
        if (!leaf) {
            if (lane < CELLS) B.leaf_boards[m * CELLS + lane] = 0;
            if (lane == 0) B.leaf_dice[m] = 1;
        }
        __builtin_amdgcn_wave_barrier();                       // this trip's LDS is read: the next may overwrite it
    }
}

// The root's picture.  The budget (and with it the tree's size) is read from the first tree's header: begin wrote it
__global__ __launch_bounds__(PU_NT) void k_puct_result(int S, int M, PuResultBuf B)
{
    __shared__ __attribute__((aligned(16))) float lds[(PU_NT / 64) * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *sw = lds + wave * 16;
    int *sn = (int *)sw + 8;
    const float inf = __builtin_inff();
    const int sims = ((const int *)B.tree)[4];
    const bool known = sims >= 0 && sims <= PU_MAX_SIMS && ((const int *)B.tree)[5] == PU_LAYOUT;
    const PuLayout L = pu_layout(S, known ? sims : 0);

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        int kd = 0, nn = 0;
        float ww = 0.0f;
        if (known) {
            const PuTree T = pu_tree(B.tree, m, L);
            if (T.hdr[3] == 0 && T.hdr[4] == sims && lane < 6) { kd = T.kind[lane]; nn = T.n[lane]; ww = T.w[lane]; }
        }
        if (lane < 8) { sw[lane] = ww; sn[lane] = nn; }
        const u32 wins = (u32)__builtin_amdgcn_ballot_w64(kd == 1) & 0x3Fu, searched = (u32)__builtin_amdgcn_ballot_w64(kd == 2) & 0x3Fu;
        __builtin_amdgcn_wave_barrier();
        if (lane < 6) {
            if (B.visits) B.visits[m * 6 + lane] = nn;
            if (B.q) B.q[m * 6 + lane] = kd == 0 ? -inf : kd == 1 ? 1.0f : nn > 0 ? ww / (float)nn : 0.0f;
        }
        if (lane == 0) {
            const float tw = ((((sw[0] + sw[1]) + sw[2]) + sw[3]) + sw[4]) + sw[5];
            const int tn = sn[0] + sn[1] + sn[2] + sn[3] + sn[4] + sn[5];
            if (B.value) B.value[m] = tn > 0 ? tw / (float)tn : 0.0f;
            int best = 0;
            if (wins) best = __builtin_ctz(wins);              // a win on the board is played
            else if (searched) {
                best = __builtin_ctz(searched);
                int nb = sn[best];
                #pragma unroll
                for (int i = 1; i < 6; i++) if (((searched >> i) & 1u) && sn[i] > nb) { nb = sn[i]; best = i; }
            }
            B.actions[m * 2] = (int8_t)(best / 3); B.actions[m * 2 + 1] = (int8_t)(best % 3);
        }
        __builtin_amdgcn_wave_barrier();                       // this trip's LDS is read: the next may overwrite it
    }
}

// The move of a self-play game off a finished tree (ewn_puct_play): a wave per game, the position played is the tree's
// root.  The edge is the first winning one, else drawn in proportion to the root's visits while ply < temp_plies (integer
// arithmetic on a Philox word), else k_puct_result's first maximum; the record row, the board after the move seen from the other
// side, the next dice (a second Philox word) and the game's state are written.  The budget is read from the first tree's header
template <int S>
__global__ __launch_bounds__(PU_NT) void k_puct_play(int M, int temp_plies, u32 k0, u32 k1, long long game_offset, PuPlayBuf B)
{
    constexpr int CELLS = S * S;
    __shared__ __attribute__((aligned(16))) int8_t lds[(PU_NT / 64) * PU_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int8_t *base = lds + wave * PU_WAVE;
    uint8_t *pos = (uint8_t *)(base + PU_O_POS);
    float *sw = (float *)(base + PU_O_OWN);
    int *sn = (int *)(base + PU_O_OWN) + 8;
    const int sims = ((const int *)B.tree)[4];
    const bool known = sims >= 0 && sims <= PU_MAX_SIMS && ((const int *)B.tree)[5] == PU_LAYOUT;
    const PuLayout L = pu_layout(S, known ? sims : 0);

    #pragma unroll 1
    for (int m0 = (int)blockIdx.x * (PU_NT / 64) + wave; m0 < M; m0 += (int)gridDim.x * (PU_NT / 64)) {   // wave-uniform
        const size_t m = (size_t)m0;
        int *g = B.game + m * 4;
        const int ply = g[0], over = g[1];
        const PuTree T = pu_tree((uint8_t *)B.tree, m, L);     // read only
        bool tree = false, live = false;
        int kd = 0, nn = 0, PA = 0, PO = 0;
        float ww = 0.0f;
        PuEdge E = { 0, 0, 0, 0, false };
        if (known) {
            const int count = T.hdr[0], pending = T.hdr[2];
            tree = T.hdr[4] == sims && T.hdr[5] == PU_LAYOUT && count >= 1 && count <= L.nodes && pending < count;
        }
        if (tree && over == 0 && T.hdr[3] == 0) {
            __builtin_amdgcn_wave_barrier();                   // what was there is read
            if (la_observation<S, 64>(T.board, lane, base, pos, PA, PO)) {
                E = pu_edge<S>(base, pos, PA, PO, la_dice((int)T.dice[0]), lane);
                if (lane < 6) {
                    kd = T.kind[lane]; nn = T.n[lane]; ww = T.w[lane];
                    kd = kd == E.kind ? kd : 0;                // an edge the rules do not know is no edge
                }
            }
        }
        if (lane < 8) { sw[lane] = ww; sn[lane] = nn; }
        const u32 wins = (u32)__builtin_amdgcn_ballot_w64(kd == 1) & 0x3Fu, searched = (u32)__builtin_amdgcn_ballot_w64(kd == 2) & 0x3Fu;
        __builtin_amdgcn_wave_barrier();
        live = (wins | searched) != 0;
        if (!live) {                                           // over, degenerate, without a move, or no tree: nothing is played
            if (lane < CELLS && B.rec_board) B.rec_board[m * CELLS + lane] = 0;
            if (lane < 6 && B.rec_visits) B.rec_visits[m * 6 + lane] = 0;
            if (lane < 2 && B.rec_action) B.rec_action[m * 2 + lane] = 0;
            if (lane == 0) {
                if (B.rec_dice) B.rec_dice[m] = 0;
                if (B.rec_value) B.rec_value[m] = 0.0f;
                if (B.rec_live) B.rec_live[m] = 0;
                if (tree && over == 0) g[1] = 1;               // a game that cannot go on is over, without a winner
            }
        } else {
            u32 o[4];
            const unsigned long long gid = (unsigned long long)game_offset + (unsigned long long)m;
            philox4x32_10((u32)ply, (u32)gid, (u32)(gid >> 32), 0x50555350u, k0, k1, o);
            const int tn = sn[0] + sn[1] + sn[2] + sn[3] + sn[4] + sn[5];
            int best;
            if (wins) best = __builtin_ctz(wins);              // a win on the board is played
            else {
                u32 ts = 0;                                    // the visits of the searched edges
                #pragma unroll
                for (int i = 0; i < 6; i++) ts += ((searched >> i) & 1u) ? (u32)sn[i] : 0u;
                best = __builtin_ctz(searched);
                if (ply < temp_plies && ts > 0) {              // in proportion to the visits: the first edge whose running sum passes r
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
                if (B.rec_board) B.rec_board[m * CELLS + lane] = base[lane];
                const int rc = CELLS - 1 - lane;               // flip(b1)
                int v = base[rc];
                v = rc == bsrc ? 0 : v;
                v = rc == bdst ? bcube : v;
                B.boards[m * CELLS + lane] = (int8_t)(-v);
            }
            if (lane < 6 && B.rec_visits) B.rec_visits[m * 6 + lane] = nn;
            if (lane == 0) {
                const float tw = ((((sw[0] + sw[1]) + sw[2]) + sw[3]) + sw[4]) + sw[5];
                if (B.rec_dice) B.rec_dice[m] = T.dice[0];
                if (B.rec_value) B.rec_value[m] = tn > 0 ? tw / (float)tn : 0.0f;
                if (B.rec_action) { B.rec_action[m * 2] = (int8_t)(best / 3); B.rec_action[m * 2 + 1] = (int8_t)(best % 3); }
                if (B.rec_live) B.rec_live[m] = 1;
                B.dice[m] = (int8_t)(1 + (int)__umulhi(o[1], 6u));
                g[0] = ply + 1;
                if (bk == 1) { g[1] = 1; g[2] = (ply & 1) ? -1 : 1; }
            }
        }
        __builtin_amdgcn_wave_barrier();                       // this trip's LDS is read: the next may overwrite it
    }
}

// ewn_lookahead_expand's order of refusals: arguments, geometry, the empty batch, pointers; then the values -- all before the launch
static inline int pu_refuse(int board_size, int cube_layer, int M)
{
    if (M < 0 || M > INT_MAX / 64) return EWN_EINVAL;          // rows of at most 64 cells are counted in 32 bits
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    return EWN_OK;
}

int64_t ewn_puct_tree_bytes(int board_size, int cube_layer, int sims)
{
    if (ewn_policy_param_count(board_size, cube_layer) < 0) return EWN_EUNSUPPORTED;
    if (sims < 0 || sims > PU_MAX_SIMS) return EWN_EINVAL;
    return pu_layout(board_size, sims).bytes;
}

int ewn_puct_begin(int board_size, int cube_layer, int M, int sims, const int8_t *boards, const int8_t *dice, void *tree,
                   int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !tree || !leaf_boards || !leaf_dice) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)tree & 3)) return EWN_EINVAL;
    const PuLayout L = pu_layout(board_size, sims);
    PuBeginBuf b = { boards, dice, (uint8_t *)tree, leaf_boards, leaf_dice };
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, 1, PU_MAX_BLOCKS);
    return board_size == 5 ? pol_launch_kernel(k_puct_begin<5>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, L, b)
                           : pol_launch_kernel(k_puct_begin<7>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, L, b);
}

// both advance entry points: the refusals in one order, `missing` says whether a pointer of the caller's own is NULL
template <bool NOISE>
static int pu_advance(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, bool missing, float noise_eps,
                      typename PuAdvanceArg<NOISE>::type b, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (missing || !b.tree || !b.logits || !b.value || !b.leaf_boards || !b.leaf_dice) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS || ((uintptr_t)b.tree & 3)) return EWN_EINVAL;
    if (!std::isfinite(terminal_value) || !(terminal_value > 0.0f) || !std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (!(noise_eps >= 0.0f && noise_eps <= 1.0f)) return EWN_EINVAL;   // NaN is refused here as well
    const PuLayout L = pu_layout(board_size, sims);
    const float inv_tv = 1.0f / terminal_value;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS);
    return board_size == 5 ? pol_launch_kernel(k_puct_advance<5, NOISE>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, c_puct, inv_tv, L, b)
                           : pol_launch_kernel(k_puct_advance<7, NOISE>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, c_puct, inv_tv, L, b);
}

int ewn_puct_advance(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                     const float *logits, const float *value, int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    PuAdvanceBuf b = { (uint8_t *)tree, logits, value, leaf_boards, leaf_dice };
    return pu_advance<false>(board_size, cube_layer, M, sims, c_puct, terminal_value, false, 0.0f, b, stream);
}

int ewn_puct_advance_noise(int board_size, int cube_layer, int M, int sims, float c_puct, float terminal_value, void *tree,
                           const float *logits, const float *value, const float *root_noise, float noise_eps,
                           int8_t *leaf_boards, int8_t *leaf_dice, void *stream)
{
    PuNoiseBuf b;
    b.tree = (uint8_t *)tree; b.logits = logits; b.value = value; b.leaf_boards = leaf_boards; b.leaf_dice = leaf_dice;
    b.noise = root_noise; b.eps = noise_eps; b.keep = 1.0f - noise_eps;
    return pu_advance<true>(board_size, cube_layer, M, sims, c_puct, terminal_value, root_noise == nullptr, noise_eps, b, stream);
}

int ewn_puct_result(int board_size, int cube_layer, int M, const void *tree, int8_t *actions, int32_t *visits, float *q, float *value,
                    void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!tree || !actions) return EWN_ENULL;
    if ((uintptr_t)tree & 3) return EWN_EINVAL;
    PuResultBuf b = { (uint8_t *)tree, actions, visits, q, value };
    return pol_launch_kernel(k_puct_result, la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS), PU_NT, 0, 64 * 1024, POL_LDS_MAX, (hipStream_t)stream, board_size, M, b);
}

int ewn_puct_play(int board_size, int cube_layer, int M, const void *tree, int8_t *boards, int8_t *dice, int32_t *game,
                  int temp_plies, uint64_t key, int64_t game_offset,
                  int8_t *rec_board, int8_t *rec_dice, int32_t *rec_visits, float *rec_value, int8_t *rec_action, int8_t *rec_live,
                  void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!tree || !boards || !dice || !game) return EWN_ENULL;
    if (temp_plies < 0 || ((uintptr_t)tree & 3) || ((uintptr_t)game & 3)) return EWN_EINVAL;
    PuPlayBuf b = { (const uint8_t *)tree, boards, dice, (int *)game, rec_board, rec_dice, (int *)rec_visits, rec_value, rec_action, rec_live };
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = la_blocks(M, PU_NT / 64, PU_MAX_BLOCKS);
    const u32 k0 = (u32)key, k1 = (u32)(key >> 32);
    return board_size == 5 ? pol_launch_kernel(k_puct_play<5>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, temp_plies, k0, k1, (long long)game_offset, b)
                           : pol_launch_kernel(k_puct_play<7>, blocks, PU_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, temp_plies, k0, k1, (long long)game_offset, b);
}
