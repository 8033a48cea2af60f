// ewn_playout_search.hip -- the PUCT tree search without a network, in one launch (C ABI: ewn_playout_search, declared in
// include/ewn_playout_search.h): uniform priors and random playouts at the leaves.  What it leaves in `tree` is, byte
// for byte, what ewn_puct_begin and then R rounds of ewn_playout_wins on the leaf rows, the host's value = (2 w - n) / n and
// ewn_puct_advance with zero logits leave there: the tree code is ewn_puct.hpp's, the one copy the staged and the fused kernels
// call, and the playouts are ewn_playout.hpp's, whose playout x starts from seed(word, x) whichever lane plays it.  No leaf row and
// no value leaves the kernel: both live in the wave's own LDS.
//
// A wave per tree, four waves per block, further trees grid-stride with a trip count that is uniform across the block: a wave
// without a tree reaches every barrier and does nothing between them.
//   once:      the block builds its PlayTab
//   per tree:  the wave fills every byte (zeros, child -1) | a block barrier | pu_root: the header, node 0, the leaf row into LDS
//   per round: a block barrier | if the tree has a pending leaf (wave-uniform): pstate_load of the leaf row, run_playouts<0> on all
//              64 lanes with the wave's own LDS counter, a wave sum of the wins, the value into LDS | pu_round on five zero logits
//              and that value: evaluation, backup, one simulation, the new leaf into the wave's LDS row
//
// Which values travel between lanes through global memory, and how (ewn_puct.hpp's rule, the fused form): a tree never leaves its
// wave, every value that one lane writes and another reads is read at the earliest in the round after the one that wrote it, and
// between two rounds (and between the fill and the root) lies __syncthreads.  Every index read from the tree is range-checked by
// pu_round; what `tree` held before the call cannot matter, because every byte is written before any is read.  No atomics on
// global memory: the playouts' `next` counter and pstate_load's four words are LDS atomics of the wave's own.
//
// The second instance, k_playout_search<S, true> (C ABI: ewn_playout_search_eg, include/ewn_playout_search_eg.h): a
// pending leaf that an endgame table covers takes its exact value from the table and runs no playouts.  Byte for byte the sequence
// above with EndgameTable.lookup(leaf rows, leaf dice) before each round's playouts: where the lookup says covered, the value is
// its q at the action it returns, the first maximum of the six under a strict >; elsewhere the playouts' share, under the same key
// and row index as without a table.
//   per round, pending >= 0 (wave-uniform): a ballot counts the row's cubes; with more than max_total the row is not covered
//              (the lookup's test counts the same cells) and is played out.  Else every lane scans the wave's leaf row in LDS
//              (eg_position, the lookup's own coverage test: broadcast reads, the same registers on all 64 lanes).  Covered:
//              lanes 0 .. 5 each gather one eg_move for (f, r) = (lane / 3, lane % 3) -- six independent loads, one memory round
//              trip -- the six go round the wave by shuffles, every lane folds them in action order, lane 0 writes the value
//              into LDS, a wave barrier.  Not covered: the playout branch above, unchanged.
// Every rule above holds for it as it stands: the grid and trip structure, a wave without a tree reaching every barrier, the block
// barrier between the fill and the root and between two rounds, the tree on one wave, pu_round's range checks, every byte written
// before any is read.  The table is only read, with indices that eg_move's argument keeps inside it (the coverage test comes first,
// a move never adds a cube); it must be complete before the launch in stream order.  The geometry (EgGeo) travels by value among the
// kernel's arguments.  leaf_counts (may be NULL): {rounds a table valued, rounds playouts valued} per tree, two wave-uniform
// counters in registers that lane 0 stores once after the round loop, a plain vector store.
#include "ewn_puct.hpp"
#include "ewn_playout.hpp"
#include "ewn_endgame.hpp"
#include "../../include/ewn_playout_search_eg.h"

#define PS_NT 256            // threads per block: four waves, one tree each per trip
#define PS_NW (PS_NT / 64)

// per wave: PU_WAVE bytes of the tree code | the leaf row (64 bytes, zero past the board is not needed: CELLS bytes are read) |
// five zero logits (padded to eight floats) | pstate_load's words | the value | the leaf dice (one byte) | the playouts' next counter
#define PS_O_LEAF PU_WAVE
#define PS_O_LOGITS (PS_O_LEAF + 64)
#define PS_O_GW (PS_O_LOGITS + 8 * 4)
#define PS_O_VALUE (PS_O_GW + 4 * 4)
#define PS_O_DICE (PS_O_VALUE + 4)
#define PS_O_NEXT (PS_O_DICE + 4)
#define PS_WAVE (PS_O_NEXT + 4 + 4)
static_assert(PS_WAVE % 16 == 0 && PS_O_LEAF % 16 == 0 && PS_O_GW % 16 == 0, "every wave's region starts on a 16-byte boundary");

struct PsBuf { const int8_t *boards; const int8_t *dice; uint8_t *tree; };

// the table instance's own arguments; the plain instance carries an empty struct
template <bool EG> struct PsEg {};
template <> struct PsEg<true> { const float *tbl; int *counts; EgGeo g; };

// rounds: R of the contract, 0 .. sims + 1; n: playouts per leaf, 1 .. 4096; k0, k1: the key's halves
template <int S, bool EG = false>
__global__ __launch_bounds__(PS_NT) void k_playout_search(int M, int sims, int rounds, int n, float c_puct, u32 k0, u32 k1, u32 obs_id0,
                                                          PuLayout L, PsBuf B, PsEg<EG> E)
{
    constexpr int CELLS = S * S;
    __shared__ PlayTab tab;
    __shared__ __attribute__((aligned(16))) int8_t lds[PS_NW * PS_WAVE];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    int8_t *base = lds + wave * PS_WAVE;
    int8_t *leaf = base + PS_O_LEAF, *ldice = base + PS_O_DICE;
    float *lg = (float *)(base + PS_O_LOGITS), *val = (float *)(base + PS_O_VALUE);
    int *next = (int *)(base + PS_O_NEXT);
    u32 *gw = (u32 *)(base + PS_O_GW);
    Geom g;                                                    // pstate_load reads the size and the cell count alone
    g.S = S; g.cells = CELLS;
    const u64 key = ((u64)k1 << 32) | (u64)k0;
    const PuNoise Z = { nullptr, 0.0f, 0.0f };

    playtab_build(&tab, S);
    if (lane < 8) lg[lane] = 0.0f;
    if (lane == 0) val[0] = 0.0f;

    const u32 words = (u32)(L.bytes / 4), c0 = L.child / 4, c1 = L.cn / 4;
    const int per_trip = (int)gridDim.x * PS_NW;               // M <= INT_MAX / 64 and at most 4096 blocks: no overflow
    const int trips = (M - 1) / per_trip + 1;                  // M >= 1; block-uniform
    #pragma unroll 1
    for (int trip = 0; trip < trips; trip++) {
        const int m0 = trip * per_trip + (int)blockIdx.x * PS_NW + wave;
        const bool has = m0 < M;                               // wave-uniform
        const size_t m = (size_t)m0;
        const PuTree T = pu_tree(B.tree, has ? m : 0, L);      // not touched without a tree
        if (has) {
            u32 *t = (u32 *)T.hdr;
            #pragma unroll 1
            for (u32 i = lane; i < words; i += 64) t[i] = i >= c0 && i < c1 ? 0xFFFFFFFFu : 0u;
        }
        __syncthreads();                                       // the table is built; the fill is done before the root goes over it
        if (has) pu_root<S>(T, B.boards + m * CELLS, B.dice + m, sims, leaf, ldice, lane, base);
        int by_table = 0, by_playouts = 0;                     // EG: the rounds of this tree that either valued (wave-uniform)
        #pragma unroll 1
        for (int rnd = 0; rnd < rounds; rnd++) {
            __syncthreads();                                   // the tree's words are handed over
            if (has) {
                const int pending = __builtin_amdgcn_readfirstlane(T.hdr[2]);
                bool covered = false;                          // wave-uniform: every lane scans the same row
                if constexpr (EG) {
                    // more cubes on the row than a table position has: not covered whatever else (eg_position counts every cell that
                    // is not empty, or refuses the row for a value outside -6 .. 6), and the scan is skipped
                    const int cubes = pending >= 0 ? __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < CELLS && leaf[lane < CELLS ? lane : 0] != 0)) : 0;
                    if (pending >= 0 && cubes <= E.g.T) {
                        int Ma, Mo, na, no;
                        u64 pa, po;
                        covered = __builtin_amdgcn_readfirstlane((int)eg_position<S>(leaf, E.g.K, E.g.T, Ma, Mo, na, no, pa, po)) != 0;
                        if (covered) {
                            float q = -__builtin_inff();
                            if (lane < 6) q = eg_move<S>(E.tbl, E.g, Ma, Mo, pa, po, la_find(lane / 3, la_dice((int)ldice[0]), Ma), lane % 3);
                            float qb = __shfl(q, 0, 64);           // k_endgame_lookup's fold: the first maximum, -0.0 == +0.0
                            #pragma unroll
                            for (int i = 1; i < 6; i++) { const float qi = __shfl(q, i, 64); if (qi > qb) qb = qi; }
                            if (lane == 0) val[0] = qb;
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                    by_table += covered ? 1 : 0; by_playouts += pending >= 0 && !covered ? 1 : 0;
                }
                if (pending >= 0 && !covered) {                // wave-uniform: the leaf in the wave's row is a position to play out
                    if (lane == 0) *next = 64;                 // the same wave reads it: its LDS operations execute in order
                    const PState b0 = pstate_load(g, leaf, lane, 64, gw);
                    const u32 word = PlayoutRng::obs_word(obs_id0 + (u32)m0, 0x53494D55u, key + (u64)rnd * 0x9E3779B97F4A7C15ull);
                    int w = run_playouts<0>(&tab, b0, S, word, 0u, lane, n, next);
                    #pragma unroll
                    for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
                    if (lane == 0) val[0] = (float)(2 * w - n) / (float)n;
                    __builtin_amdgcn_wave_barrier();
                }
                pu_round<S, false>(T, sims, c_puct, 1.0f, L.nodes, lg, val, Z, leaf, ldice, lane, base);
            }
        }
        if constexpr (EG) {
            if (has && E.counts && lane == 0) { E.counts[2 * m] = by_table; E.counts[2 * m + 1] = by_playouts; }
        }
    }
}

template <int S>
static int ps_launch(int M, int sims, int rounds, int n, float c_puct, uint64_t key, uint32_t obs_id0, unsigned blocks, const PsBuf &b, hipStream_t s)
{
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_playout_search<S>, blocks, PS_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, rounds, n, c_puct, (u32)key,
                             (u32)(key >> 32), (u32)obs_id0, L, b, PsEg<false>{});
}

template <int S>
static int ps_launch_eg(int M, int sims, int rounds, int n, float c_puct, uint64_t key, uint32_t obs_id0, unsigned blocks, const PsBuf &b,
                        const PsEg<true> &e, hipStream_t s)
{
    const PuLayout L = pu_layout(S, sims);
    return pol_launch_kernel(k_playout_search<S, true>, blocks, PS_NT, 0, 64 * 1024, POL_LDS_MAX, s, M, sims, rounds, n, c_puct, (u32)key,
                             (u32)(key >> 32), (u32)obs_id0, L, b, e);
}

// ewn_puct_search's order of refusals with this entry's own values last, all before the launch
int ewn_playout_search(int board_size, int cube_layer, int M, int sims, int rounds, int playouts, float c_puct, uint64_t key,
                       uint32_t obs_id0, int blocks, const int8_t *boards, const int8_t *dice, void *tree, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!boards || !dice || !tree) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS) return EWN_EINVAL;
    if ((uintptr_t)tree & 3) return EWN_EINVAL;
    if (playouts < 1 || playouts > EWN_PLAYOUT_SEARCH_MAX_PLAYOUTS) return EWN_EINVAL;
    if (!std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (blocks < 0 || blocks > EWN_PLAYOUT_SEARCH_MAX_BLOCKS) return EWN_EINVAL;
    const int R = rounds < 0 || rounds > sims + 1 ? sims + 1 : rounds;
    const unsigned grid = blocks > 0 ? (unsigned)blocks : la_blocks(M, PS_NW, EWN_PLAYOUT_SEARCH_MAX_BLOCKS);
    PsBuf b = { boards, dice, (uint8_t *)tree };
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? ps_launch<5>(M, sims, R, playouts, c_puct, key, obs_id0, grid, b, s)
                           : ps_launch<7>(M, sims, R, playouts, c_puct, key, obs_id0, grid, b, s);
}

// ewn_playout_search's refusals in its order, the table's after the entry's own values
int ewn_playout_search_eg(int board_size, int cube_layer, int M, int sims, int rounds, int playouts, float c_puct, uint64_t key,
                          uint32_t obs_id0, int blocks, int max_cubes, int max_total, const float *table,
                          const int8_t *boards, const int8_t *dice, void *tree, int32_t *leaf_counts, void *stream)
{
    const int rc = pu_refuse(board_size, cube_layer, M);
    if (rc != EWN_OK || M == 0) return rc;
    if (!table || !boards || !dice || !tree) return EWN_ENULL;
    if (sims < 0 || sims > PU_MAX_SIMS) return EWN_EINVAL;
    if ((uintptr_t)tree & 3) return EWN_EINVAL;
    if (playouts < 1 || playouts > EWN_PLAYOUT_SEARCH_MAX_PLAYOUTS) return EWN_EINVAL;
    if (!std::isfinite(c_puct) || c_puct < 0.0f) return EWN_EINVAL;
    if (blocks < 0 || blocks > EWN_PLAYOUT_SEARCH_MAX_BLOCKS) return EWN_EINVAL;
    if (!eg_params_ok(board_size, max_cubes, max_total)) return EWN_EINVAL;
    if (((uintptr_t)table & 3) || ((uintptr_t)leaf_counts & 3)) return EWN_EINVAL;
    const int R = rounds < 0 || rounds > sims + 1 ? sims + 1 : rounds;
    const unsigned grid = blocks > 0 ? (unsigned)blocks : la_blocks(M, PS_NW, EWN_PLAYOUT_SEARCH_MAX_BLOCKS);
    PsBuf b = { boards, dice, (uint8_t *)tree };
    PsEg<true> e;
    e.tbl = table; e.counts = leaf_counts;
    eg_geo(board_size, max_cubes, max_total, e.g);
    hipStream_t s = (hipStream_t)stream;
    return board_size == 5 ? ps_launch_eg<5>(M, sims, R, playouts, c_puct, key, obs_id0, grid, b, e, s)
                           : ps_launch_eg<7>(M, sims, R, playouts, c_puct, key, obs_id0, grid, b, e, s);
}
