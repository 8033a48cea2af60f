// ewn_movetab.hpp -- tables DERIVED from a table image (ewn_fast.hpp), built in LDS by each block of the slot-task rollout kernel
// (k_rollout_slots, ewn_rollout.hpp) from the image it has just copied in.  The image itself (FastTab<S>, FAST_TAB_BYTES,
// build_fast_tables) is what it was.
//
// The step boundary and the search entry of that kernel walk one-byte tables that are all indexed by the same position byte, one
// dependent LDS round trip after another: lgn[pb] -> nbn[dir][pb] -> real_of_ring[pb], real_of_ring[q] for the agent's move,
// nbp[0..2][rp] + real_of_ring twice for the opponent's, and rkf[d][rb] / rsetT[d][rb] for d = 0..2 per replier cube.  Here the
// entries of one position byte sit side by side:
//  * MoveEnt (8 bytes, one table per side: replier geometry nbn / lgn, mover geometry nbp / lgp), per position byte pb:
//      mv = legal directions (bits 0..2) | destination ring cell of direction d << (8 + 8 d)   (255 = the move leaves the board)
//      rc = REAL cell of pb (real_of_ring[pb & 63]) | real cell of destination d << (8 + 8 d)  (0 where there is none)
//    bytes 64..127 ("no such cube") hold no legal direction and destinations 255, as the byte tables do;
//  * ReplyEnt (32 bytes for 32-bit masks, 48 for 64-bit ones), per position byte rb: rsetT[0..2][rb], then rkf[0..2][rb]: a replier
//    cube's setup in d3_search is two or three wide reads in place of six.  48 and not 64 bytes: the address is one 24-bit
//    multiply either way, and 128 x 64 bytes would not fit the kernel's LDS budget.
#pragma once
#include "ewn_fast.hpp"

// Who reads them: the step boundary of k_rollout_slots (ewn_rollout.hpp: the agent half and the max_depth 5 / 6 opponent's move) and
// the PERLANE form of d3_search (ewn_step_d3.hpp: the search entry with the max_depth 1-4 opponent's move).  Two more derived tables
// were built and measured behind a lever of the macro that once switched all of this, and dropped: bit 4, a fused level table
// lv2[ffbh P][ffbh N] (one 16-bit read per leaf in place of the two byte reads of lvl[]), measured slower, profiles/r09/README.md;
// bit 16, a fused leaf table leaf[ix][iy] = { val, rank } of 16-byte entries (one ds_read_b128 per leaf in place of the rank read
// and the value reads a round trip later, 28 KB more LDS per block), which alone gained what the one ordered sum per game gains and
// together with it nothing, profiles/r10/README.md.

struct alignas(8) MoveEnt { u32 mv, rc; };
template <int S, bool WIDE = (sizeof(typename MaskOf<S>::type) == 8)> struct ReplyEnt;
template <int S> struct alignas(16) ReplyEnt<S, false> { u32 rset[3]; u32 rkf[3]; u32 pad[2]; };
template <int S> struct alignas(16) ReplyEnt<S, true> { u64 rset[3]; u32 rkf[3]; u32 pad; };
static_assert(sizeof(MoveEnt) == 8 && sizeof(ReplyEnt<5>) == 32 && sizeof(ReplyEnt<6>) == 48 && sizeof(ReplyEnt<8>) == 48, "entry sizes");

// Where they live.  The replier-side move table goes into the padding behind the struct inside the image's LDS copy (nothing reads
// it) where that holds its 1 KB; everything else is `EXTRA` bytes of the kernel's static LDS array behind what it had.
template <int S> struct SlotTabGeo {
    static constexpr int PAD = FAST_TAB_BYTES(S) - (int)sizeof(FastTab<S>);
    static constexpr bool MOVEN_IN_PAD = PAD >= 128 * (int)sizeof(MoveEnt);
    static constexpr int REPLY_BYTES = 128 * (int)sizeof(ReplyEnt<S>), MOVE_BYTES = 128 * (int)sizeof(MoveEnt);
    static constexpr int EXTRA = REPLY_BYTES + MOVE_BYTES + (MOVEN_IN_PAD ? 0 : MOVE_BYTES);
    static_assert(sizeof(FastTab<S>) % 8 == 0, "a MoveEnt behind the struct is aligned");
    static_assert(EXTRA <= 8 * 1024, "LDS budget of the slot-task kernel: two blocks per CU stay resident");
};
// 5x5 (32-bit masks): 1 920 bytes of padding, the replier-side move table fits; 6x6 - 8x8 (64-bit masks): 384 bytes, nothing fits
static_assert(SlotTabGeo<5>::PAD == 1920 && SlotTabGeo<5>::MOVEN_IN_PAD && SlotTabGeo<5>::EXTRA == 5 * 1024, "5x5: one move table in the image's padding");
static_assert(SlotTabGeo<6>::PAD == 384 && !SlotTabGeo<6>::MOVEN_IN_PAD && SlotTabGeo<6>::EXTRA == 8 * 1024, "6x6: a static array of their own");
static_assert(SlotTabGeo<7>::PAD == 384 && !SlotTabGeo<7>::MOVEN_IN_PAD && SlotTabGeo<7>::EXTRA == 8 * 1024, "7x7: a static array of their own");
static_assert(SlotTabGeo<8>::PAD == 384 && !SlotTabGeo<8>::MOVEN_IN_PAD && SlotTabGeo<8>::EXTRA == 8 * 1024, "8x8: a static array of their own");

template <int S> struct SlotTabs {
    const MoveEnt *mvn, *mvp;   // replier (BOTTOM_RIGHT: the agent) / mover (TOP_LEFT: the opponent)
    const ReplyEnt<S> *rep;
};

// the tables' places: `tb` = the image's LDS copy, `extra` = SlotTabGeo<S>::EXTRA bytes, 16-byte aligned
template <int S> EWN_DEV SlotTabs<S> slot_tabs_at(int8_t *tb, int8_t *extra)
{
    typedef SlotTabGeo<S> G;
    SlotTabs<S> D;
    D.rep = (const ReplyEnt<S> *)extra;
    D.mvp = (const MoveEnt *)(extra + G::REPLY_BYTES);
    D.mvn = G::MOVEN_IN_PAD ? (const MoveEnt *)(tb + sizeof(FastTab<S>)) : (const MoveEnt *)(extra + G::REPLY_BYTES + G::MOVE_BYTES);
    return D;
}

// one side's entry of position byte q: nb / lg = that side's destination and legal-direction tables
template <int S> __host__ EWN_DEV MoveEnt move_ent(const FastTab<S> *Tb, const uint8_t (&nb)[3][128], const uint8_t (&lg)[128], int q)
{
    MoveEnt e;
    e.mv = lg[q];
    e.rc = Tb->real_of_ring[q & 63];
    for (int d = 0; d < 3; d++) {
        const u32 dst = nb[d][q];
        e.mv |= dst << (8 + 8 * d);
        e.rc |= (dst == 255u ? 0u : (u32)Tb->real_of_ring[dst & 63u]) << (8 + 8 * d);
    }
    return e;
}

// The builder, plain C++ over the image (callable on the host too, for checks): entry number `e` of 256 (0..127: the two move
// entries of position byte e; 128..255: the reply entry of position byte e - 128).  A block calls it with e = its thread index,
// after the image has arrived and before the barrier in front of the first use.
template <int S> __host__ EWN_DEV void slot_tabs_build(const FastTab<S> *Tb, const SlotTabs<S> &D, int e)
{
    const int q = e & 127;
    if (e < 128) {
        ((MoveEnt *)D.mvn)[q] = move_ent<S>(Tb, Tb->nbn, Tb->lgn, q);
        ((MoveEnt *)D.mvp)[q] = move_ent<S>(Tb, Tb->nbp, Tb->lgp, q);
    } else {
        ReplyEnt<S> r = {};
        for (int d = 0; d < 3; d++) { r.rset[d] = Tb->rsetT[d][q]; r.rkf[d] = Tb->rkf[d][q]; }
        ((ReplyEnt<S> *)D.rep)[q] = r;
    }
}

// fields of a MoveEnt
EWN_DEV u32 me_legal(const MoveEnt &m) { return m.mv & 7u; }
EWN_DEV int me_dest(const MoveEnt &m, int dir) { return (int)((m.mv >> (8 + 8 * dir)) & 0xFFu); }
EWN_DEV int me_real_src(const MoveEnt &m) { return (int)(m.rc & 0xFFu); }
EWN_DEV int me_real_dest(const MoveEnt &m, int dir) { return (int)((m.rc >> (8 + 8 * dir)) & 0xFFu); }
EWN_DEV MoveEnt me_read(const MoveEnt *t, int pb) { const uint2 v = *(const uint2 *)(t + pb); MoveEnt m; m.mv = v.x; m.rc = v.y; return m; }
