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
//  * the PHANTOM form of ReplyEnt (16 bytes for 32-bit masks, 32 for 64-bit ones; 5x5 and 6x6, (level, count) images, max_depth
//    1-4: slot_phantom below): the three masks alone.  What rkf steers -- a reply that does not exist reads "no such reply", a
//    reply onto the origin reads -10 -- comes out of the lookups a leaf does anyway: the entry's mask holds ONE bit above the
//    board in place of the destination (the top bit: no such reply; the one below it: onto the origin), the replier side's mask
//    then has its highest bit there, lvl[0] / lvl[1] answer the two levels no cell of these boards has (7 and 6), and the columns
//    of those levels hold FAST_NONE8 / 8 x m10 in every row of rank[].  The block writes those two level bytes and 16 columns
//    into ITS LDS COPY of the image (slot_tabs_build); the image itself is what it was.
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
// the phantom form exists where levels 6 and 7 are free (5x5: levels 0..4, 6x6: 0..5); the kernel asks for it where its search reads
// (level, count) images at max_depth 1-4 (k_rollout_slots: OPP == 0 && !H2)
template <int S> constexpr bool slot_phantom = S <= 6;
#define PH_LVL_NONE 7   // the level of "no such reply": columns 56..63
#define PH_LVL_HOME 6   // the level of "reply onto the origin": columns 48..55
template <int S, bool PH = false, bool WIDE = (sizeof(typename MaskOf<S>::type) == 8)> struct ReplyEnt;
template <int S> struct alignas(16) ReplyEnt<S, false, false> { u32 rset[3]; u32 rkf[3]; u32 pad[2]; };
template <int S> struct alignas(16) ReplyEnt<S, false, true> { u64 rset[3]; u32 rkf[3]; u32 pad; };
template <int S> struct alignas(16) ReplyEnt<S, true, false> { u32 rset[3]; u32 pad; };
template <int S> struct alignas(16) ReplyEnt<S, true, true> { u64 rset[3]; u64 pad; };
static_assert(sizeof(MoveEnt) == 8 && sizeof(ReplyEnt<5>) == 32 && sizeof(ReplyEnt<6>) == 48 && sizeof(ReplyEnt<8>) == 48, "entry sizes");
static_assert(sizeof(ReplyEnt<5, true>) == 16 && sizeof(ReplyEnt<6, true>) == 32, "entry sizes, phantom form");
// the two phantom cells of a mask type: its top bit and the one below
template <int S> struct PhantomBits {
    typedef typename MaskOf<S>::type M;
    static constexpr M NONE = (M)1 << (8 * sizeof(M) - 1), HOME = (M)1 << (8 * sizeof(M) - 2);
    static_assert(S * S <= 8 * (int)sizeof(M) - 2, "the two bits lie above the board");
    // clz of the two bits is 0 and 1: lvl[0] and lvl[1], which no real cell reaches (clz >= 8 sizeof(M) - S S), become levels 7 and 6;
    // the real levels are 0..S-1
    static_assert(S - 1 < PH_LVL_HOME && 8 * (int)sizeof(M) - S * S > 1, "levels 6 and 7 and lvl[0..1] are free");
};

// Where they live.  The replier-side move table goes into the padding behind the struct inside the image's LDS copy (nothing reads
// it) where that holds its 1 KB; everything else is `EXTRA` bytes of the kernel's static LDS array behind what it had.
template <int S, bool PH = false> struct SlotTabGeo {
    static_assert(!PH || slot_phantom<S>, "phantom cells: 5x5 and 6x6");
    static constexpr int PAD = FAST_TAB_BYTES(S) - (int)sizeof(FastTab<S>);
    static constexpr bool MOVEN_IN_PAD = PAD >= 128 * (int)sizeof(MoveEnt);
    static constexpr int REPLY_BYTES = 128 * (int)sizeof(ReplyEnt<S, PH>), MOVE_BYTES = 128 * (int)sizeof(MoveEnt);
    static constexpr int EXTRA = REPLY_BYTES + MOVE_BYTES + (MOVEN_IN_PAD ? 0 : MOVE_BYTES);
    static_assert(sizeof(FastTab<S>) % 8 == 0, "a MoveEnt behind the struct is aligned");
    static_assert(REPLY_BYTES % 16 == 0, "the move tables behind the reply table stay aligned");
    static_assert(EXTRA <= 8 * 1024, "LDS budget of the slot-task kernel: two blocks per CU stay resident");
};
// 5x5 (32-bit masks): 1 920 bytes of padding, the replier-side move table fits; 6x6 - 8x8 (64-bit masks): 384 bytes, nothing fits
static_assert(SlotTabGeo<5>::PAD == 1920 && SlotTabGeo<5>::MOVEN_IN_PAD && SlotTabGeo<5>::EXTRA == 5 * 1024, "5x5: one move table in the image's padding");
static_assert(SlotTabGeo<6>::PAD == 384 && !SlotTabGeo<6>::MOVEN_IN_PAD && SlotTabGeo<6>::EXTRA == 8 * 1024, "6x6: a static array of their own");
static_assert(SlotTabGeo<7>::PAD == 384 && !SlotTabGeo<7>::MOVEN_IN_PAD && SlotTabGeo<7>::EXTRA == 8 * 1024, "7x7: a static array of their own");
static_assert(SlotTabGeo<8>::PAD == 384 && !SlotTabGeo<8>::MOVEN_IN_PAD && SlotTabGeo<8>::EXTRA == 8 * 1024, "8x8: a static array of their own");
static_assert(SlotTabGeo<5, true>::EXTRA == 3 * 1024 && SlotTabGeo<6, true>::EXTRA == 6 * 1024, "phantom form: 2 KB less");

template <int S, bool PH = false> struct SlotTabs {
    const MoveEnt *mvn, *mvp;   // replier (BOTTOM_RIGHT: the agent) / mover (TOP_LEFT: the opponent)
    const ReplyEnt<S, PH> *rep;
};

// the tables' places: `tb` = the image's LDS copy, `extra` = SlotTabGeo<S, PH>::EXTRA bytes, 16-byte aligned
template <int S, bool PH = false> EWN_DEV SlotTabs<S, PH> slot_tabs_at(int8_t *tb, int8_t *extra)
{
    typedef SlotTabGeo<S, PH> G;
    SlotTabs<S, PH> D;
    D.rep = (const ReplyEnt<S, PH> *)extra;
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
// PH: `Tb` is the block's own, writable copy of the image, and every e also writes four entries of the 16 constant columns of
// rank[] (row e / 4: 256 x 4 = 64 rows x 16 columns); e = 255 writes the two level bytes.  Nothing else reads those entries:
// no mask of a 5x5 or 6x6 board has a cell of level 6 or 7, and no count reaches 8 (FastTab: t <= 7, n <= 6).
template <int S, bool PH = false> __host__ EWN_DEV void slot_tabs_build(const FastTab<S> *Tb, const SlotTabs<S, PH> &D, int e)
{
    const int q = e & 127;
    if (e < 128) {
        ((MoveEnt *)D.mvn)[q] = move_ent<S>(Tb, Tb->nbn, Tb->lgn, q);
        ((MoveEnt *)D.mvp)[q] = move_ent<S>(Tb, Tb->nbp, Tb->lgp, q);
    } else {
        ReplyEnt<S, PH> r = {};
        if constexpr (PH) {
            // what rkf says, as a cell: keep = 0 and fixed = 0 -> no such reply, fixed = 2 (rank[1]) -> onto the origin
            for (int d = 0; d < 3; d++) {
                const u32 kf = Tb->rkf[d][q];
                r.rset[d] = (kf & 0xFFFFu) ? Tb->rsetT[d][q] : ((kf >> 16) ? PhantomBits<S>::HOME : PhantomBits<S>::NONE);
            }
        } else {
            for (int d = 0; d < 3; d++) { r.rset[d] = Tb->rsetT[d][q]; r.rkf[d] = Tb->rkf[d][q]; }
        }
        ((ReplyEnt<S, PH> *)D.rep)[q] = r;
    }
    if constexpr (PH) {
        FastTab<S> *Tw = const_cast<FastTab<S> *>(Tb);
        const int ix = e >> 2, c0 = 8 * PH_LVL_HOME + 4 * (e & 3);   // columns 48..55: -10, 56..63: no such reply
        const uint16_t v = c0 < 8 * PH_LVL_NONE ? (uint16_t)(8 * Tb->m10) : (uint16_t)FAST_NONE8;
        for (int j = 0; j < 4; j++) Tw->rank[ft_index(ix, c0 + j)] = v;
        if (e == 255) { Tw->lvl[0] = (uint8_t)(PH_LVL_NONE << 3); Tw->lvl[1] = (uint8_t)(PH_LVL_HOME << 3); }
    }
}

// fields of a MoveEnt
EWN_DEV u32 me_legal(const MoveEnt &m) { return m.mv & 7u; }
EWN_DEV int me_dest(const MoveEnt &m, int dir) { return (int)((m.mv >> (8 + 8 * dir)) & 0xFFu); }
EWN_DEV int me_real_src(const MoveEnt &m) { return (int)(m.rc & 0xFFu); }
EWN_DEV int me_real_dest(const MoveEnt &m, int dir) { return (int)((m.rc >> (8 + 8 * dir)) & 0xFFu); }
EWN_DEV MoveEnt me_read(const MoveEnt *t, int pb) { const uint2 v = *(const uint2 *)(t + pb); MoveEnt m; m.mv = v.x; m.rc = v.y; return m; }
