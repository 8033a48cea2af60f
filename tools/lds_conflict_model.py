"""CPU model of the LDS bank conflicts of d3_search's table reads in the headline rollout kernel (k_rollout_slots<5, 2, ...>).

  python tools/lds_conflict_model.py [--lanes 2048] [--steps 40] [--waves 4000]

Positions come from the CPU oracle on the bench's seeds and Philox key: after every env step the observed boards get one uniformly
random legal agent move (the bench's agent) and a uniform opponent dice -- the positions the opponent's depth-3 search starts from.
A search task is (position, root cube); a wave holds 32 tasks drawn at random from the pool (the slot-task kernel's lanes pick up
tasks as they finish, so the games of a wave are at unrelated stages), two lanes per task: lane = 2 * task + sub, the 32-lane halves
are tasks 0-15 and 16-31.  Per task the kernel's staged phase issues, for each of the three root directions, nine rank reads
(cube sub + 2 * ii, reply direction d) and nine value reads val[a0], val[min(a0, a1)], val[min(a0, a1, a2)].

Bank rule (LDS of gfx950): a 16-bit or 32-bit read banks by (byte address / 4) % 32, a 64-bit read by (byte address / 4) % 64, both
within each 32-lane half; lanes reading the same dword (64-bit read: the same 8 bytes) are served together; every further distinct
address on a bank costs one more LDS cycle.  The model prints, per layout, the mean cycles per half-wave read (1.0 = conflict-free)
and the extra cycles per wave-level read instruction (two halves) -- the quantity SQ_LDS_BANK_CONFLICT / instruction measures.

--lv2 adds a table the 5x5 search does NOT ship (built and measured slower, profiles/r09/README.md): both levels' share of a leaf's
rank address in one 16-bit read at lv2[zP][zN], zP / zN = v_ffbh_u32 of the leaf's two ring-space masks (31 - the highest ring
index, -1 for an empty mask), issued for steered leaves too, in place of the two byte reads of lvl[] (72 bytes on 18 banks: one
cycle each).  The candidates are row strides in bytes; the figures of profiles/r09 come from here.

--leaf adds the fused leaf table of the 5x5 search (ewn_movetab.hpp): leaf[ix][iy] = {val, rank}, 16 bytes, ONE 128-bit read per leaf in
place of the rank read and (a third of) the value reads.  A 128-bit read banks by (byte address / 4) % 64 and is served in four
groups of 16 lanes -- lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same plus 32 -- one cycle per group when no two lanes
of a group read distinct entries on one bank.  Steered leaves read entry 0 ("no such reply") or entry 1 (a reply onto the origin).
The candidates are row strides in ENTRIES (39 = the table's own width); printed: cycles per 16-lane group and per wave instruction
(4.0 = conflict-free, the same LDS-array time as the 16-bit read + the 64-bit read it replaces), profiles/r10/README.md.

Not modelled: the byte-wide reads of the small tables and the six val6[] reads of a root's expectation (they need the cut-off replay).
"""
import argparse
import collections
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 5
DIRS = ((0, 1), (1, 0), (1, 1))   # canonical space: the P side (the opponent) moves +, the N side (the agent) moves -


def rank_lookup():
    """(ix, iy) -> byte-offset rank (8 x rank), read from the host image the library builds, through its own address query"""
    from ewn_gym_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ewn_tables_bytes.restype = C.c_int64
    n = lib.ewn_tables_bytes(S, 3)
    buf = (C.c_uint8 * n)()
    assert lib.ewn_build_tables(S, 3, buf) == 0
    img = np.frombuffer(buf, np.uint8)
    off = lib.ewn_tables_rank_offset
    tab = np.zeros((64, 64), np.int64)
    for ix in range(64):
        for iy in range(64):
            o = off(S, ix, iy)
            tab[ix, iy] = int(img[o]) | (int(img[o + 1]) << 8)
    return tab


# ring order of the canonical cells (RingGeo, ewn_step_d3.hpp): ascending min(row, col), row-major inside a level
RING = {}
for _t in range(S):
    for _i in range(S):
        for _j in range(S):
            if min(_i, _j) == _t:
                RING[(_i, _j)] = len(RING)


def ffbh(cells):
    """v_ffbh_u32 of a side's ring-space mask"""
    return 31 - max(RING[c] for c in cells) if cells else -1


def side_index(cells):
    """(level, count) index of a side: 8 x the highest level min(i, j) of its cubes + their number; 0 for an empty side"""
    return 8 * max(min(c) for c in cells) + len(cells) if cells else 0


def search_tasks(board, dice_opp):
    """the search tasks of one position (real-space board, agent > 0) as lists of 3 root directions x 2 lanes x 9 (ix, iy, steer, zP, zN)"""
    P, N = {}, {}   # cube number -> canonical cell (board rotated by 180 degrees)
    for i in range(S):
        for j in range(S):
            v = int(board[i, j])
            if v < 0:
                P[-v] = (S - 1 - i, S - 1 - j)
            elif v > 0:
                N[v] = (S - 1 - i, S - 1 - j)
    if not P or not N:
        return []
    if dice_opp in P:
        roots = [dice_opp]
    else:   # the larger neighbour first, then the smaller (find_near_cube)
        up = [k for k in sorted(P) if k > dice_opp][:1]
        dn = [k for k in sorted(P, reverse=True) if k < dice_opp][:1]
        roots = up + dn
    tasks = []
    for rc in roots:
        task = []
        for di, dj in DIRS:
            rp = P[rc]
            dest = (rp[0] + di, rp[1] + dj)
            ok = dest[0] < S and dest[1] < S
            P1 = set(P.values()) - {rp}
            N1 = set(N.values())
            if ok:
                P1 |= {dest}
                N1 -= {dest}
            reads = [[], []]
            for sub in range(2):
                for ii in range(3):
                    k = sub + 2 * ii + 1
                    for d, (ei, ej) in enumerate(DIRS):
                        if k not in N:   # cube off the board: rank[0]; the level read sees the root's masks (less a stale bit)
                            reads[sub].append((0, 0, 1, ffbh(P1), ffbh(N1))); continue
                        c = N[k]
                        dn_ = (c[0] - ei, c[1] - ej)
                        if dn_[0] < 0 or dn_[1] < 0:
                            reads[sub].append((0, 0, 1, ffbh(P1), ffbh(N1 - {c}))); continue   # no such reply: rank[0]
                        N2 = (N1 - {c}) | {dn_}
                        P2 = P1 - {dn_}
                        if dn_ == (0, 0):
                            reads[sub].append((0, 1, 1, ffbh(P2), ffbh(N2))); continue           # reply onto the origin: rank[1]
                        reads[sub].append((side_index(P2), side_index(N2), 0, ffbh(P2), ffbh(N2)))
            task.append(reads)
        tasks.append(task)
    return tasks


def positions(lanes, steps, rng):
    from oracle import pyoracle as po
    env = po.OracleVecEnv(lanes, opponent="minimax", max_depth=3, rng="philox", philox_key=2024, autoreset=True, seed_stride=65536)
    env.reset(seeds=(np.arange(lanes, dtype=np.uint64) + 9487).astype(np.uint32))
    out = []
    for t in range(steps):
        b, d = env.obs()
        for g in rng.choice(lanes, size=min(lanes, 256), replace=False):   # a sample of every step: all game stages, few games each
            board, dice = b[g].copy(), int(d[g])
            mine = {int(v): tuple(int(x) for x in np.argwhere(board == v)[0]) for v in np.unique(board) if v > 0}
            if not mine or not (board < 0).any():
                continue
            if dice in mine:
                cube = dice
            else:
                near = [k for k in sorted(mine) if k > dice][:1] + [k for k in sorted(mine, reverse=True) if k < dice][:1]
                cube = near[rng.integers(len(near))]
            i, j = mine[cube]
            legal = [(i + a, j + c) for a, c in DIRS if i + a < S and j + c < S]
            if not legal:
                continue
            ni, nj = legal[rng.integers(len(legal))]
            board[i, j] = 0
            board[ni, nj] = cube
            if (ni, nj) == (S - 1, S - 1) or not (board < 0).any():
                continue   # the agent has won: no search
            out.append((board, int(rng.integers(1, 7))))
        env.step(env.sample_legal_actions(t))
    return out


LAYOUTS = collections.OrderedDict((
    ("linear  rank[(ix<<6)|iy], 128-B rows", lambda ix, iy: (ix << 7) + (iy << 1)),
    ("padded  132-B rows (33 dwords)", lambda ix, iy: ix * 132 + (iy << 1)),
    ("xor     column ^ (2*ix & 63)", lambda ix, iy: (ix << 7) + ((iy ^ ((ix << 1) & 63)) << 1)),
    ("xor-lvl column ^ (level of ix << 1)", lambda ix, iy: (ix << 7) + ((iy ^ ((ix >> 3) << 1)) << 1)),
    ("transposed rank[(iy<<6)|ix]", lambda ix, iy: (iy << 7) + (ix << 1)),
))


LV2_ROWS = (68, 76, 128, 132, 140)   # bytes per row of the fused level table: 33 entries need 66


LEAF_ROWS = (39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50)   # entries per row of the fused leaf table: 39 x 39 entries are used
# the four lane groups of a 128-bit read, as lane numbers inside the wave
B128_GROUPS = [[l + h for l in g] for h in (0, 32) for g in (list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                                                            list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)))]


def half_cycles(addrs, gran, banks):
    """LDS cycles of one 32-lane half: the largest number of distinct `gran`-byte units on one bank"""
    per = collections.defaultdict(set)
    for a in addrs:
        per[(a // 4) % banks].add(a // gran)
    return max(len(v) for v in per.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--waves", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lv2", action="store_true", help="also model the fused level table's read, per candidate row stride")
    ap.add_argument("--leaf", action="store_true", help="also model the fused leaf table's 128-bit read, per candidate row stride")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    rank = rank_lookup()
    tasks = []
    pos = positions(a.lanes, a.steps, rng)
    for board, dice in pos:
        tasks += search_tasks(board, dice)
    print("%d positions, %d search tasks, %d modelled waves of 32 tasks" % (len(pos), len(tasks), a.waves))
    iys = collections.Counter(r[1] for t in tasks for root in t for sub in root for r in sub if not r[2])
    print("distinct iy among the un-steered reads: %d; distinct (iy / 2) %% 32 banks: %d" % (len(iys), len({(y // 2) % 32 for y in iys})))
    res = {name: [0, 0] for name in LAYOUTS}
    val = [0, 0]
    lv2 = {row: [0, 0] for row in LV2_ROWS}
    leaf = {row: [0, 0] for row in LEAF_ROWS}
    for _ in range(a.waves):
        wave = [tasks[i] for i in rng.integers(len(tasks), size=32)]
        for r in range(3):
            for ii in range(3):
                ranks = [[[int(rank[x, y]) for (x, y, _, _, _) in wave[g][r][sub][3 * ii:3 * ii + 3]] for sub in range(2)] for g in range(32)]
                for d in range(3):
                    if a.leaf:   # lane 2 g + sub reads the leaf of task g
                        for row in LEAF_ROWS:
                            for grp in B128_GROUPS:
                                rd = [wave[l // 2][r][l % 2][3 * ii + d] for l in grp]
                                leaf[row][0] += half_cycles([16 * (x * row + y) for (x, y, _, _, _) in rd], 16, 64)
                                leaf[row][1] += 1
                    for half in range(2):
                        reads = [wave[g][r][sub][3 * ii + d] for g in range(16 * half, 16 * half + 16) for sub in range(2)]
                        for name, f in LAYOUTS.items():
                            res[name][0] += half_cycles([f(x, y) for (x, y, _, _, _) in reads], 4, 32)
                            res[name][1] += 1
                        if a.lv2:
                            for row in LV2_ROWS:
                                lv2[row][0] += half_cycles([(zp + 1) * row + (zn + 1) * 2 for (_, _, _, zp, zn) in reads], 4, 32)
                                lv2[row][1] += 1
                        # the value read that belongs to this rank read: prefix minimum over directions 0..d
                        va = [8192 + min(ranks[g][sub][:d + 1]) for g in range(16 * half, 16 * half + 16) for sub in range(2)]
                        val[0] += half_cycles(va, 8, 64)
                        val[1] += 1
    print("%-44s %s  %s" % ("rank[] read, layout", "cycles per half-wave read", "extra cycles per wave instruction"))
    for name, (c, n) in res.items():
        print("%-44s %25.3f  %33.3f" % (name, c / n, 2 * (c / n - 1)))
    print("%-44s %25.3f  %33.3f" % ("val[] read (64-bit, by rank)", val[0] / val[1], 2 * (val[0] / val[1] - 1)))
    for row, (c, n) in lv2.items():
        if n:
            print("%-44s %25.3f  %33.3f" % ("lv2[zP][zN] read, %d-B rows (%d dwords)" % (row, row // 4), c / n, 2 * (c / n - 1)))
    if a.leaf:
        print("%-44s %s  %s" % ("leaf[][] read, layout", "  cycles per 16-lane group", "      cycles per wave instruction"))
    for row, (c, n) in leaf.items():
        if n:
            print("%-44s %25.3f  %33.3f" % ("leaf[ix][iy] read (128-bit), %d-entry rows" % row, c / n, 4 * c / n))


if __name__ == "__main__":
    main()
