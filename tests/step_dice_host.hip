// Host program of tests/test_step_dice_cpu.py: LaneRng::step_dice (ewn_gym_amd/csrc/ewn_core.hpp, __host__ as well as __device__), the
// two dice of an env step drawn at once from the step's primed Philox block, against two randint(1, 7) on a copy of the same stream.
// No GPU call is made.
//
//   step_dice_host
//
// Prints one line per group of cases, "<group> cases <n> cold <c> shifted <s> crossed <x>": how many of the n streams left the
// straight path (a low half below 6), had a second draw that did not sit right behind the first or a position past n + 2 (a
// rejection), and ended in another block than they started in.  The first mismatch is printed and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include "ewn_core.hpp"

static u64 sm_state = 0x9E3779B97F4A7C15ull;
static u32 rnd32()   // splitmix64, upper half
{
    u64 z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (u32)((z ^ (z >> 31)) >> 32);
}

// the six words w with (u32)(w * 6) < 6: w = ceil(k * 2^32 / 6)
static u32 edge_word(int k) { return (u32)((((u64)k << 32) + 5u) / 6u); }

struct Tally { long cases, cold, shifted, crossed; };

// a stream at the start of a step: aligned to a block boundary, the block in registers -- Philox's own, or `inject`
static LaneRng stream(u32 seed, u32 wraps, u32 n, u64 key, const u32 *inject)
{
    LaneRng r;
    r.load(1, make_uint4(seed, n, seed + 1u, wraps), nullptr, 0u, key);
    r.begin_step();
    r.ps.prime();
    if (inject) { r.ps.b0 = inject[0]; r.ps.b1 = inject[1]; r.ps.b2 = inject[2]; r.ps.b3 = inject[3]; }
    return r;
}

static void check(const char *what, LaneRng r, Tally &t)
{
    LaneRng g = r;
    const int d1 = g.randint(1, 7); const u32 n1 = g.ps.n;
    const int d2 = g.randint(1, 7); const u32 n2 = g.ps.n;
    const u32 n0 = r.ps.n;
    const bool cold = (u32)((u64)r.ps.b0 * 6u) < 6u || (u32)((u64)r.ps.b1 * 6u) < 6u;
    const LaneRng::StepDice o = r.step_dice();
    if (o.d1 != d1 || o.n1 != n1 || o.d2 != d2 || o.n2 != n2 || r.ps.n != n0 || r.ps.have != 0u || d1 < 1 || d1 > 6 || d2 < 1 || d2 > 6) {
        printf("MISMATCH %s: block %08x %08x %08x %08x n %u: step_dice (%d, %u, %d, %u) randint (%d, %u, %d, %u) n after %u have %u\n", what,
               g.ps.b0, g.ps.b1, g.ps.b2, g.ps.b3, n0, o.d1, o.n1, o.d2, o.n2, d1, n1, d2, n2, r.ps.n, r.ps.have);
        exit(1);
    }
    t.cases++; t.cold += cold; t.shifted += n1 != n0 + 1u || n2 != n0 + 2u; t.crossed += (n2 - 1u) >> 2 != n0 >> 2;
}

static void report(const char *group, const Tally &t) { printf("%s cases %ld cold %ld shifted %ld crossed %ld\n", group, t.cases, t.cold, t.shifted, t.crossed); }

int main()
{
    for (int k = 0; k < 6; k++) if ((u32)(edge_word(k) * 6u) >= 6u || (k && (u32)((edge_word(k) - 1u) * 6u) < 6u)) { printf("edge word %d\n", k); return 1; }
    {   // the stream's own blocks, as a kernel meets them: a few thousand (seed, wraps, position, key)
        Tally t = {};
        for (int i = 0; i < 4096; i++) check("philox", stream(rnd32(), rnd32() & 3u, (rnd32() % 200u), ((u64)rnd32() << 32) | rnd32(), nullptr), t);
        report("philox", t);
    }
    {   // injected random blocks
        Tally t = {};
        for (int i = 0; i < 4096; i++) { const u32 b[4] = { rnd32(), rnd32(), rnd32(), rnd32() }; check("random", stream(rnd32(), 0u, 4u * (rnd32() % 50u), 2024u, b), t); }
        report("random", t);
    }
    {   // the six edge words in b0, in b1, in both; the words behind them ordinary
        Tally t0 = {}, t1 = {}, t01 = {};
        for (int rep = 0; rep < 8; rep++)
            for (int i = 0; i < 6; i++) {
                const u32 a[4] = { edge_word(i), rnd32(), rnd32(), rnd32() }; check("edge b0", stream(rnd32(), 0u, 8u, 7u, a), t0);
                const u32 b[4] = { rnd32(), edge_word(i), rnd32(), rnd32() }; check("edge b1", stream(rnd32(), 0u, 8u, 7u, b), t1);
                for (int j = 0; j < 6; j++) { const u32 c[4] = { edge_word(i), edge_word(j), rnd32(), rnd32() }; check("edge b0 b1", stream(rnd32(), 0u, 8u, 7u, c), t01); }
            }
        report("edge_b0", t0); report("edge_b1", t1); report("edge_b0_b1", t01);
    }
    {   // rejections up to the block's last word: the generic path goes on into the next block (words that reject: k = 0, 1, 3, 4)
        Tally t = {};
        static const int rej[4] = { 0, 1, 3, 4 };
        for (int first = 0; first < 4; first++)        // ordinary words in front of the rejecting ones: none, b0, b0 b1, b0 b1 b2
            for (int i = 0; i < 4; i++)
                for (int rep = 0; rep < 4; rep++) {
                    u32 b[4];
                    for (int w = 0; w < 4; w++) b[w] = w < first ? rnd32() : edge_word(rej[(i + w) & 3]);
                    check("last word", stream(rnd32(), rnd32() & 1u, 4u * (rnd32() % 50u), ((u64)rnd32() << 32) | 5u, b), t);
                }
        report("last_word", t);
    }
    return 0;
}
