// Host program of tests/test_phantom_reply_tables_cpu.py: runs slot_tabs_build (ewn_gym_amd/csrc/ewn_movetab.hpp, __host__ as well
// as __device__) over every table image of one board size, in both forms, and writes what it built.  No GPU call is made.
//
//   phantom_tables_host S OUT
//
// OUT: a header of ten int32 { S, images, image bytes, sizeof(ReplyEnt<S, true>), sizeof(ReplyEnt<S>), offsetof lvl, offsetof m10,
// mask bytes, sizeof(FastTab<S>), 0 } and then, per image (the order of ewn_build_tables: 'hybrid', 'min_dist', 'attk', 'two_min_dist' x two variants):
//   the image as build_fast_tables made it | the block's copy after slot_tabs_build<S, true> | its 128 phantom reply entries |
//   the 128 reply entries of slot_tabs_build<S, false>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ewn_movetab.hpp"

template <int S, bool PH> static void derive(std::vector<int8_t> &img, std::vector<int8_t> &rep)
{
    typedef SlotTabGeo<S, PH> G;
    std::vector<int8_t> extra((size_t)G::EXTRA + 16);
    int8_t *ex = extra.data() + ((16 - (uintptr_t)extra.data() % 16) % 16);
    SlotTabs<S, PH> D;
    D.rep = (const ReplyEnt<S, PH> *)ex;
    D.mvp = (const MoveEnt *)(ex + G::REPLY_BYTES);
    D.mvn = G::MOVEN_IN_PAD ? (const MoveEnt *)(img.data() + sizeof(FastTab<S>)) : (const MoveEnt *)(ex + G::REPLY_BYTES + G::MOVE_BYTES);
    for (int e = 0; e < 256; e++) slot_tabs_build<S, PH>((const FastTab<S> *)img.data(), D, e);
    rep.assign(ex, ex + G::REPLY_BYTES);
}

template <int S> static int run(const char *path)
{
    static const int heur_of_image[FAST_HEUR_IMAGES] = { 0, 1, 3, 2 };
    FILE *f = fopen(path, "wb");
    if (!f) return 2;
    const int32_t hdr[10] = { S, 2 * FAST_HEUR_IMAGES, FAST_TAB_BYTES(S), (int32_t)sizeof(ReplyEnt<S, true>), (int32_t)sizeof(ReplyEnt<S>),
                             (int32_t)offsetof(FastTab<S>, lvl), (int32_t)offsetof(FastTab<S>, m10), (int32_t)sizeof(typename MaskOf<S>::type),
                              (int32_t)sizeof(FastTab<S>), 0 };
    fwrite(hdr, sizeof(hdr), 1, f);
    for (int hi = 0; hi < FAST_HEUR_IMAGES; hi++)
        for (int variant = 0; variant < 2; variant++) {
            std::vector<int8_t> img((size_t)FAST_TAB_BYTES(S), 0), rep;
            if (build_fast_tables<S>((FastTab<S> *)img.data(), variant, heur_of_image[hi]) != 0) return 3;
            fwrite(img.data(), img.size(), 1, f);
            std::vector<int8_t> plain = img;            // the move table in the padding is written into the copy, as in the kernel
            derive<S, true>(img, rep);
            fwrite(img.data(), img.size(), 1, f);
            fwrite(rep.data(), rep.size(), 1, f);
            derive<S, false>(plain, rep);
            fwrite(rep.data(), rep.size(), 1, f);
        }
    return fclose(f) == 0 ? 0 : 4;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    const int S = atoi(argv[1]);
    if (S == 5) return run<5>(argv[2]);
    if (S == 6) return run<6>(argv[2]);
    return 1;
}
