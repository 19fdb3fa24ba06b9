// stage_lds_check.cpp — rt_layout.h's stage_lds_place over spheres-only scenes of 1..600 spheres and
// 1..9 lights (n_tri = n_pl = 0, n_obj = n_sph, n_chunk = ceil(n_sph / 64)), with 1 and 16 occluder
// cells, against a literal restatement of the six sections and of the bytes stage_tables (rt_cull.inc)
// copies into each.  Prints "cases staged unstaged" (one-cell cases that were / were not placed); the
// first violation is printed to stderr and ends the run with status 1.  Built with the host sanitizers
// and run by tests/test_stage_lds.py.
#include <cstdio>
#include <initializer_list>

#include "../../eraytracer_amd/csrc/rt_layout.h"

static int fail(const char *what, int n_sph, int n_light, int ncell) {
    std::fprintf(stderr, "%s: n_sph %d n_light %d ncell %d\n", what, n_sph, n_light, ncell);
    return 1;
}

int main() {
    long cases = 0, staged = 0, unstaged = 0;
    for (int n_sph = 1; n_sph <= 600; ++n_sph)
        for (int n_light = 1; n_light <= 9; ++n_light)
            for (int ncell : {1, 16}) {
                rtl::SceneHdr h = {};
                h.n_sph = h.n_obj = n_sph;
                h.n_light = n_light;
                h.n_org = 1 + n_light;
                h.n_chunk = (n_sph + 63) / 64;
                h.l_obj = h.l_meta = h.l_org = h.l_occ = h.l_id = h.l_sphb = h.l_bytes = -7; // all are set, whatever they were
                const long total = rtl::stage_lds_place(h, ncell);
                // what stage_tables copies: 96-byte object rows, 16-byte meta rows, the lights' 32-byte
                // sphere rows, one cell of 8-byte mask words per (light, sphere, chunk), 4-byte ids,
                // 32-byte sphere bounds
                const long copied[6] = {n_sph * 96L, n_sph * 16L, (long)n_light * n_sph * 32, (long)n_light * n_sph * h.n_chunk * 8,
                                        n_sph * 4L, n_sph * 32L};
                // the sections of a layout with ncell cells: the same, the masks ncell times
                long want = 0;
                for (int s = 0; s < 6; ++s) want = (want + copied[s] * (s == 3 ? ncell : 1) + 15) / 16 * 16;
                if (total != want) return fail("total", n_sph, n_light, ncell);
                const int at[7] = {h.l_obj, h.l_meta, h.l_org, h.l_occ, h.l_id, h.l_sphb, h.l_bytes};
                ++cases;
                if (ncell != 1 || total > 32 * 1024) {
                    for (int s = 0; s < 6; ++s)
                        if (at[s] != -1) return fail("an offset of a layout that is not staged", n_sph, n_light, ncell);
                    if (h.l_bytes != 0) return fail("l_bytes of a layout that is not staged", n_sph, n_light, ncell);
                    unstaged += ncell == 1;
                    continue;
                }
                ++staged;
                if (at[0] != 0 || h.l_bytes != total) return fail("start or end", n_sph, n_light, ncell);
                for (int s = 0; s < 6; ++s) {
                    if (at[s] % 16 != 0) return fail("alignment", n_sph, n_light, ncell);
                    if (at[s + 1] < at[s] + copied[s]) return fail("a section shorter than its copy", n_sph, n_light, ncell);
                }
                if (at[6] != (at[5] + copied[5] + 15) / 16 * 16) return fail("l_bytes is not the last section's end", n_sph, n_light, ncell);
            }
    std::printf("%ld %ld %ld\n", cases, staged, unstaged);
    return 0;
}
