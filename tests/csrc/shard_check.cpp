// shard_check.cpp — rt_shard.h against the definition of the shard interleave, on every small
// geometry: H in 1..70, row blocks {1, 2, 3, 5, 16, 17}, 1..5 shards, every shard.  Built with the
// host sanitizers and run by tests/test_host.py; prints the number of geometries checked.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_shard.h"

// The definition: the slab's blocks one by one, each clipped to the image.
static size_t valid_by_blocks(int H, int rb, int sh, int ns) {
    const size_t slab = rt_shard_slab_rows((uint32_t)H, (uint32_t)rb, (uint32_t)ns);
    size_t v = 0;
    for (size_t blk = 0; blk * rb < slab; ++blk) {
        const long long base = ((long long)blk * ns + sh) * rb;
        v += (size_t)std::max(0LL, std::min((long long)rb, (long long)H - base));
    }
    return v;
}

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "H=%d rb=%d ns=%d shard=%d: %s\n", H, rb, ns, sh, #cond);                  \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

int main() {
    const int blocks[] = {1, 2, 3, 5, 16, 17};
    long checked = 0;
    for (int H = 1; H <= 70; ++H)
        for (int rb : blocks)
            for (int ns = 1; ns <= 5; ++ns) {
                std::vector<int> hits(H, 0);
                const uint32_t slab = rt_shard_slab_rows((uint32_t)H, (uint32_t)rb, (uint32_t)ns);
                int sh = -1;
                CHECK(slab % rb == 0 && (uint64_t)slab * ns >= (uint64_t)H && (uint64_t)(slab - rb) * ns < (uint64_t)H);
                for (sh = 0; sh < ns; ++sh) {
                    const rt_shard_map m = {(uint32_t)H, (uint32_t)rb, (uint32_t)sh, (uint32_t)ns};
                    const uint32_t valid = rt_shard_valid_rows((uint32_t)H, (uint32_t)rb, (uint32_t)sh, (uint32_t)ns);
                    CHECK(valid == valid_by_blocks(H, rb, sh, ns));
                    CHECK(valid == rt_shard_valid_rows(m) && valid <= slab);
                    for (uint32_t r = 0; r < slab; ++r) {
                        const uint64_t g = rt_shard_image_row(r, (uint32_t)rb, (uint32_t)sh, (uint32_t)ns);
                        CHECK(g == rt_shard_image_row(m, r));
                        CHECK((g < (uint64_t)H) == (r < valid)); // the rows inside the image are a prefix
                        if (g < (uint64_t)H) ++hits[g];
                    }
                    ++checked;
                }
                sh = -1;
                for (int g = 0; g < H; ++g) CHECK(hits[g] == 1); // over all shards, every image row once
            }
    std::printf("%ld\n", checked);
    return 0;
}
