// band_check.cpp — rt_bands.h (how rt_render cuts a frame into shards per device and row bands) on
// every small geometry: heights 1..200, row blocks {1, 2, 3, 5, 16, 17, 48}, 1..64 shards over
// 1..min(shards, 8) devices, rows of {3, 24, 3 * 2^20, 24 * 2^20} bytes, bands of 1 and 24 MiB.
// Built with the host sanitizers and run by tests/test_host.py; prints the number of geometries
// checked.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_bands.h"

// The specification: rt_render's band arithmetic as it stood inline in rt_host.hip before
// rt_bands.h, restated (64 was its MAX_BANDS).
struct Spec {
    uint32_t slab, per_dev, band, nb;
};
static uint32_t spec_lcm(uint32_t a, uint32_t b) {
    uint32_t x = a, y = b;
    while (y) {
        const uint32_t t = x % y;
        x = y;
        y = t;
    }
    return a / x * b;
}
static Spec spec(uint32_t height, uint32_t rb, uint32_t ns, uint32_t nd, uint32_t rowbytes, size_t band_bytes) {
    const uint64_t span = (uint64_t)rb * ns;
    const uint32_t slab = (uint32_t)((height + span - 1) / span * rb);
    const uint32_t per_dev = (ns + nd - 1) / nd;
    const uint32_t max_nb = std::max<uint32_t>(1, 64 / per_dev);
    const uint32_t gran = spec_lcm(rb, 16);
    uint32_t band = (uint32_t)std::max<size_t>(1, band_bytes / rowbytes) / gran * gran;
    band = std::max(band, gran);
    if ((slab + band - 1) / band > max_nb) band = ((slab + max_nb - 1) / max_nb + gran - 1) / gran * gran;
    const uint32_t nb = (slab + band - 1) / band;
    return Spec{slab, per_dev, band, nb};
}

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "H=%u rb=%u ns=%u nd=%u rowbytes=%u band_bytes=%zu: %s\n", H, rb, ns, nd,  \
                         rowbytes, target, #cond);                                                          \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

int main() {
    const uint32_t blocks[] = {1, 2, 3, 5, 16, 17, 48};
    const uint32_t rows[] = {3, 24, 3u << 20, 24u << 20};
    const size_t targets[] = {(size_t)1 << 20, (size_t)24 << 20};
    long checked = 0;
    for (uint32_t H = 1; H <= 200; ++H)
        for (uint32_t rb : blocks)
            for (uint32_t ns = 1; ns <= 64; ++ns)
                for (uint32_t nd = 1; nd <= std::min<uint32_t>(ns, 8); ++nd)
                    for (uint32_t rowbytes : rows)
                        for (size_t target : targets) {
                            const rt_bands p = rt_band_plan(H, rb, ns, nd, rowbytes, target);
                            const uint32_t gran = spec_lcm(rb, 16);
                            CHECK(p.band > 0 && p.band % gran == 0);
                            CHECK((uint64_t)(p.nb - 1) * p.band < p.slab && p.slab <= (uint64_t)p.nb * p.band);
                            CHECK(p.row0(0) == 0 && p.row1(p.nb - 1) == p.slab && p.row0(p.nb - 1) < p.slab);
                            CHECK(p.nb == 1 || p.row1(0) == p.band);
                            CHECK(p.per_dev * p.nb <= (uint32_t)MAX_BANDS);
                            // the shards of the devices (d, d + nd, ...) partition 0..ns-1, none has more
                            // than per_dev, and every band event lies inside the contexts' arrays
                            std::vector<int> hits(ns, 0);
                            for (uint32_t d = 0; d < nd; ++d) {
                                const uint32_t k = p.shards_of(d);
                                CHECK(k >= 1 && k <= p.per_dev);
                                CHECK(p.event(k - 1, p.nb - 1) < (uint32_t)MAX_BANDS);
                                for (uint32_t i = 0; i < k; ++i) {
                                    CHECK(d + i * nd < ns);
                                    ++hits[d + i * nd];
                                }
                            }
                            for (uint32_t s = 0; s < ns; ++s) CHECK(hits[s] == 1);
                            const Spec w = spec(H, rb, ns, nd, rowbytes, target);
                            CHECK(p.slab == w.slab && p.per_dev == w.per_dev && p.band == w.band && p.nb == w.nb);
                            for (uint32_t d = 0; d < nd; ++d) CHECK(p.shards_of(d) == (ns - d + nd - 1) / nd);
                            ++checked;
                        }
    std::printf("%ld\n", checked);
    return 0;
}
