// trace_args_check.cpp — rt_trace_args.h (rt_query_colours' work-space size and argument checks, all
// host-only) swept over (n, depth), the overflow edge of size_t included.  Built with the host
// sanitizers and run by tests/test_trace.py; prints the number of (n, depth) pairs checked.
#include <cstdio>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_trace_args.h"

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "%s:%d: %s (n = %llu, depth = %u)\n", __FILE__, __LINE__, #cond,           \
                         (unsigned long long)n, (unsigned)depth);                                           \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

int main() {
    const uintptr_t A16 = 0x10000; // pointers never dereferenced
    const void *P = (const void *)A16;
    std::vector<uint64_t> ns = {0, 1, 2, 63, 64, 65, 127, 128, 129, 4133, (1u << 21) + 357};
    for (int s = 22; s <= 30; ++s)
        for (int e = -1; e <= 1; ++e) ns.push_back((uint64_t(1) << s) + e);
    for (uint64_t big : {uint64_t(1) << 31, uint64_t(1) << 40, uint64_t(1) << 58, UINT64_MAX - 64, UINT64_MAX - 63, UINT64_MAX})
        ns.push_back(big);
    std::vector<uint32_t> depths = {0, 1, 2, 3, 5, 40, 255, 256, 1000, 65535, 65536};
    // the overflow edge: 76 * 2^30 * depth reaches 2^64 at depth = 2^34 / 76 = 226050910.3
    for (uint32_t d = 226050900; d <= 226050920; ++d) depths.push_back(d);
    for (uint32_t d : {uint32_t(1) << 28, uint32_t(1) << 31, UINT32_MAX - 1, UINT32_MAX}) depths.push_back(d);
    unsigned long long checked = 0;
    for (uint64_t n : ns) {
        size_t prev = 0;
        bool prev_over = false;
        for (uint32_t depth : depths) { // (ascending)
            bool over = false;
            const size_t b = rt_trace_work_bytes(n, depth, &over);
            CHECK(b == rt_trace_work_bytes(n, depth));
            // exact arithmetic: waves * 64 * 76 * depth
            const unsigned __int128 waves = n / 64 + (n % 64 != 0);
            const unsigned __int128 want = waves * 64 * 76 * depth;
            if (n == 0 || depth == 0) {
                CHECK(b == 0 && !over);
            } else if (want > (unsigned __int128)SIZE_MAX) {
                CHECK(b == 0 && over);
            } else {
                CHECK(!over && (unsigned __int128)b == want);
                CHECK((unsigned __int128)b >= (unsigned __int128)n * depth * TRACE_REC_BYTES);
                CHECK(b % 16 == 0);
                CHECK(b >= prev && !prev_over); // monotone in depth until it overflows, never after
            }
            if (n <= RT_MAX_QUERY_RAYS) CHECK(rt_trace_stride(n) == (uint64_t)(waves * 64));
            prev = b;
            prev_over = prev_over || over;
            // the argument checks, in the documented order
            const int good = rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, P, SIZE_MAX);
            if (n > RT_MAX_QUERY_RAYS || over)
                CHECK(good == RT_ETOOBIG);
            else
                CHECK(good == RT_OK);
            CHECK(rt_trace_check_args(nullptr, P, P, n, depth, 0, RT_OUT_F64, P, P, SIZE_MAX) == RT_EBADARG);
            CHECK(rt_trace_check_args(P, P, P, n, depth, 2, RT_OUT_F64, P, P, SIZE_MAX) == RT_EBADARG);
            CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_U8, P, P, SIZE_MAX) == RT_EBADARG);
            CHECK(rt_trace_check_args(P, P, P, n, depth, 1, RT_OUT_F32, (const void *)(A16 + 4), P, SIZE_MAX) == good);
            CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, (const void *)(A16 + 4), P, SIZE_MAX) == RT_EBADARG);
            if (n > RT_MAX_QUERY_RAYS) { // the work space is not looked at
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, nullptr, 0) == RT_ETOOBIG);
            } else if (b) {
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, P, b) == RT_OK);
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, P, b - 1) == RT_EBADARG);
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, nullptr, b) == RT_EBADARG);
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, (const void *)(A16 + 8), b) == RT_EBADARG);
            } else {
                CHECK(rt_trace_check_args(P, P, P, n, depth, 0, RT_OUT_F64, P, nullptr, 0) == good);
            }
            ++checked;
        }
    }
    // monotone in n at every depth that does not overflow
    for (uint32_t depth : depths) {
        size_t prev = 0;
        for (uint64_t n = 0; n <= 1000; ++n) {
            const size_t b = rt_trace_work_bytes(n, depth);
            CHECK(b >= prev);
            prev = b;
        }
    }
    std::printf("%llu\n", checked);
    return 0;
}
