// rt_trace_args.h — the host-only part of rt_query_colours (RT_QUERY in include/rt_mi355x.h): the
// layout and size of its work space and its argument checks.  No HIP call, nothing dereferenced, so
// tests/csrc/trace_args_check.cpp runs it under the host sanitizers.
//
// The work space holds one record per ray and reflection level, as planes: [level][field][ray], the
// ray stride padded to the wave (64), so that every load and store of a wave covers contiguous
// memory and a level's slice is touched only by waves that reach it.  The fields of a level, in this
// order: nine binary64 planes — the direction the ray arrived with, the hit point, the normal — and
// one int32 plane, the compact id of the object hit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_mi355x.h"
#include "rt_format.h"

constexpr uint64_t TRACE_WAVE = 64;
constexpr uint64_t TRACE_REC_DOUBLES = 9;                      // direction, hit point, normal
constexpr uint64_t TRACE_REC_BYTES = TRACE_REC_DOUBLES * 8 + 4; // and the object id: 76
constexpr size_t TRACE_WORK_ALIGN = 16;

// Rays per plane: n rounded up to whole waves (n <= RT_MAX_QUERY_RAYS: no overflow).
inline uint64_t rt_trace_stride(uint64_t n) { return (n + TRACE_WAVE - 1) / TRACE_WAVE * TRACE_WAVE; }

// The bytes rt_query_colours needs for n rays at `depth`: 0 for depth 0 or n = 0, and 0 where the
// size does not fit size_t (*overflow set; the pointer may be null).
inline size_t rt_trace_work_bytes(uint64_t n, uint32_t depth, bool *overflow = nullptr) {
    if (overflow) *overflow = false;
    if (n == 0 || depth == 0) return 0;
    // n64 = the stride, computed so that n near 2^64 cannot wrap
    const uint64_t waves = n / TRACE_WAVE + (n % TRACE_WAVE != 0);
    unsigned __int128 bytes = (unsigned __int128)waves * TRACE_WAVE;
    bytes *= TRACE_REC_BYTES;
    bytes *= depth;
    if (bytes > (unsigned __int128)SIZE_MAX) {
        if (overflow) *overflow = true;
        return 0;
    }
    return (size_t)bytes;
}

// rt_query_colours' checks, in the documented order: RT_EBADARG before RT_ETOOBIG.  RT_OK: launch (or
// nothing to do: n = 0, or depth 0, which only stores zeros).
inline int rt_trace_check_args(const void *p, const void *d_origin, const void *d_dir, uint64_t n, uint32_t depth,
                               uint32_t flags, int precision, const void *d_rgb, const void *d_work, size_t work_bytes) {
    if (!p || !d_origin || !d_dir || !d_rgb) return RT_EBADARG;
    if (flags & ~(uint32_t)RT_QUERY_ONE_ORIGIN) return RT_EBADARG;
    if (!rt_is_float(precision)) return RT_EBADARG;
    if ((uintptr_t)d_origin % 8 || (uintptr_t)d_dir % 8) return RT_EBADARG;
    if ((uintptr_t)d_rgb % rt_elem_size(precision)) return RT_EBADARG;
    bool overflow = false;
    // (a batch above the limit is RT_ETOOBIG below: its size is not asked of the caller)
    const size_t need = n > RT_MAX_QUERY_RAYS ? 0 : rt_trace_work_bytes(n, depth, &overflow);
    if (need && (!d_work || (uintptr_t)d_work % TRACE_WORK_ALIGN || work_bytes < need)) return RT_EBADARG;
    if (n > RT_MAX_QUERY_RAYS || overflow) return RT_ETOOBIG;
    return RT_OK;
}
