// rt_internal.h — entry points shared between the library's translation units (not part of
// the C ABI in include/rt_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_mi355x.h"

// rt_launch_window restricted to slab rows [row_begin, min(row_end, slab rows)) of the window
// (rt_render.hip): (width, height) is the image, (x0, y0, win_w, win_h) the window, on which the
// slab, its rows and the buffers are sized.  row_begin must be a multiple of 16 (the tile height);
// d_out / d_levels point at slab row 0.
// levels_hit: d_levels gets the primary-hit mask (1 / 0) instead of the level count (RT_LEVELS_HIT).
int rt_launch_rows(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                   uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, int precision,
                   int order, uint32_t spp, uint64_t seed, uint32_t row_begin, uint32_t row_end, void *d_out,
                   uint8_t *d_levels, void *stream, int levels_hit = 0);

// The window an options block selects in a width x height image (o: the boundary's own copy, zero
// past the caller's struct_size): win_w = win_h = 0 is the whole frame.  RT_EBADARG for exactly one
// zero size, an origin with a zero size, or a window that leaves the image.  Calls nothing.
struct rt_window {
    uint32_t x0, y0, w, h;
};
inline int rt_opts_window(const rt_opts &o, uint32_t width, uint32_t height, rt_window *win) {
    if (o.win_w == 0 && o.win_h == 0) {
        if (o.win_x0 || o.win_y0) return RT_EBADARG;
        *win = rt_window{0, 0, width, height};
        return RT_OK;
    }
    if (o.win_w == 0 || o.win_h == 0) return RT_EBADARG;
    if ((uint64_t)o.win_x0 + o.win_w > width || (uint64_t)o.win_y0 + o.win_h > height) return RT_EBADARG;
    *win = rt_window{o.win_x0, o.win_y0, o.win_w, o.win_h};
    return RT_OK;
}

// Replace the scene of a prepared context in place (its work space, streams and events are
// kept; captured frame graphs are invalidated).  No launch of p may be in flight.
int rt_prepare_scene(rt_prepared *p, const rt_elem *scene, uint32_t n);

// Free p's wavefront work space (queues, colours, flags, lists, supersampling sums, primary
// masks: GBs at 4096^2); the next launch grows it again.  No launch of p may be in flight.
// Returns the bytes freed.
size_t rt_trim(rt_prepared *p);

// ---- the process's render contexts (rt_host.hip) ------------------------------------------
// One context = one device, two streams (render, copy), the most recently prepared scene with
// its grown work space, grown device output buffers and a pinned host staging buffer.  The
// pool keeps them across calls (one lazily initialised context per process;
// up to RT_CTX_PER_DEVICE concurrent callers per device get one each).
struct rt_ctx;
// Take a free context of `device` with `scene` prepared on it (compiled and uploaded only when
// it differs from the context's last scene).  Blocks while every context of the device is busy.
int rt_ctx_acquire(int device, const rt_elem *scene, uint32_t n, rt_ctx **out);
void rt_ctx_release(rt_ctx *c);
rt_prepared *rt_ctx_prepared(rt_ctx *c);
hipStream_t rt_ctx_stream(rt_ctx *c);
// Device buffer `which` (0..2) of at least `bytes`, kept (and grown) with the context.
// 0: the float frame, 1: the levels, 2: the P3 text or the integer frame.
int rt_ctx_device_buffer(rt_ctx *c, int which, size_t bytes, void **out);
// The context's counter of values an integer frame stored as 0 (rt_quantize's d_clamped): 8 bytes
// of device memory, created on first use; the caller zeroes it on its stream.
int rt_ctx_clamped(rt_ctx *c, uint64_t **out);
// Pinned host staging buffer of at least `bytes`, kept with the context.
int rt_ctx_host_buffer(rt_ctx *c, size_t bytes, void **out);
