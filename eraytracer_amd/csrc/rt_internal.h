// rt_internal.h — entry points shared between the library's translation units (not part of
// the C ABI in include/rt_mi355x.h).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>

#include <optional>

#include "../../include/rt_mi355x.h"
#include "rt_format.h"
#include "rt_shard.h"

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

// The caller's options block with every default filled in: fields past the caller's struct_size
// (or all of them, for a null pointer or struct_size 0) are zero, then row_block 0 -> 16,
// ndev 0 -> 1, spp 0 or cut off by struct_size (ABI 1 callers) -> 1, max_value 0 -> 255.  out gets
// the full struct_size, so it can be handed on as an options block of its own.
inline void rt_opts_load(const rt_opts *in, rt_opts *out) {
    memset(out, 0, sizeof *out);
    const size_t n = in ? in->struct_size : 0;
    if (n) memcpy(out, in, n < sizeof *out ? n : sizeof *out);
    out->struct_size = sizeof *out;
    if (out->row_block == 0) out->row_block = 16;
    if (out->ndev == 0) out->ndev = 1;
    if (n < offsetof(rt_opts, spp) + sizeof out->spp || out->spp == 0) out->spp = 1;
    if (out->max_value == 0) out->max_value = 255;
}

// What one launch renders: the window `win` of an img_w x img_h image, as shard `shard` of
// `nshards` interleaved in blocks of row_block rows.  The slab, its rows, the tiles and every
// buffer are sized on the window; the image and the window's origin only place the rays.
struct rt_frame {
    uint32_t img_w, img_h;
    rt_window win;
    uint32_t depth, row_block, shard, nshards;
    int precision, order;
    uint32_t spp;
    uint64_t seed;
    uint32_t slab_rows() const { return rt_shard_slab_rows(win.h, row_block, nshards); }
    // the slab rows inside the window, a prefix of the slab
    uint32_t valid_rows() const { return rt_shard_valid_rows(win.h, row_block, shard, nshards); }
};
// The frame an options block asks for, as its single shard in binary64 (rt_render fills in its
// own shards and precision).
inline rt_frame rt_opts_frame(const rt_opts &o, uint32_t img_w, uint32_t img_h, const rt_window &win, uint32_t depth) {
    rt_frame f = {};
    f.img_w = img_w;
    f.img_h = img_h;
    f.win = win;
    f.depth = depth;
    f.row_block = o.row_block;
    f.shard = 0;
    f.nshards = 1;
    f.precision = RT_OUT_F64;
    f.order = o.order;
    f.spp = o.spp;
    f.seed = o.seed;
    return f;
}
// The size, shard and window checks of every launch (rt_render.hip): RT_OK, RT_DONE (an image, a
// window and an origin that are all zero) or an error; nothing is dereferenced, no HIP call is made.
int rt_frame_check(const rt_frame &f);

// Slab rows [row_begin, min(row_end, slab rows)) of frame f (rt_render.hip): the boundary renders a
// frame in row bands.  row_begin must be a multiple of 16 (the tile height); d_out / d_levels point
// at slab row 0.
// levels_hit: d_levels gets the primary-hit mask (1 / 0) instead of the level count (RT_LEVELS_HIT).
int rt_launch_rows(rt_prepared *p, const rt_frame &f, uint32_t row_begin, uint32_t row_end, void *d_out,
                   uint8_t *d_levels, void *stream, int levels_hit);

// Async copy of slab rows [b0, b1) of shard m (a slab of row pitch rowbytes) to their rows of a
// row-major image, on `st` (rt_host.hip; rt_unshard's and rt_render's scatter).  With several
// shards the whole row blocks go as one strided copy and the partial block at the bottom of the
// image as a second one; one shard's rows are the image's, one contiguous copy.
int rt_scatter_rows_async(const char *slab, uint32_t b0, uint32_t b1, uint32_t rowbytes, const rt_shard_map &m,
                          char *image, hipMemcpyKind kind, hipStream_t st);

struct DevGuard { // make `dev` the current device; restore the caller's on scope exit
    int prev = -1;
    bool ok = true; // dev could be selected
    DevGuard() { // only save and restore: the scope selects devices itself
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    explicit DevGuard(int dev) : DevGuard() { ok = hipSetDevice(dev) == hipSuccess; }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Replace the scene of a prepared context in place (its work space, streams and events are
// kept; captured frame graphs are invalidated).  No launch of p may be in flight.
int rt_prepare_scene(rt_prepared *p, const rt_elem *scene, uint32_t n);

// What a unit other than rt_render.hip needs of a prepared context to launch a kernel on its scene
// (rt_attrs.hip): the device, the header the kernels get (the filters off when RT_CFG_CULL is 0), the
// scene tables and elem_of[compact object id] = the object's index in the caller's rt_elem array,
// all device memory owned by p and replaced by rt_update_scene; and (rt_query.hip) canon_of[index in
// the caller's array] = the index of that element's canonical (first exactly equal) element, -1 for
// an element that is not an object, n_elems entries.
namespace rtl {
struct SceneHdr;
}
struct rt_scene_view {
    int device;
    const rtl::SceneHdr *hdr;
    const double *tab;
    const int *itab;
    const int *elem_of;
    const int *canon_of;
    int n_elems;
};
rt_scene_view rt_prepared_scene(const rt_prepared *p);

// The caller's hit-attribute planes as the kernels take them (rt_planes.inc); a null pointer is a
// plane not wanted.
struct HitPlanes {
    int *elem;
    void *t, *point, *normal, *albedo;
};
// The plane checks of rt_launch_attrs and rt_query_rays, in this order: the struct's size, at least
// one plane, the precision — *precision is -1 until these have passed — and every plane aligned to
// its element.  RT_OK (and *out filled) or RT_EBADARG.  Calls nothing.
inline int rt_hit_planes(const rt_attr_planes *planes, HitPlanes *out, int *precision) {
    *precision = -1;
    if (planes->struct_size < offsetof(rt_attr_planes, d_albedo) + sizeof(planes->d_albedo)) return RT_EBADARG;
    const rt_attr_planes pl = *planes;
    if (!pl.d_elem && !pl.d_t && !pl.d_point && !pl.d_normal && !pl.d_albedo) return RT_EBADARG;
    if (!rt_is_float(pl.precision)) return RT_EBADARG;
    *precision = pl.precision;
    const uintptr_t esz = rt_elem_size(pl.precision);
    if ((uintptr_t)pl.d_elem % 4) return RT_EBADARG;
    for (const void *f : {pl.d_t, pl.d_point, pl.d_normal, pl.d_albedo})
        if ((uintptr_t)f % esz) return RT_EBADARG;
    *out = HitPlanes{pl.d_elem, pl.d_t, pl.d_point, pl.d_normal, pl.d_albedo};
    return RT_OK;
}

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

// ---- the two file writers' frame (rt_host.hip; rt_render_ppm_file, rt_render_rawppm_file) ----
// The window an options block selects, rendered in binary64 into buffer 0 of its one device's
// context, on the context's stream.  On scope exit the stream is synchronised, the context
// released and the caller's device restored.
struct rt_file_frame {
    rt_opts o;        // the caller's options, loaded (rt_opts_load)
    rt_window win;    // the file is the window's
    rt_ctx *ctx = nullptr; // null after rt_file_render: several devices (o.ndev != 1), nothing rendered
    hipStream_t st = nullptr;
    void *d_rgb = nullptr;
    std::optional<DevGuard> dev; // (not copyable, so neither is the frame)
    ~rt_file_frame() {
        if (!ctx) return;
        (void)hipStreamSynchronize(st);
        rt_ctx_release(ctx);
    }
    size_t values() const { return (size_t)win.w * win.h * 3; }
    void fill(rt_stats *stats) const { // what a writer that rendered here reports
        if (!stats) return;
        stats->pixels = (uint64_t)win.w * win.h;
        stats->ndev = 1;
    }
};
// The writers' checks, in this order: the path; both sizes zero (RT_DONE) or one; value_rc, the
// writer's verdict on its own arguments (RT_OK to go on); the window.  Then, for one device
// (o.ndev == 1): the device count and first_dev (RT_ENODEV), the context, and the launch.  With
// several devices it returns RT_OK with ff->ctx null: the writer goes through rt_render.
int rt_file_render(rt_file_frame *ff, const char *path, int value_rc, const rt_elem *scene, uint32_t n, uint32_t img_w,
                   uint32_t img_h, uint32_t depth, const rt_opts *opts);
