/*
 * rt_mi355x.h — C-ABI boundary of the MI355X-native per-pixel render path.
 *
 * This library replaces the pixel loop of the reference ray tracer
 * (plouj/eraytracer, raytracer.erl).  The reference's strategy interface is
 *
 *     F(Width, Height, Scene, Recursion_depth) -> done | [{Key, {R,G,B}}]
 *
 * implemented by raytraced_pixel_list_simple/4      (raytracer.erl:86-99),
 *                raytraced_pixel_list_concurrent/4  (raytracer.erl:101-119),
 *                raytraced_pixel_list_distributed/4 (raytracer.erl:121-149),
 * chosen by tracing_function/1 (raytracer.erl:714-719) and called once by
 * raytrace/5 (raytracer.erl:723-733).  Every pixel runs
 * trace_ray_through_pixel/3 (raytracer.erl:180-184) and the shading /
 * intersection functions below it (raytracer.erl:186-511).
 *
 * The host (an erl_nif shim, a ctypes binding, a C++ program) marshals the
 * scene list (raytracer.erl:618-665 for the default one) into an array of
 * rt_elem records in LIST ORDER, element 0 being the camera, and calls
 * rt_render().  The result is the W*H*3 framebuffer in row-major order, i.e.
 * exactly the {R,G,B} values of the reference's list, in the list's order.
 * The keys are implied: simple uses key 1 for every pixel (raytracer.erl:95),
 * concurrent/distributed use X+Y*Width (raytracer.erl:112,173) and sort by it.
 *
 * All arithmetic is IEEE binary64 in the reference's operation order
 * (Erlang floats are doubles).  No pointer passed in is retained after a call
 * returns.  Every entry point returns 0 (RT_OK), RT_DONE, or a negative RT_E*
 * code; rt_strerror() names it.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 5

/* ---- return codes ------------------------------------------------------- */
#define RT_OK 0
#define RT_DONE 1          /* W = H = 0: the reference returns the atom `done` (raytracer.erl:86,101,121) */
#define RT_EBADARG (-1)    /* malformed scene / sizes: the reference crashes (function_clause, badrecord) */
#define RT_ENODEV (-2)     /* no HIP device, or device index out of range */
#define RT_EHIP (-3)       /* a HIP runtime call failed */
#define RT_ENOMEM (-4)     /* host or device allocation failed */
#define RT_ETOOBIG (-5)    /* a frame size, spp or shard count above its documented limit (RT_MAX_*) */
#define RT_ERANGE (-6)     /* rt_ppm_format: a channel below -2^31 after scaling (see there) */

/* No limit on the recursion depth or on the number of objects or lights: the reference recurses
 * to any depth (pixel_colour_from_ray/3, raytracer.erl:186-203), folds over every light
 * (lighting_function/6, :209-252) and scans any list (nearest_object_intersecting_ray/6,
 * :300-346).  Frames whose work space (per-level hit queues, ~100 bytes per pixel and level, in
 * row passes of at least 16 rows) or scene tables (32-bit offsets: about 16 doubles per
 * (origin, object) pair, the origins being the camera and every light) do not fit fail with
 * RT_ENOMEM.  out_levels saturates at 255. */

/* ---- scene records, mirroring the reference's records (raytracer.erl:72-81) -- */
enum rt_kind {
    RT_CAMERA = 0,      /* #camera{location, rotation, fov, screen}             :76 */
    RT_POINT_LIGHT = 1, /* #point_light{diffuse_colour, location, specular_colour} :81 */
    RT_SPHERE = 2,      /* #sphere{radius, center, material}                    :78 */
    RT_TRIANGLE = 3,    /* #triangle{v1, v2, v3, material}                      :79 */
    RT_PLANE = 4,       /* #plane{normal, distance, material}                   :80 */
    RT_OTHER = 5        /* any other term: ray_object_intersect/2 -> none (:357),
                           lighting_function skips it (:248) */
};

typedef struct rt_vec3 {
    double x, y, z; /* #vector{x, y, z} / #colour{r, g, b} (:72-73) */
} rt_vec3;

typedef struct rt_material { /* #material{colour, specular_power, shininess, reflectivity} (:77) */
    rt_vec3 colour;
    double specular_power;
    double shininess;
    double reflectivity;
} rt_material;

typedef struct rt_elem {
    int32_t kind;  /* enum rt_kind */
    /* canon: index (into this array) of the FIRST element that is exactly equal
     * (=:=, so 4 and 4.0 differ) to this one; shadow_factor/4 (raytracer.erl:
     * 256-267) lights a hit iff the nearest object seen from the light MATCHES
     * the hit object term, so duplicates count as the same object.  Pass -1 to
     * let the library decide by bitwise equality of kind and every field. */
    int32_t canon;
    union {
        struct { rt_vec3 location, rotation; double fov, screen_width, screen_height; } camera;
        struct { rt_vec3 diffuse_colour, location, specular_colour; } point_light;
        struct { double radius; rt_vec3 center; rt_material material; } sphere;
        struct { rt_vec3 v1, v2, v3; rt_material material; } triangle;
        struct { rt_vec3 normal; double distance; rt_material material; } plane;
        double raw[12];
    } u;
} rt_elem;

/* ---- options / statistics ---------------------------------------------------- */
#define RT_OUT_F64 0   /* out_rgb is double[H][W][3] (the reference's values, exact) */
#define RT_OUT_F32 1   /* out_rgb is float[H][W][3]  (the "float3 framebuffer") */
/* Integer frames: every channel is min(trunc(C*max_value), max_value) of the binary64 value C,
 * the rule of write_pixels_to_ppm/5 (raytracer.erl:667-685), so the samples are the integers the
 * P3 file prints.  An unsigned sample cannot hold a negative one: see rt_quantize. */
#define RT_OUT_U8  2   /* uint8_t [H][W][3], max_value 1..255   */
#define RT_OUT_U16 3   /* uint16_t[H][W][3], native endian, max_value 1..65535 */
#define RT_MAX_INT_VALUE 65535

#define RT_ORDER_EXACT 0 /* reflection added once per light, reference fold order (bit-identical colour sums) */
#define RT_ORDER_FAST 1  /* forward-only reassociated accumulation (|delta| ~ 1e-15, same hit decisions) */

typedef struct rt_opts {
    uint32_t struct_size; /* sizeof(rt_opts); 0 or a NULL opts pointer selects every default */
    int32_t first_dev;    /* first HIP device (default 0) */
    int32_t ndev;         /* devices used by rt_render in this process (default 1; -1 = all visible).
                             Test hook: the environment variable RT_DEVICE_ALIAS=N (1..4, read once
                             per process) makes rt_render see N devices that are all first_dev; one
                             call then holds N of the device's 4 contexts, so the hook supports one
                             rt_render caller at a time (concurrent callers with N >= 3 can deadlock) */
    int32_t precision;    /* RT_OUT_F64 (default), RT_OUT_F32, or an integer frame: RT_OUT_U8, RT_OUT_U16 */
    int32_t order;        /* RT_ORDER_EXACT (default) or RT_ORDER_FAST */
    uint32_t row_block;   /* multi-device interleave granularity in rows (default 16) */
    uint8_t *out_levels;  /* optional host W*H bytes: reflection-chain levels that hit, per pixel */
    /* appended in ABI 2 (older callers' smaller struct_size leaves the defaults) */
    uint32_t spp;         /* samples per pixel (default 1 = the reference; see RT_SUPERSAMPLING) */
    uint32_t nshards;     /* rt_render: row shards (default 0 = one per device used); shard s runs on
                             device first_dev + s % ndev, so more shards than devices runs the
                             distributed strategy's split (raytracer.erl:121-149) on fewer GPUs */
    uint64_t seed;        /* jitter seed for spp > 1 */
    /* appended in ABI 4 */
    uint32_t flags;       /* RT_LEVELS_HIT: out_levels gets 1 where the pixel's primary ray hits an
                             object (depth > 0), 0 elsewhere, instead of the chain's level count —
                             all a host needs for the reference's integer {0,0,0} pixels, and it keeps
                             the fused shading kernels that a full level count turns off */
    /* appended after ABI 4's flags (additive: RT_ABI_VERSION stays 5) */
    uint32_t max_value;   /* RT_OUT_U8 / RT_OUT_U16: the samples' MaxValue; 0, or a struct_size that
                             ends before this field, selects 255 */
    /* appended after max_value (additive: RT_ABI_VERSION stays 5) */
    uint32_t win_x0, win_y0, win_w, win_h; /* RT_WINDOW: render only this pixel window of the width x height
                             image.  win_w = win_h = 0, or a struct_size that ends before these fields,
                             selects the whole frame.  RT_EBADARG for exactly one of win_w, win_h zero,
                             for a non-zero origin with a zero size, and for a window that leaves the
                             image; checked before the scene and before any HIP call */
} rt_opts;
#define RT_LEVELS_HIT 1

/* RT_WINDOW — a pixel window of a frame, bit for bit the frame's crop.
 * A window is (x0, y0, win_w, win_h) inside an image of width x height pixels:
 *     win_w, win_h >= 1,  x0 + win_w <= width,  y0 + win_h <= height.
 * Pixel values: window pixel (x, y) IS image pixel (x0+x, y0+y).  Its ray goes through
 *     X = (x0+x)/width,  Y = (y0+y)/height,
 * and with spp > 1 the RT_SUPERSAMPLING index is pixel = (y0+y)*width + (x0+x) in the whole image, so
 * a window's samples are the whole frame's.  A pixel's bits do not depend on which wave traces it
 * (the filters only skip objects that provably cannot be hit; the wave-uniform fast paths of pow,
 * sqrt and division give the library's bits), so a window equals the crop [y0 : y0+win_h,
 * x0 : x0+win_w] of the whole frame in every byte, colours and levels.
 * Buffers: everything else about the call is that of a win_w x win_h frame.  The output is packed,
 * win_h rows of win_w*3 elements; levels are win_w*win_h bytes; rows are dealt to shards by WINDOW
 * row — row g of the window belongs to shard (g / row_block) % nshards — and a slab has
 * rt_shard_rows(win_h, row_block, nshards) rows; rt_unshard and rt_slab_* are called with
 * (win_w, win_h) and know nothing of windows.  x0 and y0 need no alignment (a window whose rows
 * are multiples of 16 bytes gets wider stores where no sphere can be hit, the same bytes).
 * Placing a packed window into a pitched whole frame is the caller's hipMemcpy2DAsync (source pitch
 * win_w*3 elements, destination pitch width*3 elements, at row y0 and element x0*3): the library
 * writes no pitched output.
 * The window (0, 0, width, height) is the whole-frame call — one code path: rt_launch_spp is
 * rt_launch_window with it, and rt_render without a window fills it in.
 * rt_render with opts->win_*: width and height stay the image's, out_rgb and opts->out_levels are
 * the window's (win_w*win_h*3 elements, win_w*win_h bytes), rt_stats.pixels = win_w*win_h; every
 * other option (precision, integer frames, spp, nshards, ndev, RT_LEVELS_HIT, pinned or pageable
 * destinations) works as for a win_w x win_h frame.  rt_render_ppm_file and rt_render_rawppm_file
 * write a win_w x win_h file whose header says "win_w win_h". */

/* RT_SUPERSAMPLING — stochastic supersampling (BASELINE.json config 5; the reference has
 * none, so this definition is the contract and the oracle restates it).  With spp > 1,
 * sample s (0 <= s < spp) of pixel (x, y), pixel = y*W + x in the whole image:
 *     r = splitmix64(seed ^ (pixel*spp + s)),
 *         splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 *                        z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31;
 *     u = (r >> 40) * 2^-24,  v = ((r >> 16) & 0xFFFFFF) * 2^-24      (24-bit fractions)
 *     X = (x + u) / W,  Y = (y + v) / H                                 (binary64)
 * and the pixel is (c_0 + c_1 + ... + c_{spp-1}) / spp, summed left to right in binary64.
 * spp = 1 is the reference's X = x/W, Y = y/H exactly.  out_levels / d_levels report
 * sample 0 (its chain's level count, or with RT_LEVELS_HIT its primary-hit mask).
 * Levels count the objects a pixel's reflection chain hit (0 = background).  A scene without
 * point lights traces no reflections (the reference's fold over the lights never recurses,
 * raytracer.erl:209-252), so there a pixel's level is at most 1 with or without RT_LEVELS_HIT;
 * so it is at depth 1. */
#define RT_MAX_SPP 4096

/* RT_PROGRESSIVE — a range of a frame's samples, bit for bit a prefix of the frame's sum, at the
 * cost of the range; and a frame from a sum.
 * The supersampled frame is fixed as (c_0 + ... + c_{spp-1}) / spp, summed left to right in binary64,
 * and sample s of a pixel depends only on (seed, pixel, spp, s): a sum that is kept can be continued.
 * rt_launch_samples folds samples [sample_begin, sample_end) of the spp-sample frame that
 * rt_launch_window renders with the same (width, height, depth, window, row_block, shard, nshards,
 * spp, seed) into the caller's sum; rt_resolve turns a sum into a frame of any RT_OUT_* format.
 * The sum: d_sum is a caller-owned binary64 slab laid out like an RT_OUT_F64 output slab,
 *   rt_shard_rows(win_h, row_block, nshards) rows of win_w*3 doubles; slab rows past the image are not
 *   touched.  Sample 0 STORES (the caller need not clear d_sum, and a call with sample_begin = 0
 *   restarts the frame); every later sample s does sum = sum + c_s in binary64, in sample order, so
 *   after the call d_sum holds c_0 + ... + c_{sample_end-1} summed left to right — also when
 *   sample_end = spp: no call divides, no call writes a frame.  (A background pixel's sum is +0.0
 *   from sample 0 on and is neither read nor written by a later sample: a running sum is never -0.0,
 *   so adding the background's +0.0 would give back its bits.)  The caller promises that d_sum holds
 *   samples [0, sample_begin) of the same frame, which the library cannot check.  The call owns d_sum
 *   until its stream reaches the end of the call; it is asynchronous on `stream` like rt_launch.
 * The order is always the reference's (RT_ORDER_EXACT; rt_launch_spp ignores `order` for spp > 1 too).
 *   spp = 1 is allowed: the one sample is the unjittered frame, rendered by the wavefront engine.
 * d_levels (optional) is written by the call that holds sample 0, with sample 0's level counts
 *   (RT_SUPERSAMPLING); a call with sample_begin > 0 leaves it untouched, so a caller may pass the
 *   same arguments every time.
 * Guarantees:
 *   G1  Any partition gives the frame.  For any 0 = b_0 < b_1 < ... < b_k = spp, the calls for
 *       [b_j, b_{j+1}) in order on one stream followed by rt_resolve(samples = spp) to RT_OUT_F64 or
 *       RT_OUT_F32 give the slab rt_launch_window writes for the same arguments with RT_ORDER_EXACT,
 *       in every byte, and the same levels — for every context configuration (side streams on or off,
 *       culling on or off, levels requested or not).
 *   G2  The sum does not depend on the partition: the sum after [0, k) is bit-equal whether one call
 *       made it or several.
 *   G3  An 8- or 16-bit preview is the quantised float preview: rt_resolve to RT_OUT_U8 / RT_OUT_U16
 *       gives the bytes and the clamped count of rt_quantize applied to rt_resolve(..., RT_OUT_F64),
 *       for 3 or 6 bytes per pixel of traffic out instead of 24.
 *   G4  A call costs its samples: sample_end - sample_begin sample passes, nothing proportional to spp.
 * Splitting a frame's samples over devices is not offered: the left-to-right sum forbids it. */

typedef struct rt_stats {
    double kernel_ms;   /* device time of the render kernels, and of an integer frame's quantise
                           passes between them (max over devices) */
    double total_ms;    /* wall time of the whole call, boundary to boundary */
    uint64_t pixels;    /* W*H; with a window win_w*win_h */
    int32_t ndev;       /* devices actually used */
    int32_t flags;      /* bit 0: out_rgb was pinned host memory (written by DMA directly);
                           bit 1 (RT_STATS_CLAMPED): an integer frame stored at least one channel as
                           0 because it was negative or NaN (the call still returns RT_OK) */
} rt_stats;
#define RT_STATS_PINNED 1
#define RT_STATS_CLAMPED 2

/* ---- library / device ------------------------------------------------------------ */
int rt_abi_version(void);
const char *rt_strerror(int code);
int rt_device_count(int *count);

/* Diagnostic: the kernels' correctly rounded sqrt / division fast paths (rt_math.inc,
 * sqrt_n / div_n: the device library's sequences without their range handling, used only
 * where every operand of the wave is in range) against the library, bit for bit, on n random
 * operands; *mismatches = the count of differing results (0 expected). */
int rt_selftest_math(int device, uint64_t n, uint64_t seed, uint64_t *mismatches);

/* Diagnostic (test-only ABI like rt_selftest_math; no render path calls it, and it may change
 * with the kernels' internals): evaluate one of the kernels' arithmetic primitives on host
 * arrays of binary64 operands, one operand per work-item in array order, 256 work-items per
 * workgroup — elements 64k .. 64k+63 form one wave, so the caller's operand order decides
 * which of the primitives' wave-uniform paths run.  Results go back to host arrays.
 *   RT_EVAL_POW          out[i] = pow_libm<false>(a[i], b[i], act[i]); act (optional, n bytes):
 *                        lanes with act[i] = 0 are the shading's inactive lanes, whose out[i] is
 *                        unspecified.  b[i] must be an integer in [0, 1024] (the host's guarantee
 *                        for kernels built without the general pow).
 *   RT_EVAL_POW_GENERAL  out[i] = pow_libm<true>(a[i], b[i]): any b
 *   RT_EVAL_SQRT         out[i] = sqrt_x<false>(a[i])
 *   RT_EVAL_DIV          out[i] = div_n(a[i], b[i]): no range handling, see rt_math.inc
 *   RT_EVAL_NORMALIZE3   a and out hold n vectors (3n values): out = normalize3(a, false)
 *   RT_EVAL_DIV_DIM      out[i] = div_dim(a[i], dim), 1 <= dim <= 2^20 (one scalar per call)
 *   RT_EVAL_IDIV_DIM     out[i] = idiv_dim((int)a[i], dim), a[i] an integer in [0, 2^31)
 * b is read by the first, second and fourth operation only; n <= 2^26. */
enum rt_eval_op {
    RT_EVAL_POW = 0,
    RT_EVAL_POW_GENERAL = 1,
    RT_EVAL_SQRT = 2,
    RT_EVAL_DIV = 3,
    RT_EVAL_NORMALIZE3 = 4,
    RT_EVAL_DIV_DIM = 5,
    RT_EVAL_IDIV_DIM = 6
};
int rt_eval_math(int device, int op, uint64_t n, const double *a, const double *b, const uint8_t *act,
                 int32_t dim, double *out);

/* Validate a scene list without rendering (0 = a scene the reference would
 * trace without crashing for a pixel that hits any object). */
int rt_scene_check(const rt_elem *scene, uint32_t n_elems);

/* Fill canon[] for elems whose canon is -1 (bitwise-equality rule). */
int rt_scene_canon(rt_elem *scene, uint32_t n_elems);

/* ---- one-shot render: the drop-in for raytraced_pixel_list_{simple,concurrent,distributed} --
 * Replaces the whole pixel loop (raytracer.erl:86-178): for every pixel (x,y),
 * row-major, out = trace_ray_through_pixel({x/W, y/H}, Scene, Depth).
 * out_rgb: caller-owned host memory, W*H*3 elements of the chosen precision.
 * Returns RT_DONE for W = H = 0, RT_EBADARG if exactly one of them is 0.
 * The process keeps a pool of render contexts per device (streams, device frame buffers, the
 * wavefront work space, the last scene compiled — recompiled only when the scene's bytes
 * change), created on first use: the reference calls its strategy once per frame
 * (raytracer.erl:723-733), and repeated calls pay only the render and the copy.  The frame is
 * rendered in row bands whose copies to the host overlap the next band's render; memory from
 * rt_host_alloc (or registered with HIP) is written by DMA directly, other memory through a
 * pinned staging ring.  Thread-safe: concurrent callers get separate contexts (up to 4 per
 * device; more wait).  Device memory per context: the wavefront work space of the largest frame
 * it rendered (~5 GB at 4096^2 depth 5: 64-byte hit records per level and 16x16-tile slot,
 * colours, flags, lists; spp > 1 adds the binary64 sums, 24 B per pixel) plus its output
 * buffers (the frame, 201 MB at 4096^2 f32); it is kept while the context is idle.  An
 * allocation that fails while other contexts of the device are idle is retried once after their
 * memory is freed (a busy context's is never touched); rt_reset_contexts frees it all.
 * Integer frames (precision RT_OUT_U8 / RT_OUT_U16, opts->max_value): every row band is rendered
 * in binary64 and quantised on the GPU (rt_quantize) before its copy, so out_rgb receives 3 or
 * 6 bytes per pixel instead of 24; the context keeps the binary64 frame and the integer one.
 * Every other option works as for float frames.  RT_ETOOBIG for a max_value above the format's
 * limit; a channel that was negative or NaN is stored as 0 and sets RT_STATS_CLAMPED. */
int rt_render(const rt_elem *scene, uint32_t n_elems, uint32_t width, uint32_t height,
              uint32_t depth, const rt_opts *opts, void *out_rgb, rt_stats *stats);

/* Pinned (page-locked) host memory for rt_render's out_rgb: the frame is written by DMA
 * straight into it (a NIF can wrap it in a resource binary; the Python host uses it for its
 * frames).  rt_host_alloc returns NULL on failure.  Freed blocks are kept for reuse (up to 8
 * blocks / 4 GiB; a request reuses a block at most twice its size), so allocating one per
 * frame costs nothing after the first; rt_host_free of a pointer not from rt_host_alloc
 * returns RT_EBADARG. */
void *rt_host_alloc(size_t bytes);
int rt_host_free(void *p);
/* Free the idle render contexts of the process (device memory, streams) and the cached
 * pinned blocks; returns the number of contexts still in use by other threads.  The next
 * rt_render creates them again. */
int rt_reset_contexts(void);

/* ---- resident-scene API (device buffers, caller's HIP stream) -------------------
 * rt_prepare uploads the scene (and its per-origin constant tables) to one device.
 * rt_launch renders shard `shard` of `nshards` into device memory, asynchronously
 * on `stream` (a hipStream_t; NULL = the null stream).  Rows are dealt to shards
 * in interleaved blocks of `row_block` rows: global row g belongs to shard
 * (g / row_block) % nshards.  d_out receives the shard's rows packed in order,
 * rt_shard_rows(height,row_block,nshards) rows of width*3 elements; slab rows past
 * the image (the tail of the last row block) are not written, so with nshards = 1 a buffer
 * of `height` rows suffices.  d_levels (optional) gets one byte per slab pixel.
 * rt_launch / rt_launch_spp write floats only (precision RT_OUT_F64 or RT_OUT_F32).  A resident
 * integer frame is rt_launch into a binary64 slab followed by rt_quantize of the slab's image
 * rows (a prefix of the slab) on the same stream; rt_unshard and the compact slab transfer below
 * take the integer slabs. */
typedef struct rt_prepared rt_prepared;

int rt_prepare(const rt_elem *scene, uint32_t n_elems, int device, rt_prepared **out);
uint32_t rt_shard_rows(uint32_t height, uint32_t row_block, uint32_t nshards);
int rt_launch(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth,
              uint32_t row_block, uint32_t shard, uint32_t nshards, int precision, int order,
              void *d_out, uint8_t *d_levels, void *stream);
/* rt_launch with spp samples per pixel (RT_SUPERSAMPLING); spp = 1 is rt_launch. */
int rt_launch_spp(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth,
                  uint32_t row_block, uint32_t shard, uint32_t nshards, int precision, int order,
                  uint32_t spp, uint64_t seed, void *d_out, uint8_t *d_levels, void *stream);
/* rt_launch_spp for the window (x0, y0, win_w, win_h) of the width x height image (RT_WINDOW):
 * d_out is the window's slab, rt_shard_rows(win_h, row_block, nshards) rows of win_w*3 elements,
 * d_levels one byte per slab pixel.  RT_EBADARG for an empty window or one that leaves the image,
 * RT_ETOOBIG as rt_launch_spp for a width or height above 2^20; the arguments are checked before
 * any HIP call.  (The name holds no digits, see rt_render_rawppm_file.) */
int rt_launch_window(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                     uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards,
                     int precision, int order, uint32_t spp, uint64_t seed, void *d_out, uint8_t *d_levels,
                     void *stream);
/* RT_PROGRESSIVE: fold samples [sample_begin, sample_end) of rt_launch_window's spp-sample frame into
 * d_sum (see the contract above); writes no frame.  All checked before any HIP call and before p is
 * read: RT_EBADARG for a null p or d_sum, a d_sum that is not 8-byte aligned, spp = 0,
 * sample_begin >= sample_end or sample_end > spp; RT_ETOOBIG for spp > RT_MAX_SPP; the window, shard
 * and size errors exactly as rt_launch_window. */
int rt_launch_samples(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth,
                      uint32_t x0, uint32_t y0, uint32_t win_w, uint32_t win_h,
                      uint32_t row_block, uint32_t shard, uint32_t nshards,
                      uint32_t spp, uint64_t seed, uint32_t sample_begin, uint32_t sample_end,
                      double *d_sum, uint8_t *d_levels, void *stream);
/* RT_PROGRESSIVE: a frame from a sum, asynchronously on `stream`; neither synchronises nor allocates.
 *     m = d_sum[i] / (double)samples        (binary64, i < n_values)
 *   RT_OUT_F64 stores m, RT_OUT_F32 (float)m, RT_OUT_U8 / RT_OUT_U16 min(trunc(m*max_value), max_value)
 *   by rt_quantize's rule in every detail: a negative result or a NaN is stored as 0 and counted into
 *   *d_clamped (optional, device memory, zeroed by the caller), -0.0 and values in (-1/max_value, 0)
 *   give 0 uncounted, +inf gives max_value.  The array is flat, as for rt_quantize: pass the slab's
 *   rows inside the image (a prefix).  The buffers must not overlap.
 *   samples in [1, RT_MAX_SPP]: 0 is RT_EBADARG, more RT_ETOOBIG.  max_value is read for the integer
 *   formats only: 0 is RT_EBADARG, above the format's limit RT_ETOOBIG.  Alignment: d_sum to 8 bytes,
 *   d_out to its element, d_clamped to 8, anything else is RT_EBADARG; values before d_out's first
 *   16-byte boundary and the last few are converted one by one, the rest eight per work-item (16-byte
 *   loads when d_sum is 16-byte aligned there; the same bytes otherwise).  RT_EBADARG for a null
 *   d_sum or d_out or a bad out_format; n_values 0 launches nothing.  All checked before any HIP call. */
int rt_resolve(const double *d_sum, uint64_t n_values, uint32_t samples, int out_format,
               uint32_t max_value, void *d_out, uint64_t *d_clamped, void *stream);
/* RT_ATTRIBUTES — what a pixel's primary ray hits: the object, the distance, the point, the normal
 * and the albedo, as planes laid out like the frame (picking, depth and normal passes, guide buffers
 * of a denoiser).  Additive: RT_ABI_VERSION stays 5.
 * Planes: caller-owned device memory, each laid out as rt_launch_window's slab for the same window,
 *   row_block, shard and nshards — rt_shard_rows(win_h, row_block, nshards) rows of win_w pixels; slab
 *   rows past the image are not written.  A null pointer is a plane not wanted and is never written.
 *   d_elem holds one int32 per pixel, d_t one element, d_point / d_normal / d_albedo three elements;
 *   the element of the four float planes is `precision` (RT_OUT_F64 or RT_OUT_F32), and the three
 *   3-channel planes are RT_OUT_F64 / RT_OUT_F32 slabs in every respect: rt_unshard, rt_slab_pack and
 *   rt_slab_unpack take them as they are.
 * The ray of slab pixel (x, y) is the one rt_launch_window traces for sample `sample` of an spp-sample
 *   frame: with spp = 1 (and sample = 0) the reference's ray through {X/Width, Y/Height}, with spp > 1
 *   jittered as RT_SUPERSAMPLING defines (the window's pixels are the image's: RT_WINDOW).  There is no
 *   depth: the attributes are the primary hit's and depend on nothing deeper.
 * At a hit the values are what nearest_object_intersecting_ray/2 returns for that ray over the scene
 *   list (raytracer.erl:300-346; ties keep the earlier list element, negative distances win):
 *     d_elem    the index into the caller's rt_elem array of the object hit (>= 1: element 0 is the
 *               camera) — the list position, not the compact id and not `canon`
 *     d_t       Distance (it can be negative for triangles and planes)
 *     d_point   Intersection, as the reference's intersect functions compute it (:384-390, :443-451, :471-476)
 *     d_normal  the normal of that hit record
 *     d_albedo  #material.colour of the object
 *   At a miss d_elem = -1, d_t = +infinity (the reference's `infinity` start value) and the three
 *   3-channel planes hold +0.0 in every channel, so a packed slab treats them as background.
 *   RT_OUT_F32 stores (float) of the binary64 value; nothing is computed in binary32.
 * Checked before any HIP call and before p is read: RT_EBADARG for a null p or planes, a struct_size
 *   that ends before d_albedo, all five planes null, a bad precision, spp = 0, sample >= spp, a d_elem
 *   that is not 4-byte aligned or a float plane not aligned to its element; RT_ETOOBIG for
 *   spp > RT_MAX_SPP; the window, shard and size errors exactly as rt_launch_window.
 * The call is asynchronous on `stream`; it neither synchronises nor allocates, and uses none of the
 *   context's work space.  The values are bit-equal for every context configuration (culling on or
 *   off, side streams on or off). */
typedef struct rt_attr_planes {
    uint32_t struct_size;   /* sizeof(rt_attr_planes) */
    int32_t  precision;     /* RT_OUT_F64 or RT_OUT_F32: element of the four float planes */
    int32_t *d_elem;        /* [rows][win_w]     */
    void    *d_t;           /* [rows][win_w]     */
    void    *d_point;       /* [rows][win_w][3]  */
    void    *d_normal;      /* [rows][win_w][3]  */
    void    *d_albedo;      /* [rows][win_w][3]  */
} rt_attr_planes;

int rt_launch_attrs(rt_prepared *p, uint32_t width, uint32_t height,
                    uint32_t x0, uint32_t y0, uint32_t win_w, uint32_t win_h,
                    uint32_t row_block, uint32_t shard, uint32_t nshards,
                    uint32_t spp, uint64_t seed, uint32_t sample,
                    const rt_attr_planes *planes, void *stream);
/* RT_QUERY — the same questions for rays the caller chose: the nearest hit of n arbitrary rays
 * (rt_query_rays: nearest_object_intersecting_ray/2, raytracer.erl:300-346) and the shadow test
 * between n pairs of points (rt_query_shadow: shadow_factor/4, :256-267), on the scene of the last
 * rt_prepare / rt_update_scene.  Picking along a ray that is no pixel's, line of sight, "which lights
 * see this point", a first-hit pass for a camera the reference does not have, occlusion and collision
 * probes: each is one batch.  Additive: RT_ABI_VERSION stays 5.
 * rt_query_rays: ray i starts at d_origin[3i..3i+2] — with RT_QUERY_ONE_ORIGIN at d_origin[0..2], one
 *   point shared by all n rays — and has the direction d_dir[3i..3i+2].  Inputs are device memory and
 *   always binary64.  The direction is used as given: the reference's scan does not normalise
 *   #ray.direction, so t is in units of |direction| (and, as in the reference, a sphere's t is only a
 *   distance for a unit direction).
 *   out: an rt_attr_planes whose planes are flat arrays of n entries — d_elem[n], d_t[n], d_point,
 *   d_normal and d_albedo [n][3]; `precision` (RT_OUT_F64 or RT_OUT_F32) is the element of the four
 *   float planes; a null pointer is a plane not wanted and is never written.  Hit and miss values are
 *   RT_ATTRIBUTES': d_elem the index in the caller's rt_elem array (ties keep the earlier list element,
 *   negative distances of triangles and planes win), d_t the Distance, d_point origin + direction*t as
 *   the intersect functions compute it, d_normal that hit record's normal, d_albedo #material.colour;
 *   a miss is -1, +infinity and +0.0 in every channel.  RT_OUT_F32 stores (float) of the binary64
 *   value; nothing is computed in binary32.
 *   Every stored value is bit for bit what nearest_object_intersecting_ray/2 returns, for every ray
 *   whose arithmetic stays finite in the reference (Erlang raises badarith where C gives an infinity
 *   or a NaN).  A ray with a component that is not finite, or one whose arithmetic overflows, gets
 *   unspecified values in its own entries; it causes no fault and has no effect on any other ray.  A
 *   zero direction is inside the contract: it misses everything, as in the reference.
 *   Ray i's bytes do not depend on n, on i, on the other rays of the batch, on RT_QUERY_ONE_ORIGIN
 *   against a repeated origin, or on the context's configuration (RT_CFG_CULL, side streams).
 *   Entries >= n of every plane are never written.
 * rt_query_shadow: for triple i the ray from d_light[3i..] in the direction vector_normalize(d_hit[3i..]
 *   - d_light[3i..]) (the zero vector for equal points, as vector_normalize/1 gives); d_lit[i] = 1 iff
 *   that ray's nearest object and element d_elem[i] of the caller's rt_elem array are the same term —
 *   equal `canon`, the renderer's rule, so another bit-identical copy of the object matches (:262) — and
 *   0 in every other case: nothing is hit, another object is hit, or d_elem[i] is negative, >= the
 *   scene's element count, or a camera, light or RT_OTHER element.  RT_QUERY_ONE_ORIGIN: one light
 *   location, d_light[0..2], for all n.  Bytes >= n of d_lit are never written.
 * Both calls are asynchronous on `stream`, neither synchronise nor allocate, and use none of the
 *   context's work space.  n = 0 launches nothing and returns RT_OK.
 * Checked before any HIP call and before p is read: RT_EBADARG for a null p, d_origin, d_dir, d_light,
 *   d_hit, d_elem, d_lit or out, an unknown flag bit, an input pointer that is not 8-byte aligned
 *   (d_elem: 4-byte), an `out` that fails rt_launch_attrs' plane checks (struct_size, all planes null,
 *   precision, alignment); RT_ETOOBIG for n > RT_MAX_QUERY_RAYS.
 * rt_query_colours: the colour ray i sees, d_rgb[3i..3i+2] = pixel_colour_from_ray(Ray_i, Scene, depth)
 *   (raytracer.erl:186-252), for the rays of rt_query_rays (d_origin, d_dir, RT_QUERY_ONE_ORIGIN; the
 *   direction used as given).  Mirror probes, light-field samples, orthographic, fisheye, stereo and
 *   depth-of-field cameras, a camera that is aimed: each is one batch.  Depth 0 is {0,0,0} without a
 *   scan and a miss is the background {0,0,0}; otherwise lighting_function/6 with the reflection added
 *   once per light, in the reference's fold order — RT_ORDER_EXACT, no other order is offered — and
 *   shadow_factor/4 as the renderer has it (matched by `canon`).  `precision` is RT_OUT_F64 or
 *   RT_OUT_F32 (d_rgb's element); RT_OUT_F32 stores (float) of the binary64 value, nothing is computed
 *   in binary32.  Bit-exactness holds in the same sense as for rendered frames: for rays whose
 *   arithmetic stays finite in the reference every byte is the reference's, apart from the known pow
 *   rounding (none with specular powers 0 and 1).
 *   d_levels is optional (null: not wanted): d_levels[i] is the number of objects ray i's reflection
 *   chain hit, rt_launch's definition — 0 is a miss, the count saturates at 255, and it is at most 1 in
 *   a scene without point lights.
 *   Ray i's bytes do not depend on n, on i, on the other rays of the batch, on RT_QUERY_ONE_ORIGIN
 *   against a repeated origin, or on the context's configuration (RT_CFG_CULL, side streams).
 *   Entries >= n of d_rgb and d_levels are never written.  A ray with a component that is not finite,
 *   or one whose arithmetic overflows, gets unspecified values in its own entries; it causes no fault
 *   and has no effect on any other ray.  A zero direction is inside the contract and misses everything.
 *   d_work is caller-owned device memory, 16-byte aligned, of at least
 *   rt_query_colours_work_bytes(n, depth) bytes (76 per ray and level, n rounded up to a multiple of
 *   64); its contents are unspecified before and after the call, and the call owns it until `stream`
 *   reaches the end of the call.  The size function is host-only and makes no HIP call; it returns 0
 *   for depth 0 or n = 0 (then d_work may be null), and also 0 where the size overflows size_t.  There
 *   is no limit on depth other than the work space the caller can allocate.
 *   The call is asynchronous on `stream`, neither synchronises nor allocates, and uses none of the
 *   context's work space.  n = 0 launches nothing and returns RT_OK.
 *   Checked before any HIP call and before p is read, RT_EBADARG before RT_ETOOBIG: RT_EBADARG for a
 *   null p, d_origin, d_dir or d_rgb, an unknown flag bit, a bad precision, an input pointer that is
 *   not 8-byte aligned, a d_rgb not aligned to its element, and — for n <= RT_MAX_QUERY_RAYS with a
 *   required size that is not zero — a d_work that is null or not 16-byte aligned, or work_bytes below
 *   the required size; RT_ETOOBIG for n > RT_MAX_QUERY_RAYS (the work space is not looked at) and for
 *   a required size that overflows size_t. */
#define RT_QUERY_ONE_ORIGIN 1   /* d_origin / d_light holds ONE point (3 doubles) shared by all n rays */
#define RT_MAX_QUERY_RAYS (1u << 30)

int rt_query_rays(rt_prepared *p, const double *d_origin, const double *d_dir, uint64_t n,
                  uint32_t flags, const rt_attr_planes *out, void *stream);

int rt_query_shadow(rt_prepared *p, const double *d_light, const double *d_hit,
                    const int32_t *d_elem, uint64_t n, uint32_t flags,
                    uint8_t *d_lit, void *stream);

size_t rt_query_colours_work_bytes(uint64_t n, uint32_t depth);
int rt_query_colours(rt_prepared *p, const double *d_origin, const double *d_dir, uint64_t n,
                     uint32_t depth, uint32_t flags, int precision,
                     void *d_rgb, uint8_t *d_levels, void *d_work, size_t work_bytes, void *stream);
/* Reassemble nshards gathered slabs (d_slabs = [nshards][shard_rows][W*3]) into the
 * row-major image d_image ([H][W*3]), on `stream`.  precision: the slabs' element, any of
 * RT_OUT_F64, RT_OUT_F32, RT_OUT_U8, RT_OUT_U16 (rows of W*3 elements of 8, 4, 1 or 2 bytes); the
 * call is device copies of whole rows, so no alignment is asked of an integer slab. */
int rt_unshard(const void *d_slabs, uint32_t width, uint32_t height, uint32_t row_block,
               uint32_t nshards, int precision, void *d_image, void *stream);
int rt_release(rt_prepared *p);
/* Replace the scene of a prepared context in place (an animated scene: the next rt_launch renders
 * the new one): the scene is compiled and uploaded as by rt_prepare, the context's work space,
 * streams and options are kept.  No launch of p may be in flight (synchronise its stream first). */
int rt_update_scene(rt_prepared *p, const rt_elem *scene, uint32_t n_elems);
/* Per-context launch options.
 * RT_CFG_SIDE_STREAMS: 1 = a frame's shading runs on two low-priority side streams of the
 *   context beside its reflection chain (the fastest for ONE frame in flight); 0 = every
 *   kernel on the caller's stream (for callers that keep several frames in flight on
 *   their own streams, one context each: the frames then fill each other's latency-bound
 *   tails); -1 = the default (on, unless the environment sets RT_LIT_STREAM=0). */
#define RT_CFG_SIDE_STREAMS 1
/* RT_CFG_KERNEL_TIMING: value = a mask of RT_KT_* kernels; every later launch of those kernels
 *   by this context is bracketed by HIP timing events on the stream it runs on (0 = off, the
 *   default).  rt_kernel_time reports their summed duration and launch count (it waits for
 *   the events recorded so far).  Used by bench.py for the roofline of the dominant kernel. */
#define RT_CFG_KERNEL_TIMING 2
#define RT_KT_PRIMARY 1  /* k_primary: camera rays and their nearest scan (wavefront engine) */
#define RT_KT_LEVEL1 2   /* the level-0 shading + level-1 reflection pass (k_reflect_shade(1); with
                            side streams or levels: k_reflect(1)) */
#define RT_KT_RENDER 4   /* k_render: the fused engine's one kernel per frame */
#define RT_KT_PMASK 8    /* k_pmask: the primary rays' candidate masks, computed when the scene, the culling
                            mode or the frame geometry changes (the wavefront engine, culled scenes) */
/* RT_CFG_CULL: 1 = the default: scans skip objects a conservative filter proves cannot be hit
 *   (wave beams and shadow cones, per-light occluder masks, the sphere BVH); 0 = brute force,
 *   every nearest scan and every shadow test visits every object of the scene, as the
 *   reference's scans do (raytracer.erl:303-346, :256-267).  Both give the same bits; 0 exists
 *   to check that (it is many times slower). */
#define RT_CFG_CULL 3
int rt_configure(rt_prepared *p, int option, int64_t value);
/* Which engine rt_launch_spp runs for this context's scene at `spp` samples per pixel:
 * RT_ENGINE_WAVE (the wavefront kernels) or RT_ENGINE_FUSED (k_render, one kernel per frame);
 * negative on a bad argument.  bench.py names the dominant kernel from it. */
#define RT_ENGINE_WAVE 0
#define RT_ENGINE_FUSED 1
int rt_engine(rt_prepared *p, uint32_t spp);
int rt_kernel_time(rt_prepared *p, int kernel, double *total_ms, uint64_t *launches, int reset);
/* ---- compact slab transfer (the multi-GPU gather; raytracer.erl:151-161 collects pixels) --
 * A slab (as rt_launch writes it) is mostly background pixels, +0.0 in all three channels.
 * For the gather it is sent as a fixed-size header (count of non-zero pixels, u64 at byte
 * 0; per 256 slab pixels the non-zero pixels before them; one bit per slab pixel) plus
 * count*3 values of the slab's precision, the non-zero pixels in slab order.  The round trip
 * is exact (bit patterns are copied; a pixel is zero iff its three channels are all-zero
 * bits).  Slab rows past the image are not read and decode as zero.
 * Integer slabs (precision RT_OUT_U8 / RT_OUT_U16: a binary64 slab quantised by rt_quantize on the
 * rank that rendered it) take the same header; their values are the non-zero pixels' three
 * samples, 3 bytes per pixel for RT_OUT_U8 and 6 (native endian) for RT_OUT_U16.  A pixel is
 * non-zero iff any of its three samples is (a 16-bit sample such as 0x0100 or 0x0001 is), so the
 * round trip is exact for them too.
 * rt_slab_header_bytes: header size for one shard of this frame (0 for bad arguments).
 * rt_slab_pack: encode shard `shard`'s slab on `stream`; d_values needs room for every slab
 *   pixel (shard_rows*width*3 elements) in the worst case.
 * rt_slab_unpack: decode nshards (<= RT_MAX_SHARDS) shards into the row-major image
 *   ([H][W*3]) on `stream` — rt_unshard fused with the decode; d_headers[s] / d_values[s]
 *   are device pointers to shard s's header and values.
 * Alignment: a header must be 8-byte aligned (its u64 count and mask words; the mask offset is a
 *   multiple of 256), a slab, a values buffer and d_image aligned to their element (4 bytes for
 *   RT_OUT_F32, 8 for RT_OUT_F64).  A 16-byte aligned d_image whose width is a multiple of 4 is
 *   written with 16-byte stores; any other one element by element (slower, same bytes).
 *   Integer formats: RT_OUT_U8 buffers may start anywhere; an RT_OUT_U16 slab, values buffer or
 *   d_image that is not 2-byte aligned is RT_EBADARG (checked with the other arguments, before any
 *   HIP call).  A values buffer need not be aligned any further (rank 0's are rows of a byte
 *   matrix): the decode reads it the same way at every alignment.  A 16-byte aligned d_image whose
 *   width is a multiple of 16 (RT_OUT_U8) or 8 (RT_OUT_U16) pixels is decoded 48 bytes per thread
 *   and written with 16-byte stores; any other one sample at a time (slower, same bytes).
 * A pack owns its header and values buffers until its kernels have run: the block offsets are
 *   scanned in place in the header, so two packs in flight (on different streams) must not share
 *   a header or a values buffer, and neither may be read before the pack's stream reaches it. */
#define RT_MAX_SHARDS 64
size_t rt_slab_header_bytes(uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards);
int rt_slab_pack(const void *d_slab, uint32_t width, uint32_t height, uint32_t row_block, uint32_t shard,
                 uint32_t nshards, int precision, void *d_header, void *d_values, void *stream);
int rt_slab_unpack(const void *const *d_headers, const void *const *d_values, uint32_t width, uint32_t height,
                   uint32_t row_block, uint32_t nshards, int precision, void *d_image, void *stream);

/* ---- P3 output: write_pixels_to_ppm/5 (raytracer.erl:667-685) -----------------------
 * The file is "P3\nW H\nMaxValue\n" followed, for every pixel in row order, by
 * "R G B " where each channel is min(trunc(C*MaxValue), MaxValue) printed in decimal
 * (C*MaxValue in binary64; no lower clamp, so a negative colour prints a negative
 * number).  Byte-exact for RT_OUT_F64 frames; an RT_OUT_F32 frame is formatted from its
 * float values.
 * rt_ppm_bound: a byte count that always suffices for rt_ppm_format's output.
 * rt_ppm_format: formats a device frame (precision as rt_launch writes it) into the device
 *   buffer d_text (text_cap bytes) on `stream`, then synchronises it to report *text_len.
 *   RT_ERANGE if a channel is below -2^31 (BEAM prints such values as bignums; the file
 *   API below formats them on the host), RT_ETOOBIG if text_cap is too small.
 * rt_render_ppm_file: raytrace/5 without the strategy fun — render (opts as rt_render) and
 *   write the P3 file at `path`; the text is produced on the GPU. */
size_t rt_ppm_bound(uint32_t width, uint32_t height, uint32_t max_value);
int rt_ppm_format(const void *d_rgb, int precision, uint32_t width, uint32_t height, uint32_t max_value,
                  char *d_text, size_t text_cap, size_t *text_len, void *stream);
int rt_render_ppm_file(const rt_elem *scene, uint32_t n_elems, uint32_t width, uint32_t height,
                       uint32_t depth, const rt_opts *opts, uint32_t max_value, const char *path,
                       rt_stats *stats);

/* ---- integer frames and the binary P6 file ------------------------------------------------
 * rt_quantize: a device array of n_values channels (precision as rt_launch writes it; a frame
 *   is taken as a flat array, no pixel structure is needed) to 8- or 16-bit samples in d_out,
 *   asynchronously on `stream`; it neither synchronises nor allocates.
 *     out[i] = min(trunc((double)in[i] * (double)max_value), max_value)     (binary64)
 *   the rule of the P3 writer above, so +inf gives max_value.  What an unsigned sample cannot
 *   hold — a result below 0, or a NaN — is stored as 0, and *d_clamped (optional, device memory,
 *   zeroed by the caller) is increased by the number of such values; -0.0 and values in
 *   (-1/max_value, 0) truncate to 0 and are not counted.
 *   Alignment: d_rgb aligned to its element (8 bytes for RT_OUT_F64, 4 for RT_OUT_F32), d_out to
 *   its own (1 or 2 bytes), d_clamped to 8; anything else is RT_EBADARG.  Any such pair works: the
 *   values before d_out's first 16-byte boundary and the last n % 8 are converted one by one, the
 *   rest with 16-byte loads when d_rgb is 16-byte aligned at that boundary (element loads
 *   otherwise: slower, same bytes) and 8- or 16-byte stores.
 *   RT_EBADARG for a null d_rgb or d_out, a bad precision or out_format, or max_value 0;
 *   RT_ETOOBIG for a max_value above the format's limit; n_values 0 launches nothing.  The
 *   arguments are checked before any HIP call.
 * rt_render_rawppm_file: rt_render_ppm_file for the binary ("raw", magic P6) format:
 *   "P6\nW H\nMaxValue\n" followed by the samples of the P3 file, 1 byte each for
 *   max_value <= 255, else 2 bytes each, most significant byte first.  A frame with a value P3
 *   would print as negative cannot be written: RT_ERANGE, and no file is created.  RT_ETOOBIG for
 *   max_value > RT_MAX_INT_VALUE, RT_EBADARG for 0; a width or height of 0 as in
 *   rt_render_ppm_file.  (Entry-point names hold no digits: the export list is matched against
 *   this header by letters and underscores alone.) */
int rt_quantize(const void *d_rgb, int precision /* RT_OUT_F64|RT_OUT_F32 */, uint64_t n_values,
                uint32_t max_value, int out_format /* RT_OUT_U8|RT_OUT_U16 */, void *d_out,
                uint64_t *d_clamped /* optional, device */, void *stream);
int rt_render_rawppm_file(const rt_elem *scene, uint32_t n_elems, uint32_t width, uint32_t height,
                          uint32_t depth, const rt_opts *opts, uint32_t max_value,
                          const char *path, rt_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
