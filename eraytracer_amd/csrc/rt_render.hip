// rt_render.hip — the MI355X (gfx950) render kernels and the C-ABI of include/rt_mi355x.h.
//
// One translation unit (the kernel templates are launched from the code that picks their
// arguments): the device code lives in the rt_*.inc fragments included below, inside the anonymous
// namespace and in order of dependence; this file is the host side — rt_prepared and its work
// space, the choice of engine and kernel template, frame graphs and the C-ABI entry points.
//
// One work-item per pixel; a wave covers an 8x8 pixel tile (coherent rays), a 256-thread
// workgroup a 16x16 tile.  Per pixel the kernel runs trace_ray_through_pixel/3
// (raytracer.erl:180-184) and everything below it, in IEEE binary64 with the
// reference's operation order and no contraction (-ffp-contract=off + the pragma
// below): the geometry (every hit/miss decision, every hit point and normal) is
// bit-identical to the reference; colours differ from libm only where device pow()
// differs from the host's by an ulp.
//
// Work per hit level (the reference's recursion, raytracer.erl:186-252):
//   * one nearest-object scan (nearest_object_intersecting_ray/6, :303-346) — objects are
//     grouped by type, each type a wave-uniform loop reading its records with scalar
//     loads (uniform index -> s_load into SGPRs, the FP64 VALU reads them directly);
//   * per point light, diffuse + specular shading and one shadow test
//     (shadow_factor/4, :256-267).  The reference's test is "the nearest object seen
//     from the light is the hit object"; it is restated exactly as a bounded any-hit
//     test: with t* = the hit object's own distance along the shadow ray, the light is
//     blocked iff some object has a valid hit with t < t*, or t == t* and an earlier list
//     position.  That lets a lane stop at the first blocker and the wave leave the loop
//     as soon as every lane is decided (a wave-wide ballot).
// The reflection the reference recomputes once per light (:216-224) is the same value
// every time; it is computed once (ORDER_EXACT keeps the reference's summation order by
// shading the chain backwards from its deepest hit; ORDER_FAST accumulates forwards).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"
#include "rt_scene.h"

using namespace rtl;

namespace {

constexpr int BLOCK = 256; // 4 waves, 16x16 pixels

// Occupancy target (waves per SIMD); the default is chosen by measurement.
#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 4
#endif
constexpr int TILE = 16;

#include "rt_math.inc"     // binary64 primitives, the primitive tests
#include "rt_cull.inc"     // scene access, wave culling, candidate scans, per-lane BVH
#include "rt_shade.inc"    // nearest-object scans, shadow tests, shading
#include "rt_fused.inc"    // the fused engine (k_render)
#include "rt_wave.inc"     // the wavefront engine (default)
#include "rt_selftest.inc" // the arithmetic self-test kernels

} // namespace

// =====================================================================================
// C ABI
// =====================================================================================
struct rt_prepared {
    int device;
    SceneHdr hdr;      // what the kernels get: hdr_full, with the filters off when cull == 0
    SceneHdr hdr_full; // the compiled scene's header
    int cull = 1;      // rt_configure(RT_CFG_CULL)
    double *d_tab = nullptr;
    int *d_itab = nullptr;
    // wavefront-engine work space, grown on demand (one rt_launch in flight per rt_prepared):
    // grow, rt_trim and rt_release go through this one list
    enum Work {
        W_QUEUE,  // HitRec[slab pixels * depth]
        // double: colours of levels 1 .. depth-1, COL_W doubles per slot; inline-walk frames write none,
        // and those of LDS-staged scenes keep the per-light terms of levels 1 .. depth-2 here
        W_COLBUF,
        W_CHILD,  // uint8_t per level and slot: the record's reflection hit something
        W_LIT,    // unsigned per level and slot: shadow answers of lights 0..31 (k_light)
        W_SAMPLE, // double: supersampling, one sample's slab and the running sum
        W_COUNTS, // int per level and tile: queue lengths
        W_ITEMS,  // int: per-level record counts, then per-level dense slot lists
        // unsigned long long: primary rays' candidate masks per 8x16 pixel block of the slab (k_pmask),
        // kept while the frame geometry and the scene stay the same
        W_PMASK,
        W_COUNT
    };
    struct DevBuf { // a device buffer with its size
        void *ptr = nullptr;
        size_t bytes = 0;
    } work[W_COUNT];
    template <typename T>
    T *buf(Work w) const {
        return static_cast<T *>(work[w].ptr);
    }
    long long pmask_key[12] = {};
    bool pmask_valid = false;
    // the shadow pass runs on a second, low-priority stream beside the reflection chain
    // shading of level 0 and of the deeper levels.  The caller's stream plus these stay
    // within the hardware queues a process gets by default (GPU_MAX_HW_QUEUES=4): streams
    // sharing a queue block each other behind their event waits (measured: 5 streams, S64
    // 11 Gpx/s; 3 side streams were no faster than 2 — the chip is saturated in the overlap)
    hipStream_t side[2] = {};
    int side_mode = -1; // rt_configure(RT_CFG_SIDE_STREAMS): -1 = environment (RT_LIT_STREAM), 0 off, 1 on
    std::vector<hipEvent_t> ev_level; // level k's list is ready (depth + 1 of them, grown with the depth)
    std::vector<hipEvent_t> ev_lit;   // level k is shaded
    // Frames repeat with identical arguments (bench, multi-GPU renderer): the second identical
    // rt_launch captures the frame's launch sequence into a graph, later ones replay it.
    // gen counts changes that invalidate a captured frame: work-space reallocations (captured
    // pointers), new scene tables or header, and recomputed primary candidate masks (a graph
    // captured while they were valid holds no k_pmask launch).
    unsigned gen = 0;
    // scene_gen counts new scene tables and culling changes (the primary masks depend on them)
    unsigned scene_gen = 0;
    // RT_CFG_KERNEL_TIMING: per timed kernel (RT_KT_* bit i), a ring of event pairs; a full ring
    // folds its oldest pair into the sum (waiting for it)
    int timing_mask = 0;
    struct KTimer {
        std::vector<hipEvent_t> a, b;
        size_t head = 0, n = 0;
        double sum_ms = 0;
        unsigned long long count = 0;
    } kt[4];
    hipStream_t cap = nullptr;
    hipGraphExec_t gexec = nullptr;
    long long gkey[16] = {};
    long long last_key[16] = {};
    bool last_valid = false;
};

#define HIPCHK(x)                                                                                                  \
    do {                                                                                                           \
        hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) {                                                                                    \
            std::fprintf(stderr, "rt_mi355x: %s failed: %s\n", #x, hipGetErrorString(e_));                        \
            return RT_EHIP;                                                                                        \
        }                                                                                                          \
    } while (0)

namespace {

struct DevGuard { // restore the caller's current device on scope exit
    int prev = -1;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// RT_CFG_CULL = 0: every scan tests every object (no wave beams or cones, no occluder masks, no
// BVH, no LDS-staged tables, no host-proven skips of range checks) — the reference's brute-force
// scans, against which the filters' frames are checked bit for bit (tests/test_gpu_frames.py).
void apply_cull(rt_prepared *p) {
    p->hdr = p->hdr_full;
    if (!p->cull) {
        p->hdr.cull_ok = 0;
        p->hdr.occ_ok = 0;
        p->hdr.beam_ok = 0;
        p->hdr.bvh_ok = 0;
        p->hdr.l_bytes = 0;
        p->hdr.norm_ok = 0; // and every range check of normalize3 on
        p->hdr.prim_ok = 0;
    }
}

// The compiled scene's tables uploaded to p's device, then put in place of the ones p holds (none in
// a new context).  On failure p is unchanged and nothing is left allocated.
int upload_scene(rt_prepared *p, const Compiled &c) {
    DevGuard g(p->device);
    const size_t tab_bytes = c.tab.size() * sizeof(double), itab_bytes = c.itab.size() * sizeof(int);
    double *tab = nullptr;
    int *itab = nullptr;
    int rc = RT_OK;
    if (hipMalloc(&tab, tab_bytes) != hipSuccess || hipMalloc(&itab, itab_bytes) != hipSuccess)
        rc = RT_ENOMEM;
    else if (hipMemcpy(tab, c.tab.data(), tab_bytes, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(itab, c.itab.data(), itab_bytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = RT_EHIP;
    if (rc != RT_OK) {
        (void)hipFree(tab); // (a null pointer is a no-op)
        (void)hipFree(itab);
        return rc;
    }
    (void)hipFree(p->d_tab);
    (void)hipFree(p->d_itab);
    p->d_tab = tab;
    p->d_itab = itab;
    p->hdr_full = c.hdr;
    apply_cull(p);
    ++p->gen; // captured graphs hold the old tables
    ++p->scene_gen;
    p->last_valid = false;
    return RT_OK;
}

// Free the work space (rt_trim, rt_release); returns the bytes freed.
size_t free_work(rt_prepared *p) {
    size_t freed = 0;
    for (rt_prepared::DevBuf &b : p->work) {
        if (b.ptr) (void)hipFree(b.ptr);
        freed += b.bytes;
        b = rt_prepared::DevBuf{};
    }
    return freed;
}

// Work-space buffer w of at least `need` bytes; a reallocation invalidates captured frame graphs (gen).
int grow(rt_prepared *p, rt_prepared::Work w, size_t need) {
    rt_prepared::DevBuf &b = p->work[w];
    if (b.bytes >= need) return RT_OK;
    ++p->gen;
    if (b.ptr) (void)hipFree(b.ptr);
    b = rt_prepared::DevBuf{};
    if (hipMalloc(&b.ptr, need) != hipSuccess) {
        b.ptr = nullptr;
        return RT_ENOMEM;
    }
    b.bytes = need;
    return RT_OK;
}

constexpr size_t KT_RING = 64;
int kt_index(int kernel) {
    return kernel == RT_KT_PRIMARY ? 0 : kernel == RT_KT_LEVEL1 ? 1 : kernel == RT_KT_RENDER ? 2 : kernel == RT_KT_PMASK ? 3 : -1;
}
void kt_fold_oldest(rt_prepared::KTimer &t) {
    const size_t i = (t.head + KT_RING - t.n) % KT_RING;
    float ms = 0;
    if (hipEventSynchronize(t.b[i]) == hipSuccess && hipEventElapsedTime(&ms, t.a[i], t.b[i]) == hipSuccess) {
        t.sum_ms += ms;
        ++t.count;
    }
    --t.n;
}
// bracket one launch of `kernel` (an RT_KT_* bit) on `st` when the context times it
struct KtScope {
    rt_prepared::KTimer *t = nullptr;
    hipStream_t st;
    KtScope(rt_prepared *p, int kernel, hipStream_t s) : st(s) {
        if (!(p->timing_mask & kernel)) return;
        rt_prepared::KTimer &k = p->kt[kt_index(kernel)];
        if (k.a.empty()) {
            k.a.resize(KT_RING);
            k.b.resize(KT_RING);
            for (size_t i = 0; i < KT_RING; ++i)
                if (hipEventCreate(&k.a[i]) != hipSuccess || hipEventCreate(&k.b[i]) != hipSuccess) return;
        }
        if (k.n == KT_RING) kt_fold_oldest(k);
        if (hipEventRecord(k.a[k.head], st) != hipSuccess) return;
        t = &k;
    }
    ~KtScope() {
        if (!t) return;
        (void)hipEventRecord(t->b[t->head], st);
        t->head = (t->head + 1) % KT_RING;
        ++t->n;
    }
};

// ---- picking a kernel template: a run-time value handed to a generic lambda as a compile-time
// constant (a std::integral_constant argument c; decltype(c)::value is the template argument).
// Every helper returns what the lambda returns.
template <typename F>
auto with_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
// v in [LO, HI] (a value above HI is taken as HI)
template <int LO, int HI, typename F>
auto with_int(int v, F &&f) {
    if constexpr (LO < HI) {
        if (v != LO) return with_int<LO + 1, HI>(v, f);
    }
    return f(std::integral_constant<int, LO>{});
}
// f(PREC, GENPOW): the output precision (RT_OUT_F64 / RT_OUT_F32) and whether the scene needs the general pow
template <typename F>
auto with_prec_pow(int precision, bool int_pow, F &&f) {
    return with_int<RT_OUT_F64, RT_OUT_F32>(precision, [&](auto prec) {
        return with_bool(!int_pow, [&](auto genpow) { return f(prec, genpow); });
    });
}
// f(SPH): 2 = spheres only with the tables staged in LDS, 1 = spheres only, 0 = any scene
template <typename F>
auto with_sph(bool staged, bool sph_only, F &&f) {
    return with_int<0, 2>(staged ? 2 : sph_only ? 1 : 0, f);
}

template <int ORDER, int PREC, bool GENPOW>
int launch_t(rt_prepared *p, int W, int H, const ImageGeom &im, int depth, int rb, int shard, int nshards, int row0,
             int row_end, void *out, uint8_t *levels, hipStream_t st, int levels_hit) {
    dim3 grid((W + TILE - 1) / TILE, (row_end - row0 + TILE - 1) / TILE);
    size_t lds = ORDER == RT_ORDER_EXACT ? (size_t)depth * BLOCK * 12 + (size_t)BLOCK * 24 : 0;
    KtScope kt(p, RT_KT_RENDER, st);
    // scenes without wave beams (few spheres, e.g. the reference's own scene) take the beam-free build
    with_bool(levels != nullptr, [&](auto lv) {
        with_bool(!p->hdr.beam_ok, [&](auto nb) {
            hipLaunchKernelGGL((k_render<ORDER, PREC, decltype(lv)::value, GENPOW, decltype(nb)::value>), grid,
                               dim3(BLOCK), lds, st, p->hdr, p->d_tab, p->d_itab, W, H, depth, rb, shard, nshards, row0,
                               row_end, out, levels, levels_hit, im.IW, im.IH, im.x0, im.y0);
        });
    });
    HIPCHK(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

#ifdef RT_STATS
// diagnostic builds only (not part of include/rt_mi355x.h)
int rt_debug_stats(unsigned long long *out, int n, int reset) {
    if (n > RT_NSTATS) n = RT_NSTATS;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stats), n * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[RT_NSTATS] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stats), z, sizeof(z)));
    }
    return RT_OK;
}
#endif

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_selftest_math(int device, uint64_t n, uint64_t seed, uint64_t *mismatches) {
    if (!mismatches) return RT_EBADARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return RT_ENODEV;
    DevGuard g(device);
    unsigned long long *d = nullptr;
    if (hipMalloc(&d, sizeof(*d)) != hipSuccess) return RT_ENOMEM;
    int rc = RT_OK;
    if (hipMemset(d, 0, sizeof(*d)) != hipSuccess) rc = RT_EHIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_selftest_math, dim3(4096), dim3(256), 0, nullptr, (unsigned long long)n,
                           (unsigned long long)seed, d);
        unsigned long long h = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_EHIP;
        *mismatches = h;
    }
    (void)hipFree(d);
    return rc;
}

int rt_eval_math(int device, int op, uint64_t n, const double *a, const double *b, const uint8_t *act,
                 int32_t dim, double *out) {
    if (!a || !out || n == 0 || op < RT_EVAL_POW || op > RT_EVAL_IDIV_DIM) return RT_EBADARG;
    const bool two = op == RT_EVAL_POW || op == RT_EVAL_POW_GENERAL || op == RT_EVAL_DIV;
    if (two && !b) return RT_EBADARG;
    if ((op == RT_EVAL_DIV_DIM || op == RT_EVAL_IDIV_DIM) && (dim < 1 || dim > (1 << 20))) return RT_EBADARG;
    if (n > (1ull << 26)) return RT_ETOOBIG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return RT_ENODEV;
    DevGuard g(device);
    const size_t per = op == RT_EVAL_NORMALIZE3 ? 3 : 1, bytes = (size_t)n * per * sizeof(double);
    double *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    unsigned char *d_act = nullptr;
    int rc = RT_OK;
    if (hipMalloc(&d_a, bytes) != hipSuccess || hipMalloc(&d_out, bytes) != hipSuccess ||
        (two && hipMalloc(&d_b, bytes) != hipSuccess) ||
        (op == RT_EVAL_POW && act && hipMalloc(&d_act, (size_t)n) != hipSuccess))
        rc = RT_ENOMEM;
    if (rc == RT_OK && (hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                        (d_b && hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice) != hipSuccess) ||
                        (d_act && hipMemcpy(d_act, act, (size_t)n, hipMemcpyHostToDevice) != hipSuccess)))
        rc = RT_EHIP;
    if (rc == RT_OK) {
        const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
        with_int<RT_EVAL_POW, RT_EVAL_IDIV_DIM>(op, [&](auto opc) {
            hipLaunchKernelGGL(k_eval_math<decltype(opc)::value>, grid, blk, 0, nullptr, (unsigned long long)n, d_a, d_b,
                               d_act, (int)dim, d_out);
        });
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_EHIP;
    }
    (void)hipFree(d_a);
    (void)hipFree(d_b);
    (void)hipFree(d_out);
    (void)hipFree(d_act);
    return rc;
}

const char *rt_strerror(int code) {
    switch (code) {
    case RT_OK: return "ok";
    case RT_DONE: return "done (width = height = 0)";
    case RT_EBADARG: return "bad argument (malformed scene or sizes)";
    case RT_ENODEV: return "no HIP device / device index out of range";
    case RT_EHIP: return "HIP runtime error";
    case RT_ENOMEM: return "out of memory";
    case RT_ETOOBIG: return "size exceeds a library limit";
    case RT_ERANGE: return "a colour outside the device P3 formatter's range (below -2^31 after scaling)";
    default: return "unknown error";
    }
}

int rt_device_count(int *count) {
    if (!count) return RT_EBADARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n > 0 ? RT_OK : RT_ENODEV;
}

int rt_scene_check(const rt_elem *scene, uint32_t n) { return check_scene(scene, n); }

int rt_scene_canon(rt_elem *scene, uint32_t n) { return fill_canon(scene, n); }

uint32_t rt_shard_rows(uint32_t height, uint32_t row_block, uint32_t nshards) {
    if (row_block == 0 || nshards == 0) return 0;
    uint64_t span = (uint64_t)row_block * nshards;
    uint64_t blocks = (height + span - 1) / span;
    return (uint32_t)(blocks * row_block);
}

int rt_prepare(const rt_elem *scene, uint32_t n, int device, rt_prepared **out) {
    if (!out) return RT_EBADARG;
    *out = nullptr;
    Compiled c;
    int rc = compile_scene(scene, n, c);
    if (rc != RT_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RT_ENODEV;
    rt_prepared *p = new (std::nothrow) rt_prepared();
    if (!p) return RT_ENOMEM;
    p->device = device;
    if ((rc = upload_scene(p, c)) != RT_OK) { // an empty context on the device, then rt_prepare_scene's upload
        delete p;
        return rc;
    }
    *out = p;
    return RT_OK;
}

} // extern "C"

int rt_prepare_scene(rt_prepared *p, const rt_elem *scene, uint32_t n) {
    if (!p) return RT_EBADARG;
    Compiled c;
    int rc = compile_scene(scene, n, c);
    if (rc != RT_OK) return rc;
    return upload_scene(p, c);
}

extern "C" {

int rt_update_scene(rt_prepared *p, const rt_elem *scene, uint32_t n_elems) {
    return rt_prepare_scene(p, scene, n_elems);
}

int rt_configure(rt_prepared *p, int option, int64_t value) {
    if (!p) return RT_EBADARG;
    switch (option) {
    case RT_CFG_SIDE_STREAMS:
        if (value < -1 || value > 1) return RT_EBADARG;
        p->side_mode = (int)value;
        return RT_OK;
    case RT_CFG_KERNEL_TIMING:
        if (value < 0 || value > 15) return RT_EBADARG;
        p->timing_mask = (int)value;
        return RT_OK;
    case RT_CFG_CULL:
        if (value < 0 || value > 1) return RT_EBADARG;
        p->cull = (int)value;
        apply_cull(p);
        ++p->gen; // captured graphs hold the old header
        ++p->scene_gen;
        p->last_valid = false;
        return RT_OK;
    default:
        return RT_EBADARG;
    }
}

} // extern "C"


extern "C" {

int rt_kernel_time(rt_prepared *p, int kernel, double *total_ms, uint64_t *launches, int reset) {
    const int i = p ? kt_index(kernel) : -1;
    if (i < 0) return RT_EBADARG;
    DevGuard g(p->device);
    rt_prepared::KTimer &t = p->kt[i];
    while (t.n) kt_fold_oldest(t);
    if (total_ms) *total_ms = t.sum_ms;
    if (launches) *launches = t.count;
    if (reset) {
        t.sum_ms = 0;
        t.count = 0;
    }
    return RT_OK;
}

int rt_release(rt_prepared *p) {
    if (!p) return RT_EBADARG;
    DevGuard g(p->device);
    (void)hipFree(p->d_tab);
    (void)hipFree(p->d_itab);
    free_work(p);
    for (hipEvent_t &e : p->ev_level)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t &e : p->ev_lit)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t &x : p->side)
        if (x) (void)hipStreamDestroy(x);
    if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
    if (p->cap) (void)hipStreamDestroy(p->cap);
    for (auto &t : p->kt) {
        for (hipEvent_t e : t.a) (void)hipEventDestroy(e);
        for (hipEvent_t e : t.b) (void)hipEventDestroy(e);
    }
    delete p;
    return RT_OK;
}

} // extern "C"

// Free the wavefront work space of an idle context (rt_internal.h); the next launch regrows it.
size_t rt_trim(rt_prepared *p) {
    if (!p) return 0;
    DevGuard g(p->device);
    const size_t freed = free_work(p);
    p->pmask_valid = false;
    ++p->gen; // captured frame graphs hold the old pointers
    return freed;
}

namespace {

// Queue memory per pass is bounded (RT_QUEUE_MB, default 8 GiB); taller slabs are rendered
// in several row passes.
size_t queue_budget() {
    static size_t b = [] {
        const char *s = std::getenv("RT_QUEUE_MB");
        size_t mb = s ? std::strtoull(s, nullptr, 10) : 8192;
        return (mb < 64 ? 64 : mb) << 20;
    }();
    return b;
}

// Shading beside the reflection chain on the context's two side streams: per context
// (rt_configure RT_CFG_SIDE_STREAMS), else RT_LIT_STREAM=0 turns it off, for A/B runs.
bool lit_overlap(const rt_prepared *p) {
    static bool env_on = [] {
        const char *s = std::getenv("RT_LIT_STREAM");
        return !(s && std::strcmp(s, "0") == 0);
    }();
    return p->side_mode < 0 ? env_on : p->side_mode != 0;
}

// The side streams and one pair of level events per level 0 .. depth (created once, grown with the depth).
int side_stream(rt_prepared *p, int depth) {
    if (!p->side[0]) {
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        for (hipStream_t &x : p->side) HIPCHK(hipStreamCreateWithPriority(&x, hipStreamNonBlocking, least));
    }
    while (p->ev_level.size() < (size_t)depth + 1) {
        hipEvent_t a = nullptr, b = nullptr;
        HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        if (hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(a);
            return RT_EHIP;
        }
        p->ev_level.push_back(a);
        p->ev_lit.push_back(b);
    }
    return RT_OK;
}

// The slab rows of shard sh that lie inside the image (a prefix of the slab).
size_t valid_slab_rows(int H, int rb, int sh, int ns) {
    const size_t slab = rt_shard_rows((uint32_t)H, (uint32_t)rb, (uint32_t)ns);
    size_t v = 0;
    for (size_t blk = 0; blk * rb < slab; ++blk) {
        const long long base = ((long long)blk * ns + sh) * rb;
        v += (size_t)std::max(0LL, std::min((long long)rb, (long long)H - base));
    }
    return v;
}

// Does a wavefront pass write every pixel exactly once?  Yes with k_reflect_shade (the colours of
// records with a reflection hit are left to k_walk) and without reflections; no when k_light
// shades level 0 provisionally beside the chain (side streams, or levels requested).
bool wave_single_write(const rt_prepared *p, int D, bool levels) {
    const int nrefl = (p->hdr.n_light > 0 && D > 1) ? D - 1 : 0;
    const bool overlap = lit_overlap(p) && D > 1 && p->hdr.n_light > 0;
    return nrefl == 0 || (!overlap && !levels);
}

// acc (slab row 0, binary64, or null): supersampled passes fold their sample into it where each
// pixel is written (put_pixel) — only valid when wave_single_write holds.  keep (RT_PROGRESSIVE):
// such a pass only accumulates, whatever its sample — `out` is then never written.
// W x H is the raster the call renders (slabs, tiles, queues and stores are sized on it): a window
// of the image `im`, the whole frame being {W, H, 0, 0}.
template <int PREC, bool GENPOW>
int launch_wavefront(rt_prepared *p, int W, int H, const ImageGeom &im, int D, int rb, int sh, int ns, int row_begin,
                     int row_end, void *out, uint8_t *levels, hipStream_t st, int spp = 1, int sample = 0,
                     unsigned long long seed = 0, double *acc = nullptr, int levels_hit = 0, bool keep = false) {
    // renders slab rows [row_begin, row_end) (row_begin a multiple of TILE); out / levels point at slab row 0.
    // levels_hit: k_primary writes the primary-hit mask (what it always writes: 1 on a hit, 0 on a
    // miss) and the later kernels do not count levels, so the fused path stays on
    uint8_t *const levels_primary = levels;
    const SceneHdr &hdr = p->hdr;
    if (levels_hit) levels = nullptr;
    const int slab_rows = row_end - row_begin;
    const int nlev = D > 0 ? D : 1;
    const size_t per_row = (size_t)W * nlev * sizeof(HitRec);
    int pass_rows = (int)std::min<size_t>((size_t)slab_rows, std::max<size_t>(TILE, queue_budget() / per_row));
    pass_rows = std::max(TILE, pass_rows / TILE * TILE);
    if (pass_rows > slab_rows) pass_rows = slab_rows;
    const int tiles_x = (W + TILE - 1) / TILE;
    const size_t max_tiles = (size_t)tiles_x * ((pass_rows + TILE - 1) / TILE);
    const size_t slots = max_tiles * TILE_SLOTS; // per level
    int rc = grow(p, rt_prepared::W_QUEUE, slots * nlev * sizeof(HitRec));
    // colours of levels 1 .. depth-1, COL_W doubles per slot (level 0 goes straight to the
    // frame), and per level the has-a-child flags
    const size_t col_doubles = slots * COL_W * (size_t)std::max(1, nlev - 1);
    const bool overlap = lit_overlap(p) && D > 1 && p->hdr.n_light > 0;
    const int nrefl = (p->hdr.n_light > 0 && D > 1) ? D - 1 : 0;
    // no side streams (frames in flight): each level's shading fused into the next reflection
    // pass (k_reflect_shade)
    const bool fuse = !overlap && !levels && nrefl > 0;
    // Inline walks (k_reflect_shade's iw, levels >= 1): every level is shaded by the launch that
    // reflects it; the chain of a shaded record without a child is walked by that launch, and the
    // deepest level's hits are shaded and walked by the launch that finds them (not queued) — what
    // k_walk did, minus its launch, the deepest level's k_items, the terminal records' colour entries
    // and their re-reads.  Needs the shadow answers in the records (<= 32 lights) and two reflection
    // levels or more (level 1's kernel, the dominant one, is left as is).  For S64 the dense
    // arrangement this implies measured the same as the sparse one (profiles/r05aa_ab_memset_dense.txt).
    const bool iw = fuse && p->hdr.n_light <= 32 && nrefl >= 2;
    // spheres only, culling on: every shadow target has occluder masks (lit_by<1>); their
    // per-lane-gathered tables staged in each workgroup's LDS when they fit (SPH = 2)
    const bool sph_only = p->hdr.n_tri == 0 && p->hdr.n_pl == 0 && p->hdr.cull_ok && p->hdr.occ_ok;
    const bool staged = sph_only && p->hdr.l_bytes > 0;
    // ... and for LDS-staged scenes of up to TERM_MAX_LIGHTS lights those walks fold the child's
    // colour into per-light terms stored at the first shading instead of shading again (walk_fold):
    // one entry per slot of the queued levels 1 .. nrefl-1.  An inline-walk launch writes no colour
    // entries, so the entries take the colour buffer, grown to the larger of its two uses.  (Staged
    // scenes only: S256 depth 8 with its tables in L2 and dense deep levels measured 2.7 % slower per
    // frame with the entries than reshading, profiles/terms_ab_c3.txt; only the SPH = 2 kernels
    // compile the entries in.)
    const bool fold = iw && staged && p->hdr.n_light <= TERM_MAX_LIGHTS;
    const size_t term_bytes =
        fold ? slots * (size_t)(nrefl - 1) * term_stride(p->hdr.n_light) * sizeof(double2) : 0;
    if (rc == RT_OK) rc = grow(p, rt_prepared::W_COLBUF, std::max(col_doubles * sizeof(double), term_bytes));
    if (rc == RT_OK) rc = grow(p, rt_prepared::W_CHILD, slots * nlev);
    if (rc == RT_OK) rc = grow(p, rt_prepared::W_LIT, slots * nlev * sizeof(unsigned));
    if (rc == RT_OK) rc = grow(p, rt_prepared::W_COUNTS, max_tiles * nlev * sizeof(int));
    // dense work lists: 64 per-level record counts, then per level the slots of its records in tile order
    const size_t list0 = level_counts(nlev);
    const size_t items_ints = list0 + slots * nlev;
    if (rc == RT_OK) rc = grow(p, rt_prepared::W_ITEMS, items_ints * sizeof(int));
    if (rc == RT_OK && overlap) rc = side_stream(p, D);
    if (rc != RT_OK) return rc;
    // the primary rays' candidate masks of the whole slab (k_pmask), recomputed only when the
    // frame geometry — the raster's and the image's: two windows of one size at different origins
    // see different rays — or the scene changed (or after rt_trim)
    const unsigned long long *pmask = nullptr;
    const unsigned short *pempty = nullptr; // after the masks: one byte per half-tile, 1 = every mask zero
    if (p->hdr.beam_ok && D > 0) {
        const int slab_all = (int)rt_shard_rows(H, rb, ns);
        const size_t nhalf = (size_t)tiles_x * ((slab_all + TILE - 1) / TILE) * 2;
        const long long key[12] = {W, H, rb, sh, ns, spp > 1, (long long)p->scene_gen, slab_all, im.IW, im.IH, im.x0, im.y0};
        if (!(p->pmask_valid && std::memcmp(key, p->pmask_key, sizeof(key)) == 0)) {
            p->pmask_valid = false;
            // New masks (and perhaps a new buffer): a frame graph captured with the old ones holds
            // no k_pmask launch and would read these, so it is invalidated (gen).
            ++p->gen;
            if ((rc = grow(p, rt_prepared::W_PMASK, nhalf * p->hdr.n_chunk * 8 + nhalf)) != RT_OK) return rc;
            const dim3 pg((unsigned)std::min<size_t>(4096, (nhalf + 3) / 4));
            KtScope kt(p, RT_KT_PMASK, st);
            with_bool(spp > 1, [&](auto ss) {
                hipLaunchKernelGGL(k_pmask<decltype(ss)::value>, pg, dim3(256), 0, st, hdr, p->d_tab, p->d_itab, W, H,
                                   rb, sh, ns, slab_all, (int)nhalf, p->buf<unsigned long long>(rt_prepared::W_PMASK),
                                   reinterpret_cast<unsigned char *>(p->buf<unsigned long long>(rt_prepared::W_PMASK) +
                                                           nhalf * p->hdr.n_chunk),
                                   im);
            });
            HIPCHK(hipGetLastError());
            std::memcpy(p->pmask_key, key, sizeof(key));
            p->pmask_valid = true;
        }
        pmask = p->buf<unsigned long long>(rt_prepared::W_PMASK);
        pempty = reinterpret_cast<const unsigned short *>(pmask + nhalf * p->hdr.n_chunk);
    }
    // streams of the shading pass: level 0 (the bulk) beside the whole reflection chain, the
    // next levels each on their own, so no level waits for another's shading
    auto ls = [&](int k) { return overlap ? p->side[std::min(k, 1)] : st; };
    HitRec *const q = p->buf<HitRec>(rt_prepared::W_QUEUE);
    double *const d_colbuf = p->buf<double>(rt_prepared::W_COLBUF);
    uint8_t *const d_child = p->buf<uint8_t>(rt_prepared::W_CHILD);
    unsigned *const d_lit = p->buf<unsigned>(rt_prepared::W_LIT);
    int *const d_counts = p->buf<int>(rt_prepared::W_COUNTS);
    int *const d_items = p->buf<int>(rt_prepared::W_ITEMS);
    const int nshade = D > 0 ? 1 + nrefl : 0;
    const size_t lds = staged ? (size_t)p->hdr.l_bytes : 0; // the SPH = 2 kernels' dynamic LDS; 0 for SPH < 2
    // Reflection kernels of levels that traverse the sphere BVH: after the staged tables in LDS,
    // the BVH nodes and sphere rows (when they fit BVH_LDS_MAX) and every lane's stack.
    SceneHdr rhdr = hdr;
    size_t lds_bvh = lds;
    if (rhdr.bvh_ok) {
        const size_t nb = (size_t)rhdr.n_bvh * BVH_NODE_DOUBLES * 8, sb = (size_t)rhdr.n_sph * SPH_W * 8;
        if (nb + sb <= (size_t)BVH_LDS_MAX) {
            rhdr.l_bvh = (int)lds_bvh;
            rhdr.l_bsph = (int)(lds_bvh + nb);
            lds_bvh += nb + sb;
        }
        rhdr.l_stack = (int)lds_bvh;
        lds_bvh += (size_t)BLOCK * rhdr.bvh_depth * sizeof(unsigned);
    }
    // (LDS-staged scenes keep the candidate walks: their tables and the BVH would not fit together)
    auto bvh_at = [&](int k) { return !staged && rhdr.bvh_ok && k >= rhdr.bvh_level; };
    auto lds_r = [&](int k) { return bvh_at(k) ? lds_bvh : lds; };
    double2 *const d_terms = fold ? reinterpret_cast<double2 *>(d_colbuf) : nullptr;
    for (int row0 = row_begin; row0 < row_end; row0 += pass_rows) {
        const int rows = std::min(pass_rows, row_end - row0);
        const int ntiles = tiles_x * ((rows + TILE - 1) / TILE);
        // the pass covers slab rows [row0, row0 + rows): out/levels offset to row0; the
        // kernels map slab rows to image rows through the shard interleave themselves
        const size_t off = (size_t)row0 * W;
        void *o = static_cast<char *>(out) + off * 3 * (PREC == RT_OUT_F64 ? 8 : 4);
        uint8_t *lv = levels ? levels + off : nullptr;
        uint8_t *lv0 = levels_primary ? levels_primary + off : nullptr; // k_primary's
        double *acc_p = acc ? acc + off * 3 : nullptr;
        auto qk = [&](int k) { return q + (size_t)k * ntiles * TILE_SLOTS; };
        auto ck = [&](int k) { return d_counts + (size_t)k * ntiles; };
        int *nitems = d_items; // [0, 64): per-level record counts
        int *lists = d_items + list0;
        auto ik = [&](int k) { return lists + (size_t)k * ntiles * TILE_SLOTS; };
        auto colk = [&](int k) { return k > 0 ? d_colbuf + (size_t)(k - 1) * ntiles * TILE_SLOTS * COL_W : nullptr; };
        auto chk = [&](int k) { return d_child + (size_t)k * ntiles * TILE_SLOTS; };
        auto litk = [&](int k) { return d_lit + (size_t)k * ntiles * TILE_SLOTS; };
        const dim3 iblocks((ntiles + ITEMS_BLOCK - 1) / ITEMS_BLOCK);
        const int smp = sample_arg(sample, keep);
        const PassGeom g = make_pass_geom(W, im, rb, sh, ns, row0, spp, smp, seed, acc_p); // level-0 records are rebuilt from it
        const dim3 grid(std::min(ntiles, PRIMARY_GRID)); // k_primary: grid-stride loop over the tiles
        {
            KtScope kt(p, RT_KT_PRIMARY, st);
            with_bool(lv0 != nullptr, [&](auto has_lv) { // (without lv0 there is no lv either)
                hipLaunchKernelGGL((k_primary<PREC, decltype(has_lv)::value>), grid, dim3(PRIMARY_BLOCK), 0, st, hdr,
                                   p->d_tab, p->d_itab, W, im.y0 + H, D, rb, g.yoff, ns, rows, row0, o, lv0, q, d_counts, ntiles,
                                   spp, smp, seed, acc_p, pmask, pempty, nitems, g.img);
            });
        }
        HIPCHK(hipGetLastError());
        const int sblocks = std::min<int>(STRIDE_BLOCKS, (ntiles * (TILE_SLOTS / 64) + BLOCK / 64 - 1) / (BLOCK / 64));
        const int sblocks1 = std::min<int>(STRIDE_BLOCKS_L1, (ntiles * (TILE_SLOTS / 64) + BLOCK / 64 - 1) / (BLOCK / 64));
        const int sblocksw = std::min<int>(STRIDE_BLOCKS_WALK, (ntiles * (TILE_SLOTS / 64) + BLOCK / 64 - 1) / (BLOCK / 64));
        const int sblocksb = std::min<int>(STRIDE_BLOCKS_BVH, (ntiles * (TILE_SLOTS / 64) + BLOCK / 64 - 1) / (BLOCK / 64));
        // level k's dense list, then its shading (k_light reads only level k: on a side stream
        // it starts as soon as the list exists and runs beside the next reflections)
        auto level_lists = [&](int k) -> int {
            // (inline walks: the deepest level is shaded by the launch that finds its hits, never queued)
            if (iw && k == nrefl) return RT_OK;
            hipLaunchKernelGGL(k_items, iblocks, dim3(ITEMS_BLOCK), 0, st, ck(k), ntiles, ik(k), nitems + k);
            HIPCHK(hipGetLastError());
            if (overlap) {
                HIPCHK(hipEventRecord(p->ev_level[k], st));
                HIPCHK(hipStreamWaitEvent(ls(k), p->ev_level[k], 0));
            }
            if (fuse && k < nrefl) return RT_OK; // shaded by k_reflect_shade(k + 1)
            if (k == nrefl && k >= 2) { // the deepest level >= 2: shaded by k_walk_deep / k_walk
                if (overlap) HIPCHK(hipEventRecord(p->ev_lit[k], ls(k)));
                return RT_OK;
            }
            // levels >= 2 are shaded here only when dense (decided on the device; otherwise the
            // launch exits at once): a smaller persistent grid keeps the empty launch cheap
            const int lblocks = k >= 2 ? std::min(sblocks, DEEP_LIGHT_BLOCKS) : sblocks;
            with_sph(staged, sph_only, [&](auto sph) {
                hipLaunchKernelGGL((k_light<PREC, GENPOW, decltype(sph)::value>), dim3(lblocks), dim3(BLOCK), lds, ls(k),
                                   hdr, p->d_tab, p->d_itab, k, o, qk(k), ik(k), nitems + k, colk(k), litk(k), g);
            });
            HIPCHK(hipGetLastError());
            if (overlap) HIPCHK(hipEventRecord(p->ev_lit[k], ls(k)));
            return RT_OK;
        };
        if (nshade > 0 && (rc = level_lists(0)) != RT_OK) return rc;
        for (int k = 1; k <= nrefl; ++k) {
            // level 1 (from the primary hits) is dense and throughput-bound; deeper levels are a few
            // waves each, bound by one wave's dependent chain: they walk two candidates per step
            KtScope kt(p, k == 1 ? RT_KT_LEVEL1 : 0, st);
            if (fuse) {
                // levels traversing the sphere BVH (unstaged scenes only) take the BVH instantiations,
                // the deepest level with inline walks the LAST ones; both only come with ILP
                const bool bvh_k = bvh_at(k), ilp = bvh_k || k != 1, last = ilp && iw && k == nrefl;
                with_sph(staged, sph_only, [&](auto sph) {
                    constexpr int SPH = decltype(sph)::value;
                    auto rs = [&](auto ilp_c, auto bvh_c, auto last_c) {
                        constexpr bool BVH = decltype(bvh_c)::value;
                        hipLaunchKernelGGL(
                            (k_reflect_shade<PREC, GENPOW, SPH, decltype(ilp_c)::value, BVH, decltype(last_c)::value>),
                            dim3(k == 1 ? sblocks1 : BVH ? sblocksb : sblocks), dim3(BLOCK), lds_r(k), st, rhdr, p->d_tab,
                            p->d_itab, k, o, qk(k - 1), ik(k - 1), nitems + (k - 1), qk(k), ck(k), iw ? nullptr : chk(k - 1),
                            colk(k - 1), g, iw && k >= 2 ? (k == nrefl ? 2 : 1) : 0, d_terms);
                    };
                    auto rs_ilp = [&](auto bvh_c) {
                        with_bool(last, [&](auto last_c) { rs(std::true_type{}, bvh_c, last_c); });
                    };
                    if (!ilp) rs(std::false_type{}, std::false_type{}, std::false_type{});
                    else if constexpr (SPH == 2) rs_ilp(std::false_type{}); // (staged: never the BVH, bvh_at)
                    else with_bool(bvh_k, rs_ilp);
                });
            } else {
                with_bool(lv != nullptr, [&](auto has_lv) {
                    with_bool(k != 1, [&](auto ilp_c) {
                        hipLaunchKernelGGL((k_reflect<decltype(has_lv)::value, decltype(ilp_c)::value>), dim3(sblocks),
                                           dim3(BLOCK), lds, st, rhdr, p->d_tab, p->d_itab, k, qk(k - 1), ik(k - 1),
                                           nitems + (k - 1), qk(k), ck(k), lv, chk(k - 1), g);
                    });
                });
            }
            HIPCHK(hipGetLastError());
            if ((rc = level_lists(k)) != RT_OK) return rc;
        }
        // Without side streams one k_walk finishes every chain (sparse deep levels shaded on the
        // way).  With side streams (see deep_dense): k_walk_deep right after the chain; the chains
        // ending at level 1 (the bulk) are finished on side stream 0 as soon as levels 0 and 1 are
        // shaded, beside it; then the rest, once every level's shading is in (side stream 1
        // shades levels 1.. in order: its last level's event covers them all)
        if (nrefl > 0) {
            const size_t ls_ = (size_t)ntiles * TILE_SLOTS;
            const bool bits = p->hdr.n_light <= 32; // the shadow answers fit the record
            // deep: the merged walk (no k_walk_deep; without side streams); after k_reflect_shade
            // (fuse) the shadow answers are in the children's records (PAD)
            auto walk = [&](hipStream_t s_, int lo, int hi, bool deep) {
                with_sph(staged, sph_only, [&](auto sph) {
                    with_bool(bits, [&](auto bits_c) {
                        auto launch = [&](auto deep_c, auto pad_c) {
                            hipLaunchKernelGGL((k_walk<PREC, GENPOW, decltype(sph)::value, decltype(bits_c)::value,
                                                       decltype(deep_c)::value, decltype(pad_c)::value>),
                                               dim3(sblocksw), dim3(BLOCK), lds, s_, hdr, p->d_tab, p->d_itab, D, o, q,
                                               ls_, lists, nitems, d_colbuf, d_child, d_lit, lo, hi, g);
                        };
                        // (PAD is launched with DEEP and BITS only; its instantiations without BITS
                        // exist, as they always have, and are never run)
                        if (deep && fuse && bits) launch(std::true_type{}, std::true_type{});
                        else if (deep) launch(std::true_type{}, std::false_type{});
                        else launch(std::false_type{}, std::false_type{});
                    });
                });
            };
            if (overlap) { // side stream 0 (after level 0's shading) waits for level 1's, and for
                           // k_reflect(2), which marks the level-1 records that have a child
                HIPCHK(hipStreamWaitEvent(p->side[0], p->ev_lit[1], 0));
                if (D > 2) HIPCHK(hipStreamWaitEvent(p->side[0], p->ev_level[2], 0));
                walk(p->side[0], 1, 2, false);
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(p->ev_lit[0], p->side[0]));
            }
            if (D > 2 && overlap) {
                with_sph(staged, sph_only, [&](auto sph) {
                    hipLaunchKernelGGL((k_walk_deep<GENPOW, decltype(sph)::value>), dim3(sblocks), dim3(BLOCK), lds, st,
                                       hdr, p->d_tab, p->d_itab, D, q, ls_, lists, nitems, d_child, colk(2));
                });
                HIPCHK(hipGetLastError());
            }
            if (overlap) {
                HIPCHK(hipStreamWaitEvent(st, p->ev_lit[nrefl], 0));
                HIPCHK(hipStreamWaitEvent(st, p->ev_lit[0], 0));
                if (D > 2) walk(st, 2, D, false);
            } else if (!iw) {
                walk(st, 1, D, true); // every chain in one launch, sparse deep levels shaded there too
            }
            HIPCHK(hipGetLastError());
        } else if (overlap && nshade > 0) {
            HIPCHK(hipStreamWaitEvent(st, p->ev_lit[0], 0));
        }
    }
    return RT_OK;
}

// RT_GRAPH=1 enables frame graphs.  Off by default: measured on MI355X (ROCm 7), replaying
// the captured frame ran its kernels slower than direct launches (S64 4096^2: 1.35 vs 0.94
// ms), the side stream's low priority does not survive capture.
bool graphs_on() {
    static bool on = [] {
        const char *s = std::getenv("RT_GRAPH");
        return s && std::strcmp(s, "1") == 0;
    }();
    return on;
}

// Run enqueue(stream) for a frame: directly, or through the cached graph of identical frames.
template <typename F>
int launch_frame(rt_prepared *p, const long long (&args)[16], hipStream_t st, F &&enqueue) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!graphs_on() || hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
        return enqueue(st); // the caller is capturing (or graphs are off): plain launches
    long long key[16];
    std::memcpy(key, args, sizeof(key));
    key[15] = (long long)p->gen; // a reallocated work space invalidates captured pointers
    auto same = [&](const long long (&a)[16]) { return std::memcmp(a, key, sizeof(key)) == 0; };
    if (p->gexec && same(p->gkey)) {
        HIPCHK(hipGraphLaunch(p->gexec, st));
        return RT_OK;
    }
    if (!(p->last_valid && same(p->last_key))) { // first time with these arguments: run directly
        const int rc = enqueue(st);
        std::memcpy(p->last_key, key, sizeof(key));
        p->last_key[15] = (long long)p->gen;
        p->last_valid = rc == RT_OK;
        return rc;
    }
    // second identical frame (work space already sized): capture it on an internal stream
    if (!p->cap) HIPCHK(hipStreamCreateWithFlags(&p->cap, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(p->cap, hipStreamCaptureModeRelaxed));
    const int rc = enqueue(p->cap);
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(p->cap, &gr);
    if (rc == RT_OK && e == hipSuccess && (long long)p->gen != key[15]) {
        // the work space or the primary masks changed while capturing: no device work was run —
        // drop the graph and render this frame directly.  The host state the capture changed is
        // reset first: primary masks computed during the capture were never written (their k_pmask
        // launch is in the dropped graph), so the direct run must compute them again.
        (void)hipGraphDestroy(gr);
        p->last_valid = false;
        p->pmask_valid = false;
        return enqueue(st);
    }
    if (rc != RT_OK || e != hipSuccess) {
        if (gr) (void)hipGraphDestroy(gr);
        p->last_valid = false;
        return rc != RT_OK ? rc : RT_EHIP;
    }
    if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
    p->gexec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&p->gexec, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    if (ei != hipSuccess) {
        p->gexec = nullptr;
        return RT_EHIP;
    }
    std::memcpy(p->gkey, key, sizeof(key));
    HIPCHK(hipGraphLaunch(p->gexec, st));
    return RT_OK;
}

// Engine.  Small mixed scenes are bound by per-level latency (every level of the wavefront
// pipeline costs its kernels' fixed ramp-up) and run fastest as the single fused kernel
// (default scene 1920x1080 d5: 15.1 vs 6.1 Gpx/s); larger ones by the scans, where the wavefront
// pipeline's coherent waves and overlap win (round 1, 4096^2 d5: wavefront ahead from 48
// objects), and spheres-only scenes with LDS-staged tables at any size (below).
// RT_ENGINE=fused | wave forces one.
constexpr int FUSED_MAX_OBJECTS = 40;
// The fused kernel's reference-order chain keeps each level's (t, object) per pixel in LDS (12 bytes
// per level and pixel): deeper frames in reference order take the wavefront engine, whose per-level
// queues are sized at run time (launch_wavefront).
constexpr int FUSED_MAX_DEPTH = 16;
bool use_mega_engine(const rt_prepared *p, int depth = 0, int order = RT_ORDER_EXACT) {
    if (order == RT_ORDER_EXACT && depth > FUSED_MAX_DEPTH) return false;
    static const int mode = [] { // 0 auto, 1 fused, 2 wave
        const char *s = std::getenv("RT_ENGINE");
        if (s && (std::strcmp(s, "fused") == 0 || std::strcmp(s, "mega") == 0)) return 1;
        if (s && std::strcmp(s, "wave") == 0) return 2;
        return 0;
    }();
    if (mode) return mode == 1;
    // spheres-only scenes whose tables are staged in LDS: the wavefront engine at every size
    // (measured round 2, 4096^2 d5, 4 frames in flight: S4 115 vs 89 Gpx/s, S8 86 vs 70,
    // S16 58 vs 42, S24 49 vs 37, S32 52 vs 38).  Decided from the compiled header, not the one
    // RT_CFG_CULL = 0 strips, so the brute-force mode runs the production engine.
    const SceneHdr &h = p->hdr_full;
    if (h.n_tri == 0 && h.n_pl == 0 && h.cull_ok && h.l_bytes > 0) return false;
    return h.n_obj <= FUSED_MAX_OBJECTS;
}

} // namespace

extern "C" {

int rt_engine(rt_prepared *p, uint32_t spp) {
    if (!p || spp == 0) return RT_EBADARG;
    return (spp == 1 && use_mega_engine(p)) ? RT_ENGINE_FUSED : RT_ENGINE_WAVE;
}

int rt_launch(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t row_block, uint32_t shard,
              uint32_t nshards, int precision, int order, void *d_out, uint8_t *d_levels, void *stream) {
    return rt_launch_spp(p, width, height, depth, row_block, shard, nshards, precision, order, 1, 0, d_out, d_levels,
                         stream);
}

int rt_launch_spp(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t row_block,
                  uint32_t shard, uint32_t nshards, int precision, int order, uint32_t spp, uint64_t seed,
                  void *d_out, uint8_t *d_levels, void *stream) {
    return rt_launch_window(p, width, height, depth, 0, 0, width, height, row_block, shard, nshards, precision, order,
                            spp, seed, d_out, d_levels, stream);
}

int rt_launch_window(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                     uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, int precision,
                     int order, uint32_t spp, uint64_t seed, void *d_out, uint8_t *d_levels, void *stream) {
    return rt_launch_rows(p, width, height, depth, x0, y0, win_w, win_h, row_block, shard, nshards, precision, order, spp,
                          seed, 0, ~0u, d_out, d_levels, stream, 0);
}

} // extern "C"

namespace {

// The size, shard and window checks of rt_launch_window and rt_launch_samples, in one place so that
// they are the same: RT_OK, RT_DONE or an error; nothing is dereferenced and no HIP call is made.
int launch_args_check(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t win_w, uint32_t win_h,
                      uint32_t row_block, uint32_t shard, uint32_t nshards, int precision, int order, uint32_t spp) {
    if (width == 0 && height == 0 && win_w == 0 && win_h == 0 && x0 == 0 && y0 == 0) return RT_DONE;
    if (width == 0 || height == 0) return RT_EBADARG;
    if (row_block == 0 || nshards == 0 || shard >= nshards) return RT_EBADARG;
    if (precision != RT_OUT_F64 && precision != RT_OUT_F32) return RT_EBADARG;
    if (order != RT_ORDER_EXACT && order != RT_ORDER_FAST) return RT_EBADARG;
    if (spp == 0) return RT_EBADARG;
    if (spp > RT_MAX_SPP) return RT_ETOOBIG;
    if (width > (1u << 20) || height > (1u << 20)) return RT_ETOOBIG;
    // the window: not empty, inside the image (sums in 64 bits: x0 + win_w may pass 2^32)
    if (win_w == 0 || win_h == 0) return RT_EBADARG;
    if ((uint64_t)x0 + win_w > width || (uint64_t)y0 + win_h > height) return RT_EBADARG;
    if ((uint64_t)rt_shard_rows(win_h, row_block, nshards) > 65535ull * TILE) return RT_ETOOBIG;
    return RT_OK;
}

} // namespace

// rt_launch_window restricted to slab rows [row_begin, min(row_end, slab rows)) of the window: the
// boundary (rt_host.hip) renders a frame in row bands so that each band's copy to the host overlaps
// the next band's render.  row_begin must be a multiple of 16 (the tile height).  From here on
// (W, H) is the raster the kernels tile and store — the window — and `im` the image it lies in.
int rt_launch_rows(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                   uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, int precision,
                   int order, uint32_t spp, uint64_t seed, uint32_t row_begin, uint32_t row_end, void *d_out,
                   uint8_t *d_levels, void *stream, int levels_hit) {
    if (!p || !d_out) return RT_EBADARG;
    const int ok = launch_args_check(width, height, x0, y0, win_w, win_h, row_block, shard, nshards, precision, order, spp);
    if (ok != RT_OK) return ok;
    const ImageGeom im{(int)width, (int)height, (int)x0, (int)y0};
    uint32_t slab = rt_shard_rows(win_h, row_block, nshards);
    if (row_begin % TILE) return RT_EBADARG;
    if (row_end > slab) row_end = slab;
    if (row_begin >= row_end) return RT_OK;
    DevGuard g(p->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int W = (int)win_w, H = (int)win_h, D = (int)depth, rb = (int)row_block, sh = (int)shard, ns = (int)nshards;
    const int r0 = (int)row_begin, r1 = (int)row_end, slab_rows = (int)slab;
    if (spp > 1) { // RT_SUPERSAMPLING, on the wavefront engine: one pass per sample, summed in order
        // the slab rows inside the image (a prefix: global rows grow with slab rows)
        const size_t valid_rows = valid_slab_rows(H, rb, sh, ns);
        const size_t v1 = std::min<size_t>(valid_rows, (size_t)r1);
        if (v1 <= (size_t)r0) return RT_OK;
        const size_t e0 = (size_t)r0 * W * 3, n = (v1 - r0) * W * 3; // the band's elements
        const size_t n_slab = (size_t)slab_rows * W * 3;
        int rc = grow(p, rt_prepared::W_SAMPLE, 2 * n_slab * sizeof(double));
        if (rc != RT_OK) return rc;
        double *smp = p->buf<double>(rt_prepared::W_SAMPLE), *acc = smp + n_slab;
        const int blocks = (int)std::min<size_t>(8192, (n + 255) / 256);
        void *dst = static_cast<char *>(d_out) + e0 * (precision == RT_OUT_F64 ? 8 : 4);
        for (int s = 0; s < (int)spp; ++s) {
            uint8_t *lv = s == 0 ? d_levels : nullptr;
            // every pixel written once: the pass folds its sample into acc (and the last one writes the
            // output) itself — no sample slab, no k_accum; otherwise a binary64 sample slab, then k_accum
            const bool single = wave_single_write(p, D, lv != nullptr && !levels_hit);
            rc = with_prec_pow(single ? precision : RT_OUT_F64, p->hdr.int_pow, [&](auto prec, auto genpow) {
                return launch_wavefront<decltype(prec)::value, decltype(genpow)::value>(
                    p, W, H, im, D, rb, sh, ns, r0, r1, single ? d_out : smp, lv, st, (int)spp, s, seed,
                    single ? acc : nullptr, levels_hit);
            });
            if (rc != RT_OK) return rc;
            if (single) continue;
            with_int<RT_OUT_F64, RT_OUT_F32>(precision, [&](auto prec) {
                hipLaunchKernelGGL(k_accum<decltype(prec)::value>, dim3(blocks), dim3(256), 0, st, n, smp + e0, acc + e0, dst,
                                   s, (int)spp);
            });
            HIPCHK(hipGetLastError());
        }
        return RT_OK;
    }
    if (!use_mega_engine(p, D, order)) { // the wavefront engine always evaluates the reference's exact order
        const long long key[16] = {W, H, D, rb, sh, ns, precision, ((long long)r0 << 32) | r1,
                                   (long long)(intptr_t)d_out, (long long)(intptr_t)d_levels, levels_hit,
                                   im.IW, im.IH, im.x0, im.y0, 0};
        return launch_frame(p, key, st, [&](hipStream_t s) {
            return with_prec_pow(precision, p->hdr.int_pow, [&](auto prec, auto genpow) {
                return launch_wavefront<decltype(prec)::value, decltype(genpow)::value>(
                    p, W, H, im, D, rb, sh, ns, r0, r1, d_out, d_levels, s, 1, 0, 0, nullptr, levels_hit);
            });
        });
    }
    return with_int<RT_ORDER_EXACT, RT_ORDER_FAST>(order, [&](auto ord) {
        return with_prec_pow(precision, p->hdr.int_pow, [&](auto prec, auto genpow) {
            return launch_t<decltype(ord)::value, decltype(prec)::value, decltype(genpow)::value>(
                p, W, H, im, D, rb, sh, ns, r0, r1, d_out, d_levels, st, levels_hit);
        });
    });
}

extern "C" {

// RT_PROGRESSIVE: samples [sample_begin, sample_end) of rt_launch_window's frame folded into the
// caller's binary64 sum, one wavefront pass per sample with rt_launch_rows' choice between the two
// ways of summing.  Every pass has the keep bit: none divides, none writes a frame.
int rt_launch_samples(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                      uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, uint32_t spp,
                      uint64_t seed, uint32_t sample_begin, uint32_t sample_end, double *d_sum, uint8_t *d_levels,
                      void *stream) {
    if (!p || !d_sum || (uintptr_t)d_sum % 8) return RT_EBADARG;
    const int ok = launch_args_check(width, height, x0, y0, win_w, win_h, row_block, shard, nshards, RT_OUT_F64,
                                     RT_ORDER_EXACT, spp);
    if (ok != RT_OK) return ok;
    if (sample_begin >= sample_end || sample_end > spp) return RT_EBADARG;
    const ImageGeom im{(int)width, (int)height, (int)x0, (int)y0};
    DevGuard g(p->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int W = (int)win_w, H = (int)win_h, D = (int)depth, rb = (int)row_block, sh = (int)shard, ns = (int)nshards;
    const int slab_rows = (int)rt_shard_rows(win_h, row_block, nshards);
    const size_t n = valid_slab_rows(H, rb, sh, ns) * W * 3; // the slab's elements inside the image, a prefix
    if (n == 0) return RT_OK;
    const int blocks = (int)std::min<size_t>(8192, (n + 255) / 256);
    for (uint32_t s = sample_begin; s < sample_end; ++s) {
        uint8_t *lv = s == 0 ? d_levels : nullptr;
        const bool single = wave_single_write(p, D, lv != nullptr);
        double *smp = nullptr; // the pass's own slab, where it does not write every pixel exactly once
        if (!single) {
            const int rc = grow(p, rt_prepared::W_SAMPLE, (size_t)slab_rows * W * 3 * sizeof(double));
            if (rc != RT_OK) return rc;
            smp = p->buf<double>(rt_prepared::W_SAMPLE);
        }
        // (a single-write pass is handed the sum as its frame too: with the keep bit it stores to neither)
        const int rc = with_bool(!p->hdr.int_pow, [&](auto genpow) {
            return launch_wavefront<RT_OUT_F64, decltype(genpow)::value>(p, W, H, im, D, rb, sh, ns, 0, slab_rows,
                                                                         single ? d_sum : smp, lv, st, (int)spp, (int)s,
                                                                         seed, single ? d_sum : nullptr, 0, true);
        });
        if (rc != RT_OK) return rc;
        if (single) continue;
        // k_accum told of a frame one sample longer: it folds and keeps the sum, and never reads `out`
        hipLaunchKernelGGL(k_accum<RT_OUT_F64>, dim3(blocks), dim3(256), 0, st, n, smp, d_sum, nullptr, (int)s,
                           (int)s + 2);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// Copy the blocks of one shard's slab to their rows in a row-major image.  dst_kind selects
// hipMemcpyDeviceToDevice or DeviceToHost.
static int scatter_slab(const char *slab, uint32_t rowbytes, uint32_t H, uint32_t rb, uint32_t shard,
                        uint32_t nshards, char *image, hipMemcpyKind kind, hipStream_t st) {
    uint64_t blk_bytes = (uint64_t)rb * rowbytes;
    uint32_t nfull = 0;
    while ((((uint64_t)nfull * nshards + shard) * rb + rb) <= H) nfull++;
    if (nfull)
        HIPCHK(hipMemcpy2DAsync(image + (uint64_t)shard * blk_bytes, (size_t)blk_bytes * nshards, slab,
                                (size_t)blk_bytes, (size_t)blk_bytes, nfull, kind, st));
    uint64_t g0 = ((uint64_t)nfull * nshards + shard) * rb;
    if (g0 < H) { // one partial block at the bottom of the image
        uint64_t rows = H - g0;
        HIPCHK(hipMemcpyAsync(image + g0 * rowbytes, slab + (uint64_t)nfull * blk_bytes, rows * rowbytes, kind, st));
    }
    return RT_OK;
}

int rt_unshard(const void *d_slabs, uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards,
               int precision, void *d_image, void *stream) {
    if (!d_slabs || !d_image || width == 0 || height == 0 || row_block == 0 || nshards == 0) return RT_EBADARG;
    if (precision != RT_OUT_F64 && precision != RT_OUT_F32 && precision != RT_OUT_U8 && precision != RT_OUT_U16)
        return RT_EBADARG;
    uint32_t esz = precision == RT_OUT_F64 ? 8 : precision == RT_OUT_F32 ? 4 : precision == RT_OUT_U16 ? 2 : 1;
    uint32_t rowbytes = width * 3 * esz;
    uint64_t slab_bytes = (uint64_t)rt_shard_rows(height, row_block, nshards) * rowbytes;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (uint32_t s = 0; s < nshards; s++) {
        int rc = scatter_slab(static_cast<const char *>(d_slabs) + s * slab_bytes, rowbytes, height, row_block, s,
                              nshards, static_cast<char *>(d_image), hipMemcpyDeviceToDevice, st);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

} // extern "C"
