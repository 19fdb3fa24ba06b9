// rt_render.hip — the MI355X (gfx950) render kernels and the C-ABI of include/rt_mi355x.h.
//
// One translation unit (the kernel templates are launched from the code that picks their
// arguments): the device code lives in the rt_*.inc fragments included below, inside the anonymous
// namespace and in order of dependence; this file is the host side — rt_prepared and its work
// space, the choice of engine and kernel template, frame graphs and the C-ABI entry points.
// Every launch is described by one rt_frame (rt_internal.h) from the entry point down to the
// kernels' arguments.  The wavefront engine's host side is a plan and four stages: wave_plan (the
// mode, the sizes, the LDS layout: no HIP call), wave_grow, wave_pmask and wave_pass, the last
// built of wave_level_lists, wave_reflect and wave_walks; launch_sample_passes is the one loop
// over the samples of a supersampled band.
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
#include <initializer_list>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"
#include "rt_pick.h"
#include "rt_plist.h"
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
#include "rt_primary.inc"  // primary rays, the jitter, hit normals (shared with rt_attrs.hip)
#include "rt_wave.inc"     // the wavefront engine (default): records, pass geometry, lists, pixel output
#include "rt_wave_primary.inc" // ... its primary pass (k_pmask, k_primary)
#include "rt_wave_walk.inc"    // ... its chain walks (walk_up, walk_fold, k_walk_deep, k_walk)
#include "rt_wave_levels.inc"  // ... its per-level kernels (k_reflect, k_light, k_reflect_shade)
#include "rt_selftest.inc" // the arithmetic self-test kernels

} // namespace

// The launch record: which instantiation of each render-path kernel a context has launched (enqueued,
// so a replayed frame graph adds nothing), for tests/dispatch_matrix.py.  A launch site ORs one bit
// into its family's set; the bit is the template arguments read as the digits of a mixed-radix number
// (an int argument ranges over [0, radix), a bool over false, true).  rt_debug_launched spells the set
// bits as the demangled names of the kernels' host stubs.
struct LaunchRecord {
    enum Family { RENDER, PMASK, PRIMARY, ITEMS, REFLECT, REFLECT_SHADE, LIGHT, WALK, WALK_DEEP, ACCUM, NFAMILY };
    static constexpr int MAX_ARGS = 6;
    struct Spec {
        const char *name;
        int nargs;
        int radix[MAX_ARGS]; // > 0: an int argument; -2: a bool
    };
    static constexpr Spec spec[NFAMILY] = {
        {"k_render", 5, {2, 2, -2, -2, -2}},            // ORDER, PREC, LEVELS, GENPOW, NB
        {"k_pmask", 1, {-2}},                           // JITTER
        {"k_primary", 2, {2, -2}},                      // PREC, LEVELS
        {"k_items", 0, {}},                             // (no template)
        {"k_reflect", 2, {-2, -2}},                     // LEVELS, ILP
        {"k_reflect_shade", 6, {2, -2, 3, -2, -2, -2}}, // PREC, GENPOW, SPH, ILP, BVH, LAST
        {"k_light", 3, {2, -2, 3}},                     // PREC, GENPOW, SPH
        {"k_walk", 5, {2, -2, 3, 3, -2}},               // PREC, GENPOW, SPH, SRC, DEEP
        {"k_walk_deep", 2, {-2, 3}},                    // GENPOW, SPH
        {"k_accum", 1, {2}},                            // PREC
    }; // (tests/test_dispatch_matrix.py reads this table and compares it with the compiled stubs)
    unsigned long long bits[NFAMILY][2] = {}; // (the widest families have 96 instantiations)
    void note(Family f, std::initializer_list<int> args) {
        int i = 0, k = 0;
        for (int a : args) i = i * std::abs(spec[f].radix[k++]) + a;
        bits[f][i >> 6] |= 1ull << (i & 63);
    }
};

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
    int *d_elem_of = nullptr; // compact object id -> index in the caller's scene list (rt_launch_attrs)
    int *d_canon_of = nullptr; // scene list index -> its canonical element's index, -1: no object (rt_query_shadow)
    int n_elems = 0;           // entries of d_canon_of: the caller's scene list
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
    LaunchRecord launched; // rt_debug_launched
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
    const size_t elem_bytes = c.elem_of.size() * sizeof(int), canon_bytes = c.canon_of.size() * sizeof(int);
    double *tab = nullptr;
    int *itab = nullptr, *elem_of = nullptr, *canon_of = nullptr;
    int rc = RT_OK;
    // (a scene without objects still gets a table: one int nobody reads)
    if (hipMalloc(&tab, tab_bytes) != hipSuccess || hipMalloc(&itab, itab_bytes) != hipSuccess ||
        hipMalloc(&elem_of, elem_bytes ? elem_bytes : sizeof(int)) != hipSuccess ||
        hipMalloc(&canon_of, canon_bytes ? canon_bytes : sizeof(int)) != hipSuccess)
        rc = RT_ENOMEM;
    else if (hipMemcpy(tab, c.tab.data(), tab_bytes, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(itab, c.itab.data(), itab_bytes, hipMemcpyHostToDevice) != hipSuccess ||
             (elem_bytes && hipMemcpy(elem_of, c.elem_of.data(), elem_bytes, hipMemcpyHostToDevice) != hipSuccess) ||
             (canon_bytes && hipMemcpy(canon_of, c.canon_of.data(), canon_bytes, hipMemcpyHostToDevice) != hipSuccess))
        rc = RT_EHIP;
    if (rc != RT_OK) {
        (void)hipFree(tab); // (a null pointer is a no-op)
        (void)hipFree(itab);
        (void)hipFree(elem_of);
        (void)hipFree(canon_of);
        return rc;
    }
    (void)hipFree(p->d_tab);
    (void)hipFree(p->d_itab);
    (void)hipFree(p->d_elem_of);
    (void)hipFree(p->d_canon_of);
    p->d_tab = tab;
    p->d_itab = itab;
    p->d_elem_of = elem_of;
    p->d_canon_of = canon_of;
    p->n_elems = (int)c.canon_of.size();
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

// ---- picking a kernel template (with_bool, with_int, with_prec_pow: rt_pick.h)
// f(SPH): 2 = spheres only with the tables staged in LDS, 1 = spheres only, 0 = any scene
template <typename F>
auto with_sph(bool staged, bool sph_only, F &&f) {
    return with_int<0, 2>(staged ? 2 : sph_only ? 1 : 0, f);
}

// The image a frame's window lies in, as the kernels take it.
ImageGeom image_geom(const rt_frame &f) { return ImageGeom{(int)f.img_w, (int)f.img_h, (int)f.win.x0, (int)f.win.y0}; }

// The fused engine: slab rows [row0, row_end) of f in one k_render launch.
template <int ORDER, int PREC, bool GENPOW>
int launch_t(rt_prepared *p, const rt_frame &f, int row0, int row_end, void *out, uint8_t *levels, hipStream_t st,
             int levels_hit) {
    const int W = (int)f.win.w, H = (int)f.win.h, depth = (int)f.depth;
    const int rb = (int)f.row_block, shard = (int)f.shard, nshards = (int)f.nshards;
    const ImageGeom im = image_geom(f);
    dim3 grid((W + TILE - 1) / TILE, (row_end - row0 + TILE - 1) / TILE);
    size_t lds = ORDER == RT_ORDER_EXACT ? (size_t)depth * BLOCK * 12 + (size_t)BLOCK * 24 : 0;
    KtScope kt(p, RT_KT_RENDER, st);
    // scenes without wave beams (few spheres, e.g. the reference's own scene) take the beam-free build
    with_bool(levels != nullptr, [&](auto lv) {
        with_bool(!p->hdr.beam_ok, [&](auto nb) {
            p->launched.note(LaunchRecord::RENDER, {ORDER, PREC, decltype(lv)::value, GENPOW, decltype(nb)::value});
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

// Test-only (not part of include/rt_mi355x.h; tests/dispatch_matrix.py): the kernel instantiations
// launched on p since the last reset, one per line as the demangled name of its host stub
// ("k_walk<1, true, 2, 1, true>"), NUL-terminated, in buf[0, cap).  Returns the bytes the
// whole text needs, the NUL included (text cut to cap when larger); reset != 0 then clears the record.
int rt_debug_launched(rt_prepared *p, char *buf, int cap, int reset) {
    if (!p || cap < 0 || (cap > 0 && !buf)) return RT_EBADARG;
    size_t need = 0;
    auto put = [&](const char *s) {
        for (; *s; ++s, ++need)
            if ((long long)need < (long long)cap - 1) buf[need] = *s;
    };
    for (int f = 0; f < LaunchRecord::NFAMILY; ++f) {
        const LaunchRecord::Spec &sp = LaunchRecord::spec[f];
        for (int i = 0; i < 128; ++i) {
            if (!(p->launched.bits[f][i >> 6] >> (i & 63) & 1)) continue;
            int digit[LaunchRecord::MAX_ARGS] = {};
            for (int k = sp.nargs - 1, r = i; k >= 0; --k) {
                const int radix = std::abs(sp.radix[k]);
                digit[k] = r % radix;
                r /= radix;
            }
            put(sp.name);
            for (int k = 0; k < sp.nargs; ++k) {
                char num[16];
                std::snprintf(num, sizeof(num), "%d", digit[k]);
                put(k ? ", " : "<");
                put(sp.radix[k] > 0 ? num : digit[k] ? "true" : "false");
            }
            put(sp.nargs ? ">\n" : "\n");
        }
    }
    if (cap > 0) buf[std::min<size_t>(need, (size_t)cap - 1)] = 0;
    if (reset) p->launched = LaunchRecord{};
    return (int)need + 1;
}

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
    return rt_shard_slab_rows(height, row_block, nshards);
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
    (void)hipFree(p->d_elem_of);
    (void)hipFree(p->d_canon_of);
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

rt_scene_view rt_prepared_scene(const rt_prepared *p) {
    return rt_scene_view{p->device, &p->hdr, p->d_tab, p->d_itab, p->d_elem_of, p->d_canon_of, p->n_elems};
}

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

// ---- the wavefront engine's host side: a plan (pure arithmetic), the work space grown from it,
// the primary-mask cache, and one function per stage of a row pass.

// What tells one pass over a band from another when a pixel is sampled more than once.
struct WaveSample {
    int sample = 0, spp = 1;
    unsigned long long seed = 0;
    // acc (slab row 0, binary64, or null): the pass folds its sample into it where each pixel is
    // written (put_pixel) — only valid when WavePlan::single_write holds
    double *acc = nullptr;
    // keep (RT_PROGRESSIVE): the pass only accumulates, whatever its sample — `out` is never written
    bool keep = false;
    // levels_hit: k_primary writes the primary-hit mask (what it always writes: 1 on a hit, 0 on a
    // miss) and the later kernels do not count levels, so the fused path stays on
    int levels_hit = 0;
};

// Everything a launch of slab rows [row_begin, row_end) decides before it touches the device.
struct WavePlan {
    int row_begin, row_end;
    int nlev;          // queued levels: the depth, at least 1
    bool count_levels; // the kernels after k_primary count levels (levels wanted, and not just the hit mask)
    // shading beside the reflection chain on the side streams (level 0 provisionally, by k_light)
    bool overlap;
    int nrefl, nshade; // reflection levels; shaded levels
    // no side streams (frames in flight): each level's shading fused into the next reflection
    // pass (k_reflect_shade)
    bool fuse;
    // Inline walks (k_reflect_shade's iw, levels >= 1): every level is shaded by the launch that
    // reflects it; the chain of a shaded record without a child is walked by that launch, and the
    // deepest level's hits are shaded and walked by the launch that finds them (not queued) — what
    // k_walk did, minus its launch, the deepest level's k_items, the terminal records' colour entries
    // and their re-reads.  Needs the shadow answers in the records (<= 32 lights) and two reflection
    // levels or more (level 1's kernel, the dominant one, is left as is).  For S64 the dense
    // arrangement this implies measured the same as the sparse one (profiles/r05aa_ab_memset_dense.txt).
    bool iw;
    // spheres only, culling on: every shadow target has occluder masks (lit_by<1>); their
    // per-lane-gathered tables staged in each workgroup's LDS when they fit (SPH = 2)
    bool sph_only, staged;
    // ... and for LDS-staged scenes of up to TERM_MAX_LIGHTS lights those walks fold the child's
    // colour into per-light terms stored at the first shading instead of shading again (walk_fold):
    // one entry per slot of the queued levels 1 .. nrefl-1.  An inline-walk launch writes no colour
    // entries, so the entries take the colour buffer, grown to the larger of its two uses.  (Staged
    // scenes only: S256 depth 8 with its tables in L2 and dense deep levels measured 2.7 % slower per
    // frame with the entries than reshading, profiles/terms_ab_c3.txt; only the SPH = 2 kernels
    // compile the entries in.)
    bool fold;
    int pass_rows, tiles_x; // rows per pass (queue memory is bounded, queue_budget), tiles per tile row
    size_t slots, list0;    // record slots per level of a pass; ints before the dense lists in W_ITEMS
    size_t bytes[rt_prepared::W_COUNT]; // the work space a pass needs (0: not this plan's to grow)
    // the primary rays' candidate masks (k_pmask), of the whole slab: half-tiles, bytes (0: no masks)
    // after the flags: the list of active tiles (pmask_list) — int rowoff[tile_rows + 1] at list_off
    // bytes, uint2 list[tiles of the slab] at alist_off
    int slab_all, tile_rows;
    size_t nhalf, pmask_bytes, list_off, alist_off;
    // dynamic LDS: the SPH = 2 kernels' staged tables (0 for SPH < 2); for the reflection kernels of
    // levels that traverse the sphere BVH, after them the BVH nodes and sphere rows (when they fit
    // BVH_LDS_MAX) and every lane's stack, at the offsets rhdr carries
    size_t lds, lds_bvh;
    SceneHdr rhdr;
    // (LDS-staged scenes keep the candidate walks: their tables and the BVH would not fit together)
    bool bvh_at(int k) const { return !staged && rhdr.bvh_ok && k >= rhdr.bvh_level; }
    size_t lds_r(int k) const { return bvh_at(k) ? lds_bvh : lds; }
    // Does a pass write every pixel exactly once?  Yes with k_reflect_shade (the colours of records
    // with a reflection hit are left to k_walk) and without reflections; no when k_light shades
    // level 0 provisionally beside the chain (side streams, or levels requested).
    bool single_write() const { return nrefl == 0 || (!overlap && !count_levels); }
};

WavePlan wave_plan(const rt_prepared *p, const rt_frame &f, int row_begin, int row_end, bool levels, int levels_hit) {
    const SceneHdr &hdr = p->hdr;
    const int W = (int)f.win.w, D = (int)f.depth;
    WavePlan pl = {};
    pl.row_begin = row_begin;
    pl.row_end = row_end;
    pl.nlev = D > 0 ? D : 1;
    pl.count_levels = levels && !levels_hit;
    const int slab_rows = row_end - row_begin;
    const size_t per_row = (size_t)W * pl.nlev * sizeof(HitRec);
    pl.pass_rows = (int)std::min<size_t>((size_t)slab_rows, std::max<size_t>(TILE, queue_budget() / per_row));
    pl.pass_rows = std::max(TILE, pl.pass_rows / TILE * TILE);
    if (pl.pass_rows > slab_rows) pl.pass_rows = slab_rows;
    pl.tiles_x = (W + TILE - 1) / TILE;
    const size_t max_tiles = (size_t)pl.tiles_x * ((pl.pass_rows + TILE - 1) / TILE);
    const size_t slots = pl.slots = max_tiles * TILE_SLOTS;
    pl.overlap = lit_overlap(p) && D > 1 && hdr.n_light > 0;
    pl.nrefl = (hdr.n_light > 0 && D > 1) ? D - 1 : 0;
    pl.nshade = D > 0 ? 1 + pl.nrefl : 0;
    pl.fuse = !pl.overlap && !pl.count_levels && pl.nrefl > 0;
    pl.iw = pl.fuse && hdr.n_light <= 32 && pl.nrefl >= 2;
    pl.sph_only = hdr.n_tri == 0 && hdr.n_pl == 0 && hdr.cull_ok && hdr.occ_ok;
    pl.staged = pl.sph_only && hdr.l_bytes > 0;
    pl.fold = pl.iw && pl.staged && hdr.n_light <= TERM_MAX_LIGHTS;
    // colours of levels 1 .. depth-1, COL_W doubles per slot (level 0 goes straight to the frame) —
    // or the per-light terms — and per level the has-a-child flags
    const size_t col_doubles = slots * COL_W * (size_t)std::max(1, pl.nlev - 1);
    const size_t term_bytes =
        pl.fold ? slots * (size_t)(pl.nrefl - 1) * term_stride(hdr.n_light) * sizeof(double2) : 0;
    pl.bytes[rt_prepared::W_QUEUE] = slots * pl.nlev * sizeof(HitRec);
    pl.bytes[rt_prepared::W_COLBUF] = std::max(col_doubles * sizeof(double), term_bytes);
    pl.bytes[rt_prepared::W_CHILD] = slots * pl.nlev;
    pl.bytes[rt_prepared::W_LIT] = slots * pl.nlev * sizeof(unsigned);
    pl.bytes[rt_prepared::W_COUNTS] = max_tiles * pl.nlev * sizeof(int);
    // dense work lists: 64 per-level record counts, then per level the slots of its records in tile order
    pl.list0 = level_counts(pl.nlev);
    pl.bytes[rt_prepared::W_ITEMS] = (pl.list0 + slots * pl.nlev) * sizeof(int);
    if (hdr.beam_ok && D > 0) {
        pl.slab_all = (int)f.slab_rows();
        const rt_pmask_layout lay = rt_pmask_layout_of(W, pl.slab_all, hdr.n_chunk, TILE); // (rt_plist.h)
        pl.nhalf = lay.nhalf; // (after the masks: one flag byte per half-tile)
        pl.tile_rows = lay.tile_rows;
        pl.list_off = lay.rowoff_off;
        pl.alist_off = lay.list_off;
        pl.pmask_bytes = lay.bytes;
    }
    pl.lds = pl.lds_bvh = pl.staged ? (size_t)hdr.l_bytes : 0;
    pl.rhdr = hdr;
    if (pl.rhdr.bvh_ok) pl.lds_bvh = bvh_lds_place(pl.rhdr, pl.lds, BLOCK);
    return pl;
}

// The work space of a plan's passes (grow bumps gen where it reallocates), and the side streams.
int wave_grow(rt_prepared *p, const WavePlan &pl, int depth) {
    for (int w = 0; w < rt_prepared::W_COUNT; ++w) {
        const int rc = grow(p, (rt_prepared::Work)w, pl.bytes[w]);
        if (rc != RT_OK) return rc;
    }
    return pl.overlap ? side_stream(p, depth) : RT_OK;
}

// The primary rays' candidate masks of the whole slab (k_pmask, on st), recomputed only when the
// frame geometry — the raster's and the image's: two windows of one size at different origins see
// different rays — or the scene changed (or after rt_trim).
int wave_pmask(rt_prepared *p, const WavePlan &pl, const rt_frame &f, bool supersampled, hipStream_t st) {
    if (!pl.pmask_bytes) return RT_OK;
    const int W = (int)f.win.w, H = (int)f.win.h, rb = (int)f.row_block, sh = (int)f.shard, ns = (int)f.nshards;
    const ImageGeom im = image_geom(f);
    const long long key[12] = {W, H, rb, sh, ns, supersampled, (long long)p->scene_gen, pl.slab_all, im.IW, im.IH, im.x0, im.y0};
    if (p->pmask_valid && std::memcmp(key, p->pmask_key, sizeof(key)) == 0) return RT_OK;
    p->pmask_valid = false;
    // New masks (and perhaps a new buffer): a frame graph captured with the old ones holds
    // no k_pmask launch and would read these, so it is invalidated (gen).
    ++p->gen;
    const int rc = grow(p, rt_prepared::W_PMASK, pl.pmask_bytes);
    if (rc != RT_OK) return rc;
    const int nhalf = (int)pl.nhalf;
    const dim3 pg((unsigned)std::min<size_t>(4096, (pl.nhalf + 3) / 4));
    const dim3 lg((unsigned)std::min(4096, (pl.tile_rows + 3) / 4)); // the list's phases 1 and 3: a wave per tile row
    unsigned long long *const masks = p->buf<unsigned long long>(rt_prepared::W_PMASK);
    char *const base = p->buf<char>(rt_prepared::W_PMASK);
    KtScope kt(p, RT_KT_PMASK, st);
    with_bool(supersampled, [&](auto ss) {
        p->launched.note(LaunchRecord::PMASK, {decltype(ss)::value});
        for (int phase = 0; phase <= 3; ++phase) // the masks and flags, then the list of active tiles (pmask_list)
            hipLaunchKernelGGL(k_pmask<decltype(ss)::value>, phase == 0 ? pg : phase == 2 ? dim3(1) : lg, dim3(256), 0, st,
                               p->hdr, p->d_tab, p->d_itab, W, H, rb, sh, ns, pl.slab_all, nhalf, masks,
                               reinterpret_cast<unsigned char *>(masks + pl.nhalf * p->hdr.n_chunk), im, phase,
                               reinterpret_cast<int *>(base + pl.list_off), reinterpret_cast<uint2 *>(base + pl.alist_off));
    });
    HIPCHK(hipGetLastError());
    std::memcpy(p->pmask_key, key, sizeof(key));
    p->pmask_valid = true;
    return RT_OK;
}

// The grid of a persistent per-level kernel: a wave per 64 slots of the pass's tiles, `cap` workgroups at most.
int stride_blocks(int ntiles, int cap) {
    return std::min<int>(cap, (ntiles * (TILE_SLOTS / 64) + BLOCK / 64 - 1) / (BLOCK / 64));
}

// One row pass: slab rows [row0, row0 + rows), its slices of the work space and its grids.
struct WavePass {
    hipStream_t st;
    int rows, ntiles;
    // the pass's first row of out / levels (the kernels map slab rows to image rows through the
    // shard interleave themselves).  lv: the level count, null unless counted; lv0: k_primary's
    void *o;
    uint8_t *lv, *lv0;
    PassGeom g; // level-0 records are rebuilt from it
    HitRec *q;
    double *colbuf;
    double2 *terms; // the colour buffer as per-light terms (fold), else null
    uint8_t *child;
    unsigned *lit;
    int *counts, *nitems, *lists; // nitems: [0, 64) per-level record counts
    int sblocks, sblocks1, sblocksw, sblocksb;
    size_t lslots() const { return (size_t)ntiles * TILE_SLOTS; } // record slots of one level
    HitRec *qk(int k) const { return q + k * lslots(); }
    int *ck(int k) const { return counts + (size_t)k * ntiles; }
    int *ik(int k) const { return lists + k * lslots(); }
    double *colk(int k) const { return k > 0 ? colbuf + (k - 1) * lslots() * COL_W : nullptr; }
    uint8_t *chk(int k) const { return child + k * lslots(); }
    unsigned *litk(int k) const { return lit + k * lslots(); }
};

// streams of the shading pass: level 0 (the bulk) beside the whole reflection chain, the next
// levels each on their own, so no level waits for another's shading
hipStream_t shade_stream(const rt_prepared *p, const WavePlan &pl, const WavePass &ps, int k) {
    return pl.overlap ? p->side[std::min(k, 1)] : ps.st;
}

// level k's dense list, then its shading (k_light reads only level k: on a side stream it starts
// as soon as the list exists and runs beside the next reflections)
template <int PREC, bool GENPOW>
int wave_level_lists(rt_prepared *p, const WavePlan &pl, const WavePass &ps, int k) {
    // (inline walks: the deepest level is shaded by the launch that finds its hits, never queued)
    if (pl.iw && k == pl.nrefl) return RT_OK;
    const hipStream_t st = ps.st, ls = shade_stream(p, pl, ps, k);
    const dim3 iblocks((ps.ntiles + ITEMS_BLOCK - 1) / ITEMS_BLOCK);
    p->launched.note(LaunchRecord::ITEMS, {});
    hipLaunchKernelGGL(k_items, iblocks, dim3(ITEMS_BLOCK), 0, st, ps.ck(k), ps.ntiles, ps.ik(k), ps.nitems + k);
    HIPCHK(hipGetLastError());
    if (pl.overlap) {
        HIPCHK(hipEventRecord(p->ev_level[k], st));
        HIPCHK(hipStreamWaitEvent(ls, p->ev_level[k], 0));
    }
    if (pl.fuse && k < pl.nrefl) return RT_OK; // shaded by k_reflect_shade(k + 1)
    if (k == pl.nrefl && k >= 2) { // the deepest level >= 2: shaded by k_walk_deep / k_walk
        if (pl.overlap) HIPCHK(hipEventRecord(p->ev_lit[k], ls));
        return RT_OK;
    }
    // levels >= 2 are shaded here only when dense (decided on the device; otherwise the
    // launch exits at once): a smaller persistent grid keeps the empty launch cheap
    const int lblocks = k >= 2 ? std::min(ps.sblocks, DEEP_LIGHT_BLOCKS) : ps.sblocks;
    with_sph(pl.staged, pl.sph_only, [&](auto sph) {
        p->launched.note(LaunchRecord::LIGHT, {PREC, GENPOW, decltype(sph)::value});
        hipLaunchKernelGGL((k_light<PREC, GENPOW, decltype(sph)::value>), dim3(lblocks), dim3(BLOCK), pl.lds, ls, p->hdr,
                           p->d_tab, p->d_itab, k, ps.o, ps.qk(k), ps.ik(k), ps.nitems + k, ps.colk(k), ps.litk(k), ps.g);
    });
    HIPCHK(hipGetLastError());
    if (pl.overlap) HIPCHK(hipEventRecord(p->ev_lit[k], ls));
    return RT_OK;
}

// The reflections of level k - 1's records into level k.  Level 1 (from the primary hits) is dense
// and throughput-bound; deeper levels are a few waves each, bound by one wave's dependent chain:
// they walk two candidates per step.
template <int PREC, bool GENPOW>
int wave_reflect(rt_prepared *p, const WavePlan &pl, const WavePass &ps, int k) {
    const hipStream_t st = ps.st;
    const bool iw = pl.iw;
    const int nrefl = pl.nrefl;
    if (pl.fuse) {
        // levels traversing the sphere BVH (unstaged scenes only) take the BVH instantiations,
        // the deepest level with inline walks the LAST ones; both only come with ILP
        const bool bvh_k = pl.bvh_at(k), ilp = bvh_k || k != 1, last = ilp && iw && k == nrefl;
        with_sph(pl.staged, pl.sph_only, [&](auto sph) {
            constexpr int SPH = decltype(sph)::value;
            auto rs = [&](auto ilp_c, auto bvh_c, auto last_c) {
                constexpr bool BVH = decltype(bvh_c)::value;
                p->launched.note(LaunchRecord::REFLECT_SHADE,
                                 {PREC, GENPOW, SPH, decltype(ilp_c)::value, BVH, decltype(last_c)::value});
                hipLaunchKernelGGL(
                    (k_reflect_shade<PREC, GENPOW, SPH, decltype(ilp_c)::value, BVH, decltype(last_c)::value>),
                    dim3(k == 1 ? ps.sblocks1 : BVH ? ps.sblocksb : ps.sblocks), dim3(BLOCK), pl.lds_r(k), st, pl.rhdr,
                    p->d_tab, p->d_itab, k, ps.o, ps.qk(k - 1), ps.ik(k - 1), ps.nitems + (k - 1), ps.qk(k), ps.ck(k),
                    iw ? nullptr : ps.chk(k - 1), ps.colk(k - 1), ps.g, iw && k >= 2 ? (k == nrefl ? 2 : 1) : 0, ps.terms);
            };
            auto rs_ilp = [&](auto bvh_c) {
                with_bool(last, [&](auto last_c) { rs(std::true_type{}, bvh_c, last_c); });
            };
            if (!ilp) rs(std::false_type{}, std::false_type{}, std::false_type{});
            else if constexpr (SPH == 2) rs_ilp(std::false_type{}); // (staged: never the BVH, bvh_at)
            else with_bool(bvh_k, rs_ilp);
        });
    } else {
        with_bool(ps.lv != nullptr, [&](auto has_lv) {
            with_bool(k != 1, [&](auto ilp_c) {
                p->launched.note(LaunchRecord::REFLECT, {decltype(has_lv)::value, decltype(ilp_c)::value});
                hipLaunchKernelGGL((k_reflect<decltype(has_lv)::value, decltype(ilp_c)::value>), dim3(ps.sblocks),
                                   dim3(BLOCK), pl.lds, st, pl.rhdr, p->d_tab, p->d_itab, k, ps.qk(k - 1), ps.ik(k - 1),
                                   ps.nitems + (k - 1), ps.qk(k), ps.ck(k), ps.lv, ps.chk(k - 1), ps.g);
            });
        });
    }
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// The chain walks that finish a pass with reflections (nrefl > 0).  Without side streams one
// k_walk finishes every chain (sparse deep levels shaded on the way).  With side streams (see
// deep_dense): k_walk_deep right after the chain; the chains ending at level 1 (the bulk) are
// finished on side stream 0 as soon as levels 0 and 1 are shaded, beside it; then the rest, once
// every level's shading is in (side stream 1 shades levels 1.. in order: its last level's event
// covers them all).
template <int PREC, bool GENPOW>
int wave_walks(rt_prepared *p, const WavePlan &pl, const WavePass &ps, int D) {
    const SceneHdr &hdr = p->hdr;
    const hipStream_t st = ps.st;
    const bool overlap = pl.overlap, staged = pl.staged, sph_only = pl.sph_only;
    const size_t ls_ = ps.lslots();
    const bool bits = hdr.n_light <= 32; // the shadow answers fit the record
    // deep: the merged walk (no k_walk_deep; without side streams); after k_reflect_shade
    // (fuse) the shadow answers are in the children's records (ANS_REC), otherwise in k_light's array
    auto walk = [&](hipStream_t s_, int lo, int hi, bool deep) {
        const int src = !bits ? ANS_TEST : deep && pl.fuse ? ANS_REC : ANS_LIT;
        with_sph(staged, sph_only, [&](auto sph) {
            with_int<ANS_TEST, ANS_REC>(src, [&](auto src_c) {
                with_bool(deep, [&](auto deep_c) {
                    // (the records hold answers in the merged launch only: no other ANS_REC kernel exists)
                    if constexpr (decltype(src_c)::value != ANS_REC || decltype(deep_c)::value) {
                        p->launched.note(LaunchRecord::WALK, {PREC, GENPOW, decltype(sph)::value, decltype(src_c)::value,
                                                              decltype(deep_c)::value});
                        hipLaunchKernelGGL((k_walk<PREC, GENPOW, decltype(sph)::value, decltype(src_c)::value,
                                                   decltype(deep_c)::value>),
                                           dim3(ps.sblocksw), dim3(BLOCK), pl.lds, s_, hdr, p->d_tab, p->d_itab, D, ps.o,
                                           ps.q, ls_, ps.lists, ps.nitems, ps.colbuf, ps.child, ps.lit, lo, hi, ps.g);
                    }
                });
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
            p->launched.note(LaunchRecord::WALK_DEEP, {GENPOW, decltype(sph)::value});
            hipLaunchKernelGGL((k_walk_deep<GENPOW, decltype(sph)::value>), dim3(ps.sblocks), dim3(BLOCK), pl.lds, st, hdr,
                               p->d_tab, p->d_itab, D, ps.q, ls_, ps.lists, ps.nitems, ps.child, ps.colk(2));
        });
        HIPCHK(hipGetLastError());
    }
    if (overlap) {
        HIPCHK(hipStreamWaitEvent(st, p->ev_lit[pl.nrefl], 0));
        HIPCHK(hipStreamWaitEvent(st, p->ev_lit[0], 0));
        if (D > 2) walk(st, 2, D, false);
    } else if (!pl.iw) {
        walk(st, 1, D, true); // every chain in one launch, sparse deep levels shaded there too
    }
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// One row pass, slab rows [row0, ...) of the plan's range, enqueued on st: k_primary, then per
// level the reflections and the lists (and what shades them), then the walks.  out / levels point
// at slab row 0.
template <int PREC, bool GENPOW>
int wave_pass(rt_prepared *p, const WavePlan &pl, const rt_frame &f, int row0, void *out, uint8_t *levels,
              hipStream_t st, const WaveSample &smp) {
    const int W = (int)f.win.w, H = (int)f.win.h, D = (int)f.depth;
    const int rb = (int)f.row_block, sh = (int)f.shard, ns = (int)f.nshards;
    const ImageGeom im = image_geom(f);
    WavePass ps = {};
    ps.st = st;
    ps.rows = std::min(pl.pass_rows, pl.row_end - row0);
    const int ntiles = ps.ntiles = pl.tiles_x * ((ps.rows + TILE - 1) / TILE);
    const size_t off = (size_t)row0 * W;
    ps.o = static_cast<char *>(out) + off * 3 * sizeof(typename rt_format<PREC>::type);
    ps.lv0 = levels ? levels + off : nullptr;
    ps.lv = pl.count_levels ? ps.lv0 : nullptr;
    double *acc_p = smp.acc ? smp.acc + off * 3 : nullptr;
    ps.q = p->buf<HitRec>(rt_prepared::W_QUEUE);
    ps.colbuf = p->buf<double>(rt_prepared::W_COLBUF);
    ps.terms = pl.fold ? reinterpret_cast<double2 *>(ps.colbuf) : nullptr;
    ps.child = p->buf<uint8_t>(rt_prepared::W_CHILD);
    ps.lit = p->buf<unsigned>(rt_prepared::W_LIT);
    ps.counts = p->buf<int>(rt_prepared::W_COUNTS);
    ps.nitems = p->buf<int>(rt_prepared::W_ITEMS);
    ps.lists = ps.nitems + pl.list0;
    ps.sblocks = stride_blocks(ntiles, STRIDE_BLOCKS);
    ps.sblocks1 = stride_blocks(ntiles, STRIDE_BLOCKS_L1);
    ps.sblocksw = stride_blocks(ntiles, STRIDE_BLOCKS_WALK);
    ps.sblocksb = stride_blocks(ntiles, STRIDE_BLOCKS_BVH);
    const unsigned long long *pmask = pl.pmask_bytes ? p->buf<unsigned long long>(rt_prepared::W_PMASK) : nullptr;
    // after the masks: one byte per half-tile, 1 = every mask zero
    const unsigned short *pempty =
        pmask ? reinterpret_cast<const unsigned short *>(pmask + pl.nhalf * p->hdr.n_chunk) : nullptr;
    // ... and the list of active tiles: the offsets from the pass's first tile row on, and the list
    const char *const pbase = p->buf<char>(rt_prepared::W_PMASK);
    const int *prow = pmask ? reinterpret_cast<const int *>(pbase + pl.list_off) + row0 / TILE : nullptr;
    const uint2 *alist = pmask ? reinterpret_cast<const uint2 *>(pbase + pl.alist_off) : nullptr;
    const int sarg = sample_arg(smp.sample, smp.keep);
    ps.g = make_pass_geom(W, im, rb, sh, ns, row0, smp.spp, sarg, smp.seed, acc_p);
    const dim3 grid(std::min(ntiles, PRIMARY_GRID)); // k_primary: grid-stride loop over the tiles
    {
        KtScope kt(p, RT_KT_PRIMARY, st);
        with_bool(ps.lv0 != nullptr, [&](auto has_lv) { // (without lv0 there is no lv either)
            p->launched.note(LaunchRecord::PRIMARY, {PREC, decltype(has_lv)::value});
            hipLaunchKernelGGL((k_primary<PREC, decltype(has_lv)::value>), grid, dim3(PRIMARY_BLOCK), 0, st, p->hdr,
                               p->d_tab, p->d_itab, W, im.y0 + H, D, rb, ps.g.yoff, ns, ps.rows, row0, ps.o, ps.lv0, ps.q,
                               ps.counts, ntiles, smp.spp, sarg, smp.seed, acc_p, pmask, pempty, ps.nitems, ps.g.img,
                               prow, alist);
        });
    }
    HIPCHK(hipGetLastError());
    int rc = RT_OK;
    if (pl.nshade > 0 && (rc = wave_level_lists<PREC, GENPOW>(p, pl, ps, 0)) != RT_OK) return rc;
    for (int k = 1; k <= pl.nrefl; ++k) {
        KtScope kt(p, k == 1 ? RT_KT_LEVEL1 : 0, st); // (level 1's time takes in its list and k_light)
        if ((rc = wave_reflect<PREC, GENPOW>(p, pl, ps, k)) != RT_OK) return rc;
        if ((rc = wave_level_lists<PREC, GENPOW>(p, pl, ps, k)) != RT_OK) return rc;
    }
    if (pl.nrefl > 0) return wave_walks<PREC, GENPOW>(p, pl, ps, D);
    if (pl.overlap && pl.nshade > 0) HIPCHK(hipStreamWaitEvent(st, p->ev_lit[0], 0));
    return RT_OK;
}

// The wavefront engine: slab rows [row_begin, row_end) of f (row_begin a multiple of TILE), in as
// many row passes as the queue budget asks for; out / levels point at slab row 0.
template <int PREC, bool GENPOW>
int launch_wavefront(rt_prepared *p, const rt_frame &f, int row_begin, int row_end, void *out, uint8_t *levels,
                     hipStream_t st, const WaveSample &smp) {
    const WavePlan pl = wave_plan(p, f, row_begin, row_end, levels != nullptr, smp.levels_hit);
    int rc = wave_grow(p, pl, (int)f.depth);
    if (rc == RT_OK) rc = wave_pmask(p, pl, f, smp.spp > 1, st);
    for (int row0 = row_begin; row0 < row_end && rc == RT_OK; row0 += pl.pass_rows)
        rc = wave_pass<PREC, GENPOW>(p, pl, f, row0, out, levels, st, smp);
    return rc;
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

// One wavefront pass per sample of a band, summed in order: what rt_launch_rows (spp > 1) and
// rt_launch_samples share.  Samples [s0, s1) of slab rows [r0, r1) of f are folded into acc (slab
// row 0); sample 0 is the one that writes the levels.
struct SampleBand {
    uint32_t r0, r1, s0, s1;
    double *acc;
    // the frame of f.precision (slab row 0) that the pass of the last sample writes — or, with
    // keep (RT_PROGRESSIVE), nothing: every pass only accumulates, and out is never written
    void *out;
    bool keep;
};
int launch_sample_passes(rt_prepared *p, const rt_frame &f, const SampleBand &b, uint8_t *d_levels, int levels_hit,
                         hipStream_t st) {
    // the band's rows inside the image (a prefix of the slab)
    const size_t v1 = std::min<size_t>(f.valid_rows(), b.r1);
    if (v1 <= b.r0) return RT_OK;
    const size_t e0 = (size_t)b.r0 * f.win.w * 3, n = (v1 - b.r0) * f.win.w * 3; // the band's elements
    const int blocks = (int)std::min<size_t>(8192, (n + 255) / 256);
    for (uint32_t s = b.s0; s < b.s1; ++s) {
        uint8_t *lv = s == 0 ? d_levels : nullptr;
        WaveSample smp;
        smp.sample = (int)s;
        smp.spp = (int)f.spp;
        smp.seed = f.seed;
        smp.keep = b.keep;
        smp.levels_hit = levels_hit;
        // every pixel written once: the pass folds its sample into acc (and the last one writes the
        // output) itself — no sample slab, no k_accum; otherwise a binary64 sample slab, then k_accum
        const bool single = wave_plan(p, f, (int)b.r0, (int)b.r1, lv != nullptr, levels_hit).single_write();
        double *slab = nullptr; // the pass's own slab, where it does not write every pixel exactly once
        if (single) {
            smp.acc = b.acc;
        } else {
            const int rc = grow(p, rt_prepared::W_SAMPLE, (size_t)f.slab_rows() * f.win.w * 3 * sizeof(double));
            if (rc != RT_OK) return rc;
            slab = p->buf<double>(rt_prepared::W_SAMPLE);
        }
        const int rc = with_prec_pow(single ? f.precision : RT_OUT_F64, p->hdr.int_pow, [&](auto prec, auto genpow) {
            return launch_wavefront<decltype(prec)::value, decltype(genpow)::value>(
                p, f, (int)b.r0, (int)b.r1, single ? b.out : slab, lv, st, smp);
        });
        if (rc != RT_OK) return rc;
        if (single) continue;
        // keep: k_accum told of a frame one sample longer folds and keeps the sum, and never reads its output
        void *dst = b.keep ? nullptr : static_cast<char *>(b.out) + e0 * rt_elem_size(f.precision);
        with_int<RT_OUT_F64, RT_OUT_F32>(f.precision, [&](auto prec) {
            p->launched.note(LaunchRecord::ACCUM, {decltype(prec)::value});
            hipLaunchKernelGGL(k_accum<decltype(prec)::value>, dim3(blocks), dim3(256), 0, st, n, slab + e0, b.acc + e0, dst,
                               (int)s, b.keep ? (int)s + 2 : (int)f.spp);
        });
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// The whole frame width x height as shard `shard`, binary64 in the reference's order, one sample:
// what the exported launches start from.
rt_frame whole_frame(uint32_t width, uint32_t height, uint32_t depth, uint32_t row_block, uint32_t shard,
                     uint32_t nshards) {
    rt_frame f = {};
    f.img_w = width;
    f.img_h = height;
    f.win = rt_window{0, 0, width, height};
    f.depth = depth;
    f.row_block = row_block;
    f.shard = shard;
    f.nshards = nshards;
    f.precision = RT_OUT_F64;
    f.order = RT_ORDER_EXACT;
    f.spp = 1;
    return f;
}

} // namespace

int rt_frame_check(const rt_frame &f) {
    const rt_window &w = f.win;
    if (f.img_w == 0 && f.img_h == 0 && w.w == 0 && w.h == 0 && w.x0 == 0 && w.y0 == 0) return RT_DONE;
    if (f.img_w == 0 || f.img_h == 0) return RT_EBADARG;
    if (f.row_block == 0 || f.nshards == 0 || f.shard >= f.nshards) return RT_EBADARG;
    if (f.precision != RT_OUT_F64 && f.precision != RT_OUT_F32) return RT_EBADARG;
    if (f.order != RT_ORDER_EXACT && f.order != RT_ORDER_FAST) return RT_EBADARG;
    if (f.spp == 0) return RT_EBADARG;
    if (f.spp > RT_MAX_SPP) return RT_ETOOBIG;
    if (f.img_w > (1u << 20) || f.img_h > (1u << 20)) return RT_ETOOBIG;
    // the window: not empty, inside the image (sums in 64 bits: x0 + w may pass 2^32)
    if (w.w == 0 || w.h == 0) return RT_EBADARG;
    if ((uint64_t)w.x0 + w.w > f.img_w || (uint64_t)w.y0 + w.h > f.img_h) return RT_EBADARG;
    if ((uint64_t)f.slab_rows() > 65535ull * TILE) return RT_ETOOBIG;
    return RT_OK;
}

// Slab rows [row_begin, min(row_end, slab rows)) of f: the boundary (rt_host.hip) renders a frame
// in row bands so that each band's copy to the host overlaps the next band's render.  The kernels
// tile and store the window; the image it lies in only places the rays.
int rt_launch_rows(rt_prepared *p, const rt_frame &f, uint32_t row_begin, uint32_t row_end, void *d_out,
                   uint8_t *d_levels, void *stream, int levels_hit) {
    if (!p || !d_out) return RT_EBADARG;
    const int ok = rt_frame_check(f);
    if (ok != RT_OK) return ok;
    const uint32_t slab = f.slab_rows();
    if (row_begin % TILE) return RT_EBADARG;
    if (row_end > slab) row_end = slab;
    if (row_begin >= row_end) return RT_OK;
    DevGuard g(p->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int r0 = (int)row_begin, r1 = (int)row_end;
    if (f.spp > 1) { // RT_SUPERSAMPLING, on the wavefront engine: one sample's slab and the running sum
        if (f.valid_rows() <= row_begin) return RT_OK;
        const size_t n_slab = (size_t)slab * f.win.w * 3;
        const int rc = grow(p, rt_prepared::W_SAMPLE, 2 * n_slab * sizeof(double));
        if (rc != RT_OK) return rc;
        const SampleBand b = {row_begin, row_end, 0, f.spp, p->buf<double>(rt_prepared::W_SAMPLE) + n_slab, d_out, false};
        return launch_sample_passes(p, f, b, d_levels, levels_hit, st);
    }
    WaveSample one;
    one.levels_hit = levels_hit;
    if (!use_mega_engine(p, (int)f.depth, f.order)) { // the wavefront engine always evaluates the reference's exact order
        const long long key[16] = {f.win.w, f.win.h, f.depth, f.row_block, f.shard, f.nshards, f.precision,
                                   ((long long)r0 << 32) | r1, (long long)(intptr_t)d_out, (long long)(intptr_t)d_levels,
                                   levels_hit, f.img_w, f.img_h, f.win.x0, f.win.y0, 0};
        return launch_frame(p, key, st, [&](hipStream_t s) {
            return with_prec_pow(f.precision, p->hdr.int_pow, [&](auto prec, auto genpow) {
                return launch_wavefront<decltype(prec)::value, decltype(genpow)::value>(p, f, r0, r1, d_out, d_levels, s, one);
            });
        });
    }
    return with_int<RT_ORDER_EXACT, RT_ORDER_FAST>(f.order, [&](auto ord) {
        return with_prec_pow(f.precision, p->hdr.int_pow, [&](auto prec, auto genpow) {
            return launch_t<decltype(ord)::value, decltype(prec)::value, decltype(genpow)::value>(
                p, f, r0, r1, d_out, d_levels, st, levels_hit);
        });
    });
}

extern "C" {

int rt_engine(rt_prepared *p, uint32_t spp) {
    if (!p || spp == 0) return RT_EBADARG;
    return (spp == 1 && use_mega_engine(p)) ? RT_ENGINE_FUSED : RT_ENGINE_WAVE;
}

int rt_launch(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t row_block, uint32_t shard,
              uint32_t nshards, int precision, int order, void *d_out, uint8_t *d_levels, void *stream) {
    rt_frame f = whole_frame(width, height, depth, row_block, shard, nshards);
    f.precision = precision;
    f.order = order;
    return rt_launch_rows(p, f, 0, ~0u, d_out, d_levels, stream, 0);
}

int rt_launch_spp(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t row_block,
                  uint32_t shard, uint32_t nshards, int precision, int order, uint32_t spp, uint64_t seed,
                  void *d_out, uint8_t *d_levels, void *stream) {
    rt_frame f = whole_frame(width, height, depth, row_block, shard, nshards);
    f.precision = precision;
    f.order = order;
    f.spp = spp;
    f.seed = seed;
    return rt_launch_rows(p, f, 0, ~0u, d_out, d_levels, stream, 0);
}

int rt_launch_window(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                     uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, int precision,
                     int order, uint32_t spp, uint64_t seed, void *d_out, uint8_t *d_levels, void *stream) {
    rt_frame f = whole_frame(width, height, depth, row_block, shard, nshards);
    f.win = rt_window{x0, y0, win_w, win_h};
    f.precision = precision;
    f.order = order;
    f.spp = spp;
    f.seed = seed;
    return rt_launch_rows(p, f, 0, ~0u, d_out, d_levels, stream, 0);
}

// RT_PROGRESSIVE: samples [sample_begin, sample_end) of rt_launch_window's frame folded into the
// caller's binary64 sum, one wavefront pass per sample with rt_launch_rows' choice between the two
// ways of summing.  Every pass has the keep bit: none divides, none writes a frame (a single-write
// pass is handed the sum as its frame too: it stores to neither).
int rt_launch_samples(rt_prepared *p, uint32_t width, uint32_t height, uint32_t depth, uint32_t x0, uint32_t y0,
                      uint32_t win_w, uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, uint32_t spp,
                      uint64_t seed, uint32_t sample_begin, uint32_t sample_end, double *d_sum, uint8_t *d_levels,
                      void *stream) {
    if (!p || !d_sum || (uintptr_t)d_sum % 8) return RT_EBADARG;
    rt_frame f = whole_frame(width, height, depth, row_block, shard, nshards);
    f.win = rt_window{x0, y0, win_w, win_h};
    f.spp = spp;
    f.seed = seed;
    const int ok = rt_frame_check(f);
    if (ok != RT_OK) return ok;
    if (sample_begin >= sample_end || sample_end > spp) return RT_EBADARG;
    DevGuard g(p->device);
    const SampleBand b = {0, f.slab_rows(), sample_begin, sample_end, d_sum, d_sum, true};
    return launch_sample_passes(p, f, b, d_levels, 0, reinterpret_cast<hipStream_t>(stream));
}

int rt_unshard(const void *d_slabs, uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards,
               int precision, void *d_image, void *stream) {
    if (!d_slabs || !d_image || width == 0 || height == 0 || row_block == 0 || nshards == 0) return RT_EBADARG;
    if (!rt_format_ok(precision)) return RT_EBADARG;
    uint32_t rowbytes = width * 3 * (uint32_t)rt_elem_size(precision);
    const uint32_t slab = rt_shard_slab_rows(height, row_block, nshards);
    uint64_t slab_bytes = (uint64_t)slab * rowbytes;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (uint32_t s = 0; s < nshards; s++) {
        int rc = rt_scatter_rows_async(static_cast<const char *>(d_slabs) + s * slab_bytes, 0, slab, rowbytes,
                                       rt_shard_map{height, row_block, s, nshards}, static_cast<char *>(d_image),
                                       hipMemcpyDeviceToDevice, st);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

} // extern "C"
