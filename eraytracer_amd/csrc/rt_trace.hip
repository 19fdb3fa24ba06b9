// rt_trace.hip — traced colours for rays the caller chose (rt_query_colours, RT_QUERY in
// include/rt_mi355x.h): pixel_colour_from_ray/3 (raytracer.erl:186-252) of n arbitrary rays over the
// resident scene, in the reference's fold order (RT_ORDER_EXACT).  The third member of the query
// family; a camera that can be aimed is a ray generator on the host plus this call.
//
// One kernel family, k_trace<PREC, GENPOW, SCAN>, shaped as k_query (rt_query.hip): 256-thread blocks,
// one ray per lane, a grid-stride loop over the batch in waves of 64 consecutive rays, everything in
// the general forms and in binary64 (norm_ok and prim_ok are cleared in the header the kernel gets;
// RT_OUT_F32 rounds at the store).  Nothing here is new arithmetic: the scans are nearest<..> as
// rt_query.hip calls them (SCAN as there, the BVH walk only for a wave whose live rays all lie in
// bvh_domain, tested per level on that level's ray), a hit's point and normal are hit_attrs'
// (rt_planes.inc), the next ray is bounce3 (vector_bounce_off_plane/2) and a level's colour is
// shade<GENPOW, 0, NB>, which holds the one copy of the light fold.  A wave stays converged from its
// loads to its stores: a lane whose chain has ended, and a lane past the batch, carries act = false.
//   forward, k = 0 .. depth-1: the nearest object, the hit's point and normal, the record of level k
//     stored in the work space, the bounced ray; ends when no lane is alive, and after level 0 in a
//     scene without lights (lighting_function/6 folds over the lights: none, no reflection either)
//   backward, from the wave's last level to 0: col = shade(record, col) on the lanes that hit at that
//     level, col = +0.0 where the chain ended or the depth ran out; level 0 stores d_rgb, d_levels
// The work space is the caller's: [level][field][ray] planes, the ray stride padded to 64
// (rt_trace_args.h); a lane reads only the records it wrote in this launch.
//
// shade's filters, for a hit point anywhere.  shade and lit_by (rt_shade.inc) were written for the
// renderer's hit records; here the ray is anybody's, so a "hit point" o + d t may lie far from the
// scene, off the object (the reference's sphere t is the ray parameter only for |d| = 1) or be
// non-finite.  The shadow ray itself, sd = -normalize(Lp - hit), is a unit vector or zero whatever
// the hit point is, it starts at a light — a tabled origin inside the scene's extent — and the
// exact test (the target's t* and every candidate's t along sd, from the lights' per-origin rows)
// has no domain.  What has one are the three filters that choose the candidates:
//  (1) occ_cell and the occluder masks (sphere targets, occ_ok).  The masks are a function of the
//      light, the target sphere and the direction cell; they were built to hold every sphere that
//      can block a ray from that light that reaches the target, for every direction in the cone the
//      target subtends.  A lane walks them only if its shadow ray hits the target (`valid`, the exact
//      test), and then sd lies in that cone wherever the hit point is: the filter depends on the
//      shadow ray, not on the hit point.  occ_cell's result is four comparisons' worth of bits, 0..15,
//      for any input, NaN included: the mask index cannot leave the table.
//  (2) make_hitball (other targets, or no masks).  It guards itself against far and non-finite
//      points: hit points beyond CULL_EXTENT (`mo`, an infinity included) turn it off, and a NaN
//      among them makes the centre NaN, which fails shadow_cone's `D > ...` test: no cone, every
//      sphere scanned.  It does NOT guard against a hit point that is off its object: shadow_cone's
//      tmax = D + r assumes the target is entered no farther from the light than the hit point, which
//      holds for a point on the target (to rounding) but not for one short of a sphere, where
//      |d| < 1 puts it.  So the kernel decides per wave and level (hitball_domain below): unless every
//      shading lane's ray had |d.d - 1| <= 2^-46 and an origin within 4 CULL_EXTENT per axis — then
//      o + d t is on the object to the rounding the renderer's own records have: its rays drift
//      that far from unit length by depth ~40, and its origins and hit points obey the same bounds —
//      shade gets a header with beam_ok = 0, the switch make_hitball reads first: no ball, no cone,
//      every sphere scanned, the brute-force result.  Triangles' and planes' t is the ray parameter
//      for any d, so their points are on their planes whenever the origin bound holds.
//  (3) shadow_cone and cull_chunk(org >= 0).  Given a ball that contains the shading lanes' hit
//      points, the cone from the light contains every sd, for hit points anywhere; its own guards
//      (light inside the ball, a sine >= 1, a cosine <= 0) turn it off, as in the renderer.
// No memory index in this unit derives from a floating-point value: rays are addressed by i, records
// by (level, field, i), table rows by object ids that nearest<..> took from the scene tables (or 0 for
// a lane without a hit), the mask cell is (1) above.  That is what makes the non-finite-ray clause
// true: such a ray misses, or "hits" with a non-finite point that (2) and the exact tests' comparisons
// (false for a NaN) keep to its own lane.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"
#include "rt_pick.h"
#include "rt_trace_args.h"

using namespace rtl;

namespace {

#include "rt_math.inc"    // binary64 primitives, the primitive tests, bounce3
#include "rt_cull.inc"    // scene access, wave culling, candidate scans, the per-lane BVH
#include "rt_shade.inc"   // nearest-object scans, the shadow test, lighting_function/6
#include "rt_primary.inc" // hit normals
#include "rt_planes.inc"  // a hit's attributes, the stores
#include "rt_query.inc"   // SCAN_*, bvh_domain

constexpr int TRACE_BLOCK = 256; // four waves, as k_query
constexpr int TRACE_GRID = 8192; // blocks at most: a batch above 2^21 rays loops

// Where make_hitball's tmax holds (filter (2) at the top of this file): the ray that produced the hit.
__device__ __forceinline__ bool hitball_domain(const D3 &o, const D3 &d) {
    const double lim = 4.0 * CULL_EXTENT, dd = d.x * d.x + d.y * d.y + d.z * d.z;
    return fabs(o.x) <= lim && fabs(o.y) <= lim && fabs(o.z) <= lim && fabs(dd - 1.0) <= 0x1p-46;
}

// The planes of level k of a work space of stride n64 (rt_trace_args.h): field f of ray i is at
// f * n64 + i of the doubles, the object id at i of the ints behind them.
struct LevelRec {
    double *f;
    int *id;
};
__device__ __forceinline__ LevelRec level_rec(char *work, unsigned long long n64, unsigned k) {
    double *f = reinterpret_cast<double *>(work + (size_t)k * (size_t)n64 * TRACE_REC_BYTES);
    return LevelRec{f, reinterpret_cast<int *>(f + TRACE_REC_DOUBLES * n64)};
}
__device__ __forceinline__ void put_d3(const LevelRec &r, unsigned long long n64, int f, size_t i, const D3 &v) {
    r.f[(size_t)f * n64 + i] = v.x;
    r.f[(size_t)(f + 1) * n64 + i] = v.y;
    r.f[(size_t)(f + 2) * n64 + i] = v.z;
}
__device__ __forceinline__ D3 get_d3(const LevelRec &r, unsigned long long n64, int f, size_t i) {
    return D3{r.f[(size_t)f * n64 + i], r.f[(size_t)(f + 1) * n64 + i], r.f[(size_t)(f + 2) * n64 + i]};
}
enum { F_DIR = 0, F_HIT = 3, F_NORMAL = 6 };

// a, b: the rays' origins and directions, n triples of doubles each — `a` one triple with one_origin.
// rgb: n colours of PREC; levels (or null): n counts; entries >= n of either are never written.
// work: depth levels of n64 = n rounded up to 64 records.  hdr: norm_ok = prim_ok = 0, and for SCAN_BVH
// the LDS offsets of this launch (rt_query_colours below).
template <int PREC, bool GENPOW, int SCAN>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace(SceneHdr hdr, const double *__restrict__ tab,
                                                      const int *__restrict__ itab, const int *__restrict__ elem_of,
                                                      const double *__restrict__ a, const double *__restrict__ b,
                                                      unsigned long long n, int one_origin, unsigned depth,
                                                      unsigned long long n64, void *__restrict__ rgb,
                                                      uint8_t *__restrict__ levels, char *__restrict__ work) {
    constexpr bool NB = SCAN == SCAN_BRUTE;
    const Scene S{hdr, tab, itab};
    if (SCAN == SCAN_BVH) stage_bvh(S); // (every thread of the block: it ends in a barrier)
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * TRACE_BLOCK;
    // base: this wave's first ray (wave-uniform, so the wave's lanes leave the loop together)
    for (unsigned long long base = (unsigned long long)blockIdx.x * TRACE_BLOCK + (threadIdx.x & ~63u); base < n;
         base += stride) {
        const unsigned long long i = base + lane;
        const bool act = i < n;
        const size_t j = (size_t)(act ? i : n - 1); // a lane past the batch: a copy of the last ray, never stored
        const size_t ja = one_origin ? 0 : j;
        const D3 o0 = {a[ja * 3], a[ja * 3 + 1], a[ja * 3 + 2]};
        D3 o = o0, d = {b[j * 3], b[j * 3 + 1], b[j * 3 + 2]};
        // forward: the chain's nearest-object scans (:186-203, the bounce of :232)
        bool alive = act;
        unsigned nlev = 0; // the levels this lane's chain hit
        unsigned wl = 0;   // (wave-uniform) the levels some lane of the wave hit
        for (unsigned k = 0; k < depth; ++k) {
            double t;
            int id;
            if (SCAN == SCAN_BRUTE) {
                id = nearest<false, false, 0, true>(S, 0, o, d, t, alive);
            } else {
                const bool walk = SCAN == SCAN_BVH && __ballot(alive && !bvh_domain(o, d, hdr.ext + 1.0)) == 0;
                id = nearest<false, false, 0, false>(S, 0, o, d, t, alive, 0, walk);
            }
            alive = alive && id >= 0;
            if (__ballot(alive) == 0) break; // (then, below, the scene has an object: row 0 exists)
            const HitAttrs at = hit_attrs(S, elem_of, o, d, id, t, true, true);
            wl = k + 1;
            if (alive) {
                const LevelRec r = level_rec(work, n64, k);
                r.id[i] = id;
                put_d3(r, n64, F_DIR, (size_t)i, d);
                put_d3(r, n64, F_HIT, (size_t)i, at.point);
                put_d3(r, n64, F_NORMAL, (size_t)i, at.normal);
                nlev = k + 1;
                d = bounce3(d, at.normal);
                o = at.point;
            }
            if (hdr.n_light == 0) break; // no light, no fold step: the reflection is never asked for
        }
        // backward: each level shaded with the colour of the level below it (:209-252)
        D3 col = {0.0, 0.0, 0.0};
        for (unsigned k = wl; k-- > 0;) {
            const bool on = nlev > k; // this lane hit at this level
            const D3 zero = {0.0, 0.0, 0.0};
            int id = 0;
            D3 dk = zero, hit = zero, N = zero, ok = o0;
            if (on) {
                const LevelRec r = level_rec(work, n64, k);
                id = r.id[i];
                dk = get_d3(r, n64, F_DIR, (size_t)i);
                hit = get_d3(r, n64, F_HIT, (size_t)i);
                N = get_d3(r, n64, F_NORMAL, (size_t)i);
                if (k > 0) ok = get_d3(level_rec(work, n64, k - 1), n64, F_HIT, (size_t)i); // this level's origin
            }
            // filter (2) at the top of this file: no hit ball unless every shading lane's ray is in its domain
            Scene SS = S;
            if (!NB && __ballot(on && !hitball_domain(ok, dk)) != 0) SS.h.beam_ok = 0;
            const double refl = obj_row<0>(S, id)[8]; // #material.reflectivity
            const D3 F = shade<GENPOW, 0, NB>(SS, id, dk, hit, N, col, refl, on);
            if (on) col = F;
        }
        if (act) {
            put3<PREC>(rgb, (size_t)i, col);
            if (levels) levels[i] = (uint8_t)(nlev < 255u ? nlev : 255u); // (counts saturate at 255)
        }
    }
}

} // namespace

extern "C" size_t rt_query_colours_work_bytes(uint64_t n, uint32_t depth) { return rt_trace_work_bytes(n, depth); }

extern "C" int rt_query_colours(rt_prepared *p, const double *d_origin, const double *d_dir, uint64_t n, uint32_t depth,
                                uint32_t flags, int precision, void *d_rgb, uint8_t *d_levels, void *d_work,
                                size_t work_bytes, void *stream) {
    const int rc = rt_trace_check_args(p, d_origin, d_dir, n, depth, flags, precision, d_rgb, d_work, work_bytes);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    const rt_scene_view v = rt_prepared_scene(p);
    DevGuard g(v.device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // The kernel's header: a copy with the host-proven shortcuts off (they were proved for the
    // renderer's rays) and, for a scene with a BVH, this launch's dynamic LDS placed in it.
    SceneHdr h = *v.hdr;
    h.norm_ok = h.prim_ok = 0;
    h.l_bvh = h.l_bsph = -1;
    h.l_stack = 0;
    const int scan = !h.cull_ok ? SCAN_BRUTE : h.bvh_ok ? SCAN_BVH : SCAN_BEAM;
    const size_t lds = scan == SCAN_BVH ? bvh_lds_place(h, 0, TRACE_BLOCK) : 0;
    const dim3 grid((unsigned)std::min<uint64_t>((n + TRACE_BLOCK - 1) / TRACE_BLOCK, TRACE_GRID));
    with_prec_pow(precision, h.int_pow != 0, [&](auto pc, auto gp) {
        with_int<SCAN_BRUTE, SCAN_BVH>(scan, [&](auto sc) {
            hipLaunchKernelGGL((k_trace<decltype(pc)::value, decltype(gp)::value, decltype(sc)::value>), grid,
                               dim3(TRACE_BLOCK), lds, st, h, v.tab, v.itab, v.elem_of, d_origin, d_dir,
                               (unsigned long long)n, (int)(flags & RT_QUERY_ONE_ORIGIN), (unsigned)depth,
                               (unsigned long long)rt_trace_stride(n), d_rgb, d_levels, static_cast<char *>(d_work));
        });
    });
    return hipGetLastError() == hipSuccess ? RT_OK : RT_EHIP;
}
