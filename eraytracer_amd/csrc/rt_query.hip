// rt_query.hip — ray queries (RT_QUERY in include/rt_mi355x.h): the nearest hit of rays the caller
// chose (rt_query_rays: nearest_object_intersecting_ray/2, raytracer.erl:300-346) and the shadow test
// between pairs of points (rt_query_shadow: shadow_factor/4, :256-267), over the resident scene.
//
// One kernel family, k_query<PREC, MODE, SCAN>: 256-thread blocks, one ray per lane, a grid-stride
// loop over the batch in waves of 64 consecutive rays.  The rays are anybody's, so everything runs in
// the general forms — the per-ray sphere terms (sphere_BC<false>), sqrt_x<false>, normalize3 with its
// range check, no host-proven shortcut (norm_ok and prim_ok are cleared in the header the kernel
// gets) — and all of it in binary64; RT_OUT_F32 rounds at the store.  The scans, sqrt_x and
// normalize3 reduce across the wave, so a wave stays converged from its loads to the end of the
// geometry: a lane past the batch traces a copy of the last ray with act = false, and only the stores
// are predicated.  What a hit means and how the planes are stored is rt_attrs.hip's (hit_attrs and
// put_hit, rt_planes.inc).
//
// SCAN — how a wave finds the nearest object; every form computes the reference's binary64 tests on
// the objects it keeps and the (t, list position) minimum, so all give the same bits:
//   SCAN_BRUTE  every object (nearest<.., NB>): the header says culling is off
//   SCAN_BEAM   the wave's binary32 beam (nearest<false>, one group): it turns itself off — every
//               sphere scanned — for a wave holding a direction that is not a unit vector, an
//               origin beyond CULL_EXTENT or a cone wider than a hemisphere
//   SCAN_BVH    the scene has a sphere BVH: a wave whose active rays all lie in the domain below
//               walks it per lane (scan_bvh), any other wave takes the beam
//
// The BVH's domain.  scan_bvh has no guard of its own; it was written for the renderer's reflection
// rays (unit directions, origins on objects).  A wave walks it only if every active lane has
//     |o.x|, |o.y|, |o.z| <= 4 E   and   | d.d - 1 | <= 2^-20,        E = hdr.ext + 1
// (a NaN or an infinity fails either test).  Why the walk then drops no sphere the reference's test
// accepts — bvh_ok implies cull_ok, so every centre coordinate and radius is <= hdr.ext < E <= 10001,
// and u = 2^-53:
//  (1) The reported distance is the ray parameter.  sph_t returns t = (-B - sqrt(disc)) / 2, which is
//      the parameter of o + d t only for |d| = 1; the walk prunes boxes whose entry parameter exceeds
//      the best t so far.  With |d.d - 1| <= 2^-20 the two differ by a factor within 1 +- 2^-20.
//  (2) An accepted ray passes the sphere closely.  |o - c| <= 5 E per axis, so |oc|^2 <= 75 E^2; the
//      rounding errors of B^2 (<= 36 u |d|^2 |oc|^2) and of A4 C (<= 4 |d|^2 (8 u max(|oc|^2, r^2) +
//      5 u |C|)) leave the computed discriminant within 7000 u |d|^2 E^2 of the exact one.  disc >=
//      0.001 therefore implies an exact discriminant above -7000 u |d|^2 E^2: the ray's distance p
//      from the centre satisfies p^2 - r^2 <= 1750 u E^2 < 2e-13 E^2, so p <= r + 4.5e-7 E.  The
//      same error in sqrt(disc) >= 0.0316 moves t by at most 7000 u E^2 / 0.063 + 8 u |oc| < 1.3e-11
//      E^2 <= 1.3e-7 E (E <= 10001) against the exact entry parameter.  The point o + d t is thus
//      within 6e-7 E of the ball of radius r.
//  (3) The boxes are wider than that.  Every sphere's box is c +- (|r| + m), m = BVH_BOX_REL (ext' +
//      1) >= 1e-5 E (rt_scene.cpp's ext' >= hdr.ext), rounded outwards to binary32.  The slab test
//      evaluates b * (1/d) - o * (1/d) in binary32: rounding o to binary32 and the product moves a
//      slab bound by at most |o| 2^-22 <= 4 E 2^-22 < 1e-6 E in space, and 1/d (v_rcp_f32 of the
//      rounded component, ~1 ulp) scales a distance by a factor within 1 +- 2^-21.  (2) and this
//      together stay below 1.6e-6 E, a sixth of m.  A component |d_a| < 1e-30 is replaced by 1e-30:
//      over t <= 9 sqrt(3) E the ray moves less than 2e-29 E along that axis, and the slab interval
//      computed, (b - o_a) 1e30, still covers every such t since |b - o_a| > m / 2.  |d_a| <= 1 +
//      2^-21 keeps every reciprocal and product inside binary32's normal range; a product that
//      underflows changes a distance by 2^-126.
//  (4) Hence each box on the path to an accepted sphere has, on every axis, a slab interval
//      containing t (1 +- 2^-20) (1 +- 2^-21), and bvh_slab2's tolerance of 2^-16 on either side, the
//      stack entries' rounding down and tlim = (float)t (1 + 2^-16) all exceed that factor.
// Tighter than scan_bvh strictly needs (8 E would do); nothing is gained by walking the BVH from afar.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"
#include "rt_pick.h"

using namespace rtl;

namespace {

#include "rt_math.inc"    // binary64 primitives, the primitive tests
#include "rt_cull.inc"    // scene access, wave culling, candidate scans, the per-lane BVH
#include "rt_shade.inc"   // nearest-object scans
#include "rt_primary.inc" // hit normals
#include "rt_planes.inc"  // the attribute planes: a hit's attributes, the stores

#include "rt_query.inc"   // SCAN_*, bvh_domain (the BVH's domain, see the top of this file)

constexpr int QUERY_BLOCK = 256; // four waves
constexpr int QUERY_GRID = 8192; // blocks at most: a batch above 2^21 rays loops
enum { MODE_RAYS = 0, MODE_SHADOW = 1 };

// a, b: the rays' origins and directions (MODE_RAYS) or the light and hit points (MODE_SHADOW), n
// triples of doubles each — `a` one triple with one_origin; elem (MODE_SHADOW): the element each
// shadow ray is aimed at.  Results: the planes pl (MODE_RAYS), lit (MODE_SHADOW); entries >= n of
// either are never written.  hdr: norm_ok = prim_ok = 0, and for SCAN_BVH the LDS offsets of this
// launch (l_bvh, l_bsph, l_stack; rt_query_launch below).
template <int PREC, int MODE, int SCAN>
__global__ __launch_bounds__(QUERY_BLOCK) void k_query(SceneHdr hdr, const double *__restrict__ tab,
                                                      const int *__restrict__ itab, const int *__restrict__ elem_of,
                                                      const int *__restrict__ canon_of, int n_elems,
                                                      const double *__restrict__ a, const double *__restrict__ b,
                                                      const int *__restrict__ elem, unsigned long long n, int one_origin,
                                                      HitPlanes pl, uint8_t *__restrict__ lit) {
    const Scene S{hdr, tab, itab};
    if (SCAN == SCAN_BVH) stage_bvh(S); // (every thread of the block: it ends in a barrier)
    const int lane = threadIdx.x & 63;
    const bool want_geom = MODE == MODE_RAYS && (pl.point != nullptr || pl.normal != nullptr);
    const unsigned long long stride = (unsigned long long)gridDim.x * QUERY_BLOCK;
    // base: this wave's first ray (wave-uniform, so the wave's lanes leave the loop together)
    for (unsigned long long base = (unsigned long long)blockIdx.x * QUERY_BLOCK + (threadIdx.x & ~63u); base < n;
         base += stride) {
        const unsigned long long i = base + lane;
        const bool act = i < n;
        const size_t j = (size_t)(act ? i : n - 1); // a lane past the batch: a copy of the last ray, never stored
        const size_t ja = one_origin ? 0 : j;
        const D3 o = {a[ja * 3], a[ja * 3 + 1], a[ja * 3 + 2]};
        D3 d = {b[j * 3], b[j * 3 + 1], b[j * 3 + 2]};
        // shadow_factor/4: from the light towards the hit point, vector_normalize(Hit - Light)
        if (MODE == MODE_SHADOW) d = normalize3(D3{d.x - o.x, d.y - o.y, d.z - o.z});
        double t;
        int id;
        if (SCAN == SCAN_BRUTE) {
            id = nearest<false, false, 0, true>(S, 0, o, d, t, act);
        } else {
            const bool walk = SCAN == SCAN_BVH && __ballot(act && !bvh_domain(o, d, hdr.ext + 1.0)) == 0;
            id = nearest<false, false, 0, false>(S, 0, o, d, t, act, 0, walk);
        }
        const bool any_hit = __ballot(id >= 0) != 0; // (then the scene has an object: row 0 exists)
        if (MODE == MODE_SHADOW) {
            // lit iff the nearest object and element e are the same term: the same canonical element
            int same = 0;
            if (any_hit) { // (wave-uniform; a lane without a hit reads object 0's row, unstored)
                const int e = elem[j];
                const int ce = (e >= 0 && e < n_elems) ? canon_of[e] : -1; // -1: not an object of the scene
                const int ch = elem_of[obj_meta<0>(S, id >= 0 ? id : 0).z];
                same = id >= 0 && ce >= 0 && ce == ch;
            }
            if (act) lit[i] = (uint8_t)same;
            continue;
        }
        const HitAttrs at = hit_attrs(S, elem_of, o, d, id, t, any_hit, want_geom);
        if (act) put_hit<PREC>(pl, i, id, t, at);
    }
}

// One launch of n > 0 queries on p's scene; the arguments are checked.
template <int MODE>
int rt_query_launch(rt_prepared *p, int prec, const double *a, const double *b, const int *elem, uint64_t n,
                    uint32_t flags, const HitPlanes &pl, uint8_t *lit, void *stream) {
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
    const size_t lds = scan == SCAN_BVH ? bvh_lds_place(h, 0, QUERY_BLOCK) : 0;
    const dim3 grid((unsigned)std::min<uint64_t>((n + QUERY_BLOCK - 1) / QUERY_BLOCK, QUERY_GRID));
    // (the shadow answers have no float plane: one PREC)
    with_int<RT_OUT_F64, MODE == MODE_SHADOW ? RT_OUT_F64 : RT_OUT_F32>(prec, [&](auto pc) {
        with_int<SCAN_BRUTE, SCAN_BVH>(scan, [&](auto sc) {
            hipLaunchKernelGGL((k_query<decltype(pc)::value, MODE, decltype(sc)::value>), grid, dim3(QUERY_BLOCK), lds, st,
                               h, v.tab, v.itab, v.elem_of, v.canon_of, v.n_elems, a, b, elem, (unsigned long long)n,
                               (int)(flags & RT_QUERY_ONE_ORIGIN), pl, lit);
        });
    });
    return hipGetLastError() == hipSuccess ? RT_OK : RT_EHIP;
}

} // namespace

extern "C" int rt_query_rays(rt_prepared *p, const double *d_origin, const double *d_dir, uint64_t n, uint32_t flags,
                             const rt_attr_planes *out, void *stream) {
    if (!p || !d_origin || !d_dir || !out) return RT_EBADARG;
    if (flags & ~(uint32_t)RT_QUERY_ONE_ORIGIN) return RT_EBADARG;
    if ((uintptr_t)d_origin % 8 || (uintptr_t)d_dir % 8) return RT_EBADARG;
    HitPlanes hp;
    int prec;
    if (rt_hit_planes(out, &hp, &prec) != RT_OK) return RT_EBADARG;
    if (n > RT_MAX_QUERY_RAYS) return RT_ETOOBIG;
    if (n == 0) return RT_OK;
    return rt_query_launch<MODE_RAYS>(p, prec, d_origin, d_dir, nullptr, n, flags, hp, nullptr, stream);
}

extern "C" int rt_query_shadow(rt_prepared *p, const double *d_light, const double *d_hit, const int32_t *d_elem, uint64_t n,
                               uint32_t flags, uint8_t *d_lit, void *stream) {
    if (!p || !d_light || !d_hit || !d_elem || !d_lit) return RT_EBADARG;
    if (flags & ~(uint32_t)RT_QUERY_ONE_ORIGIN) return RT_EBADARG;
    if ((uintptr_t)d_light % 8 || (uintptr_t)d_hit % 8 || (uintptr_t)d_elem % 4) return RT_EBADARG;
    if (n > RT_MAX_QUERY_RAYS) return RT_ETOOBIG;
    if (n == 0) return RT_OK;
    const HitPlanes none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    return rt_query_launch<MODE_SHADOW>(p, RT_OUT_F64, d_light, d_hit, d_elem, n, flags, none, d_lit, stream);
}
