// rt_cull.inc — scene access and culling, included inside rt_render.hip's anonymous namespace:
// Scene and fresh_scene, the table rows in HBM or staged in LDS (obj_row ... stage_tables), the
// RT_STAT counters, the DPP wave reductions, the binary64 and binary32 beams (Beam, Beam32) with
// their per-chunk cull tests, the candidate scans (scan_spheres, scan_tri_pl) and the per-lane BVH.
// Expects: rt_layout.h (namespace rtl in scope) and rt_math.inc.

struct Scene {
    SceneHdr h;
    const double *__restrict__ tab;
    const int *__restrict__ itab;
};

// The scene header re-read from the kernel argument segment (scalar loads; every kernel here takes
// the SceneHdr its Scene holds as its first argument) instead of being held in SGPRs across a
// long loop: the kernels' uniform values exceed the SGPR file, and spilled ones come back through
// v_readlane on every use (measured on k_reflect_shade: SGPR spills 90 -> 21, config 3 +2 %).
__device__ __forceinline__ Scene fresh_scene(const Scene &S) {
#if defined(__HIP_DEVICE_COMPILE__) // (the host pass has no kernel argument segment)
    typedef __attribute__((address_space(4))) const SceneHdr KHdr;
    KHdr *hp = (KHdr *)(__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(hp)); // opaque: the loads stay where the values are used
    return Scene{*hp, S.tab, S.itab};
#else
    return S;
#endif
}

// ---- scene table access; SPH (template argument of the shading code): 0 = any scene, 1 = spheres
// only (occluder masks), 2 = spheres only with the per-lane-gathered tables staged in LDS.
// Lanes of a wave read these rows by their own object / target / candidate (gathers whose L2
// round trips the shading waits on); staged, they are LDS reads.  Wave-uniform reads stay
// scalar loads from the tables in HBM (scalar cache).
extern __shared__ __attribute__((aligned(16))) char g_lds[];

template <int SPH>
__device__ __forceinline__ const double *obj_row(const Scene &S, int id) {
    if (SPH == 2) return reinterpret_cast<const double *>(g_lds + S.h.l_obj) + id * OBJ_W;
    return S.tab + S.h.o_obj + id * OBJ_W;
}
template <int SPH>
__device__ __forceinline__ int4 obj_meta(const Scene &S, int id) {
    if (SPH == 2) return reinterpret_cast<const int4 *>(g_lds + S.h.l_meta)[id];
    return *reinterpret_cast<const int4 *>(S.itab + S.h.i_obj_meta + id * OBJ_META_W);
}
// per-origin sphere row (o - c, C); staged only for the light origins (org >= 1)
template <int SPH>
__device__ __forceinline__ const double *org_row(const Scene &S, int org, int k) {
    if (SPH == 2) return reinterpret_cast<const double *>(g_lds + S.h.l_org) + ((org - 1) * S.h.n_sph + k) * SPH_ORG_W;
    return S.tab + S.h.o_sph_org + (org * S.h.n_sph + k) * SPH_ORG_W;
}
// occluder masks of `light`, chunk `chunk64`: element (t*OCC_CELLS + e)*n_chunk is the mask of
// target sphere t, direction cell e
template <int SPH>
__device__ __forceinline__ const unsigned long long *occ_masks(const Scene &S, int light, int chunk64) {
    const int w = (light * S.h.n_sph * (SPH == 2 ? 1 : S.h.occ_cells)) * S.h.n_chunk + chunk64; // staged: 1 cell
    if (SPH == 2) return reinterpret_cast<const unsigned long long *>(g_lds + S.h.l_occ) + w;
    return reinterpret_cast<const unsigned long long *>(S.itab + S.h.i_occ) + w;
}
template <int SPH>
__device__ __forceinline__ int sph_id(const Scene &S, int k) {
    if (SPH == 2) return reinterpret_cast<const int *>(g_lds + S.h.l_id)[k];
    return S.itab[S.h.i_sph_id + k];
}
// Copy the staged tables into this workgroup's LDS (every thread of the block, before any use).
// The six offsets, and room for exactly these byte counts, are written by stage_lds_place (rt_layout.h).
template <int SPH>
__device__ __forceinline__ void stage_tables(const Scene &S) {
    if (SPH != 2) return;
    const SceneHdr &h = S.h;
    auto copy16 = [&](int dst, const void *src, int bytes) { // src 16-byte aligned
        const int4 *s4 = reinterpret_cast<const int4 *>(src);
        int4 *d4 = reinterpret_cast<int4 *>(g_lds + dst);
        for (int i = threadIdx.x; i < bytes / 16; i += blockDim.x) d4[i] = s4[i];
    };
    auto copy4 = [&](int dst, const int *src, int n) {
        int *d = reinterpret_cast<int *>(g_lds + dst);
        for (int i = threadIdx.x; i < n; i += blockDim.x) d[i] = src[i];
    };
    copy16(h.l_obj, S.tab + h.o_obj, h.n_obj * OBJ_W * 8);
    copy16(h.l_meta, S.itab + h.i_obj_meta, h.n_obj * OBJ_META_W * 4);
    copy16(h.l_org, S.tab + h.o_sph_org + h.n_sph * SPH_ORG_W, h.n_light * h.n_sph * SPH_ORG_W * 8);
    copy4(h.l_occ, S.itab + h.i_occ, h.n_light * h.n_sph * h.n_chunk * 2); // 1 cell; 8-byte aligned in the int table
    copy4(h.l_id, S.itab + h.i_sph_id, h.n_sph);
    copy16(h.l_sphb, S.tab + h.o_sph_b, h.n_sph * SPH_B_W * 8);
    __syncthreads();
}

// Diagnostic build only (-DRT_STATS): per-wave event counters read back with rt_debug_stats().
#define RT_NSTATS 24
#ifdef RT_STATS
__device__ unsigned long long g_stats[RT_NSTATS];
#define RT_STAT(i, v)                                                                                              \
    do {                                                                                                           \
        const unsigned long long v_ = (v);                                                                         \
        if ((threadIdx.x & 63) == __builtin_ctzll(__ballot(1))) atomicAdd(&g_stats[i], v_);                          \
    } while (0)
#else
#define RT_STAT(i, v) \
    do {              \
    } while (0)
#endif
enum { ST_WAVES, ST_NEAR_PRE, ST_NEAR_PRE_CAND, ST_NEAR_GEN, ST_NEAR_GEN_CAND, ST_SHADOW, ST_SHADOW_CAND,
       ST_SHADOW_ITER, ST_SHADE, ST_SHADOW_CONE_ON, ST_BEAM_ON, ST_SHADOW_LANES, ST_NEAR_LANES, ST_BVH_SCANS,
       ST_BVH_ITER, ST_BVH_LEAF, ST_BVH_ITER_LANES, ST_BVH_LEAF_LANES,
       ST_PRIM_WAVES, ST_PRIM_EMPTY, ST_PRIM_FILL }; // k_primary: its waves, those with all-zero masks, those filling wide

// ---- Beam culling ----------------------------------------------------------------------------
// A wave's 64 rays are coherent (an 8x8 pixel tile; shadow rays of one light; their
// reflections).  Before a sphere scan the wave bounds its active rays by a cone of
// directions (axis a, half-angle theta given by a lower bound c on cos and an upper bound s
// on sin) around an origin ball (centre m, radius ro; ro = 0 for the camera and the
// lights).  Lane j then tests sphere j of a 64-sphere chunk against that beam and a ballot
// yields the chunk's candidate mask; the scan visits only candidates, with a wave-uniform
// index (scalar loads).  A sphere is dropped only if its angular distance phi from the axis
// exceeds theta + rho, rho = asin((r + ro) / |c - m|): then no ray of the beam comes within
// r of the centre, and the reference's test (disc >= 0.001 and both roots >= 0, :378-381)
// cannot succeed — its rounding error is < 1e-9 of the threshold for scenes within
// CULL_EXTENT, and every bound below carries a CULL_EPS margin in the safe direction.
// Wave reductions of binary64 values without LDS: four DPP steps reduce each 16-lane row
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror — each an involution, so every lane
// of a row ends with the same value), then the four row results are read into SGPRs.  The
// wave must be converged (all 64 lanes active).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double lane_f64(double v, int lane) { // v of `lane`, in SGPRs
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((int)b, lane);
    const unsigned hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
// (combining the four rows with row_bcast:15 / row_bcast:31 and one readlane of lane 63 measured within
// noise on configs 3 and 5: profiles/r06m_ab_dpp_row_bcast.txt)
template <typename Op>
__device__ __forceinline__ double wave_reduce(double v, Op op) {
    v = op(v, dpp_f64<DPP_XOR1>(v));
    v = op(v, dpp_f64<DPP_XOR2>(v));
    v = op(v, dpp_f64<DPP_HALF_MIRROR>(v));
    v = op(v, dpp_f64<DPP_MIRROR>(v));
    return op(op(lane_f64(v, 0), lane_f64(v, 16)), op(lane_f64(v, 32), lane_f64(v, 48)));
}
__device__ __forceinline__ double wave_sum(double v) {
    return wave_reduce(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double wave_min(double v) {
    return wave_reduce(v, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ double wave_max(double v) {
    return wave_reduce(v, [](double a, double b) { return fmax(a, b); });
}
// every lane holds the same v: keep it in SGPRs
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long b) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double uniform(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct Beam {
    double ax, ay, az; // unit axis
    double c, s;       // cos(theta) lower bound, sin(theta) upper bound
    double mx, my, mz; // origin ball centre (unused when the origin is tabled)
    double ro;         // origin ball radius
    bool on;
};

// Must be called with the whole wave converged (it reduces across lanes).
__device__ __forceinline__ Beam make_beam(const SceneHdr &h, bool act, const D3 &o, const D3 &d, bool fixed_origin) {
    Beam b;
    b.on = false;
    b.ax = b.ay = b.az = b.c = b.s = b.mx = b.my = b.mz = b.ro = 0.0;
    const unsigned long long am = __ballot(act);
    if (!h.beam_ok || am == 0) return b;
    // Axis: the (normalised) direction of one active lane — the tile centre when it is active.
    // Any axis inside the bundle gives a valid cone, at most twice as wide as the best one.
    const int al = ((am >> 27) & 1) ? 27 : __builtin_ctzll(am);
    const double rx = lane_f64(d.x, al), ry = lane_f64(d.y, al), rz = lane_f64(d.z, al);
    const double n2 = rx * rx + ry * ry + rz * rz;
    if (!(n2 > 0.0)) return b;
    const double inv = uniform(1.0 / sqrt(n2));
    const double ax = rx * inv, ay = ry * inv, az = rz * inv;
    // The rays traced here are unit vectors to ~1e-15 (normalize/1 and bounces off unit
    // normals).  Lanes are only required to have |d|^2 within DIR_TOL of 1, and the bounds are
    // widened by 2*DIR_TOL instead of dividing by |d| (a plane normal that is not unit makes
    // its reflections fail the check: that wave simply scans every sphere).
    constexpr double DIR_TOL = 1.0e-6;
    const double dd = d.x * d.x + d.y * d.y + d.z * d.z;
    const double cl = ax * d.x + ay * d.y + az * d.z;
    const double qx = ay * d.z - az * d.y, qy = az * d.x - ax * d.z, qz = ax * d.y - ay * d.x;
    const double sl = sqrt(qx * qx + qy * qy + qz * qz);
    const bool bad = act && !(dd > 1.0 - DIR_TOL && dd < 1.0 + DIR_TOL);
    const double c = uniform(wave_min(act ? cl : 2.0)) - CULL_EPS - 2 * DIR_TOL;
    const double s = uniform(wave_max(act ? sl : 0.0)) + CULL_EPS + 2 * DIR_TOL;
    if (__ballot(bad) != 0 || !(c > 0.0)) return b; // cone wider than a hemisphere: scan everything
    b.ax = ax; b.ay = ay; b.az = az; b.c = c; b.s = s;
    if (!fixed_origin) {
        const int first = __builtin_ctzll(am);
        b.mx = lane_f64(o.x, first);
        b.my = lane_f64(o.y, first);
        b.mz = lane_f64(o.z, first);
        const double ex = o.x - b.mx, ey = o.y - b.my, ez = o.z - b.mz;
        const double r2 = wave_max(act ? ex * ex + ey * ey + ez * ez : 0.0);
        const double mo = wave_max(act ? fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z))) : 0.0);
        if (!(uniform(mo) <= CULL_EXTENT)) return b;
        b.ro = uniform(sqrt(r2)) * (1 + CULL_EPS) + CULL_EPS;
    }
    b.on = true;
    return b;
}

// Candidate mask of spheres [chunk, chunk+64): lane j tests sphere chunk+j against the beam.
// org >= 0: the beam starts at tabled origin `org` (camera / light) and uses its cone table;
// a sphere whose nearest surface point is farther than tmax from the origin is dropped too
// (its hits have t > tmax; shadow scans only care about t <= t*, and t* <= tmax).
template <int SPH = 0>
__device__ __forceinline__ unsigned long long cull_chunk(const Scene &S, const Beam &b, int chunk, int org,
                                                         double tmax = __builtin_inf()) {
    // Branch-free: every load of the record is issued at once and the decision is a mask.
    const SceneHdr &h = S.h;
    const int k = chunk + (int)(threadIdx.x & 63);
    const bool in = k < h.n_sph;
    const int kk = in ? k : 0;
    bool keep;
    if (org >= 0) { // wave-uniform
        const double2 *q = reinterpret_cast<const double2 *>(S.tab + h.o_sph_ob + (org * h.n_sph + kk) * SPH_OB_W);
        const double2 q01 = q[0], q23 = q[1], q45 = q[2], q67 = q[3];
        const double thr = b.c * q45.y - b.s * q45.x;                  // <= cos(theta + rho)
        const double av = b.ax * q01.x + b.ay * q01.y + b.az * q23.x;  // |v| cos(phi)
        keep = ((q67.x != 0.0) | !(av + CULL_EPS * q23.y < thr * q23.y)) & !(q67.y > tmax);
    } else {
        const double2 *g = SPH == 2 ? reinterpret_cast<const double2 *>(g_lds + h.l_sphb) + kk * (SPH_B_W / 2)
                                    : reinterpret_cast<const double2 *>(S.tab + h.o_sph_b + kk * SPH_B_W);
        const double2 g01 = g[0], g23 = g[1];
        const double vx = g01.x - b.mx, vy = g01.y - b.my, vz = g23.x - b.mz;
        const double vl = sqrt(vx * vx + vy * vy + vz * vz);
        const double rp = g23.y + b.ro;
        const double sr = rp / vl * (1 + CULL_EPS) + CULL_EPS;
        const double cr = sqrt(fmax(1.0 - sr * sr, 0.0)) - CULL_EPS;
        const double thr = b.c * cr - b.s * sr;
        const double av = b.ax * vx + b.ay * vy + b.az * vz;
        keep = (vl <= rp * (1 + CULL_EPS) + CULL_EPS) | (sr >= 1.0) | !(av + CULL_EPS * vl < thr * vl);
    }
    return __ballot(in & keep);
}

// ---- Binary32 beams for reflection rays ------------------------------------------------------
// The reflection scans' beams (origin ball + direction cone over a group of lanes) and their
// per-sphere cull tests are filters: they only have to keep every sphere some ray of the group
// can hit.  They run in binary32 (hardware sqrt / reciprocal, half the issue cost of binary64,
// single-register DPP reductions) with margins far above binary32 rounding: BEAM32_EPS (1e-5,
// vs ~1e-6 accumulated relative error in the O(1) cosines and sines), and the positions' rounding
// (|x| * 2^-24 per coordinate) covered by widening the origin ball by (|origins| + extent) * 1e-6.
// Their square roots are the hardware's v_sqrt_f32 (sqrt_f32f: within ~1 ulp, 2^-23 relative, far
// inside those margins) — the correctly rounded sqrtf the compiler emits under IEEE rules is
// that instruction wrapped in a dozen fix-up operations per call.
// The axis need not be a unit vector: the cone bounds and the sphere test scale with |axis| alike.
struct Beam32 {
    float ax, ay, az; // axis (about unit)
    float c, s;       // lower bound of the lanes' a.d, upper bound of |a x d|
    float mx, my, mz; // origin ball centre
    float ro;         // origin ball radius, position rounding included
    bool on;
};
__device__ __forceinline__ float lane_f32(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float sqrt_f32f(float x) { return __builtin_amdgcn_sqrtf(x); } // the filters' sqrt
// Wave minimum / maximum of binary32 values by their bit patterns as signed integers, which order
// as the values do for every value >= +0 (lengths, radii, extents: the maxima here).  For the
// minima (the beams' cosine bounds) a negative value anywhere gives some negative result, not
// necessarily the least, and a negative bound is all the callers test for (the beam is off): the
// same decisions.  A NaN (positive as an integer) goes into a maximum, where it turns the beam off
// or keeps every sphere.  Integer min/max need no NaN canonicalisation, so each DPP step is one
// v_min/max_i32_dpp (bound_ctrl: these four permutations read no invalid lane), and the four rows'
// results are read and combined — against a v_mov, a v_mov_dpp and a canonicalising v_max around
// every fminf / fmaxf step.  (Combining them with s_min/s_max in inline asm measured slower:
// profiles/r06ab_ab_salu_bvh_knobs.txt.)
template <bool MAX>
__device__ __forceinline__ float wave_ext32(float x) {
    auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    int v = __float_as_int(x);
    v = op(v, __builtin_amdgcn_mov_dpp(v, DPP_XOR1, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, DPP_XOR2, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, DPP_HALF_MIRROR, 0xF, 0xF, true));
    v = op(v, __builtin_amdgcn_mov_dpp(v, DPP_MIRROR, 0xF, 0xF, true));
    return __int_as_float(op(op(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
                             op(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48))));
}
__device__ __forceinline__ float wave_min32(float x) { return wave_ext32<false>(x); }
__device__ __forceinline__ float wave_max32(float x) { return wave_ext32<true>(x); }
// Must be called with the whole wave converged.  o, d: the lanes' ray origins and directions.
// SPHO: a spheres-only scene's reflection rays — every origin is a hit point on a sphere, so its
// coordinates are within 2 h.ext (h.ext bounds |centre| and |radius| alike; the binary64 hit point's
// rounding is ~1e-16 of that), which replaces the wave maximum of |origin|; and every direction is a
// reflection off a normalised sphere normal of a normalised ray, of unit length to ~1e-15 per level,
// so the DIR_TOL check (which catches the reflections off planes with non-unit normals) cannot fail.
template <bool SPHO = false>
__device__ __forceinline__ Beam32 make_beam32(const SceneHdr &h, bool act, const D3 &o, const D3 &d) {
    Beam32 b;
    b.on = false;
    b.ax = b.ay = b.az = b.c = b.s = b.mx = b.my = b.mz = b.ro = 0.0f;
    const unsigned long long am = __ballot(act);
    if (!h.beam_ok || am == 0) return b;
    const int al = ((am >> 27) & 1) ? 27 : __builtin_ctzll(am);
    const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
    const float rx = lane_f32(dx, al), ry = lane_f32(dy, al), rz = lane_f32(dz, al);
    const float n2 = rx * rx + ry * ry + rz * rz;
    if (!(n2 > 1.0e-6f)) return b;
    const float inv = __builtin_amdgcn_rsqf(n2);
    const float ax = rx * inv, ay = ry * inv, az = rz * inv;
    // the lanes' directions are unit vectors to ~1e-15 (make_beam); bounds widened by 2 * DIR_TOL
    constexpr float DIR_TOL = 1.0e-6f;
    const float dd = dx * dx + dy * dy + dz * dz;
    const float cl = ax * dx + ay * dy + az * dz;
    const bool bad = !SPHO && act && !(dd > 1.0f - 0.5f * DIR_TOL && dd < 1.0f + 0.5f * DIR_TOL);
    const float cmin = wave_min32(act ? cl : 2.0f);
    const float c = cmin - BEAM32_EPS - 2 * DIR_TOL;
    if (__ballot(bad) != 0 || !(c > 0.0f)) return b; // cone wider than a hemisphere: scan everything
    // The sine bound from the cosine bound: every lane has cos >= cmin (to f32 rounding, ~1e-6 with
    // the directions' and the axis' deviation from unit length), so sin^2 = |a|^2 |d|^2 - cos^2 <=
    // 1 + 4 DIR_TOL - cmin^2 (0 < cmin <= 1) — no second reduction (nor the lanes' cross products).
    const float s = sqrt_f32f(fmaxf(1.0f + 4 * DIR_TOL - cmin * cmin, 0.0f)) + BEAM32_EPS + 2 * DIR_TOL;
    const int first = __builtin_ctzll(am);
    const float ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
    b.mx = lane_f32(ox, first);
    b.my = lane_f32(oy, first);
    b.mz = lane_f32(oz, first);
    const float ex = ox - b.mx, ey = oy - b.my, ez = oz - b.mz;
    const float r2 = wave_max32(act ? ex * ex + ey * ey + ez * ez : 0.0f);
    // the origins' extent in binary32 (|o| rounded to nearest: within 2^-24 relative, far inside the
    // 1e-6 margin below; the extent check keeps a 1e-6 relative slack for it)
    const float mo = SPHO ? (float)(2.0 * h.ext) * (1.0f + 1.0e-6f)
                          : wave_max32(act ? fmaxf(fabsf(ox), fmaxf(fabsf(oy), fabsf(oz))) : 0.0f);
    if (!(mo <= (float)(CULL_EXTENT * (1.0 - 1.0e-6)))) return b;
    b.ax = ax; b.ay = ay; b.az = az; b.c = c; b.s = s;
    b.ro = sqrt_f32f(r2) * (1.0f + BEAM32_EPS) + BEAM32_EPS + (mo + (float)h.ext) * 1.0e-6f;
    b.on = true;
    return b;
}
// Candidate mask of spheres [chunk, chunk+64) for a binary32 beam (lane j tests sphere chunk+j).
template <int SPH = 0>
__device__ __forceinline__ unsigned long long cull_chunk32(const Scene &S, const Beam32 &b, int chunk) {
    const SceneHdr &h = S.h;
    const int k = chunk + (int)(threadIdx.x & 63);
    const bool in = k < h.n_sph;
    const int kk = in ? k : 0;
    const double2 *g = SPH == 2 ? reinterpret_cast<const double2 *>(g_lds + h.l_sphb) + kk * (SPH_B_W / 2)
                                : reinterpret_cast<const double2 *>(S.tab + h.o_sph_b + kk * SPH_B_W);
    const double2 g01 = g[0], g23 = g[1];
    const float vx = (float)g01.x - b.mx, vy = (float)g01.y - b.my, vz = (float)g23.x - b.mz;
    const float vl = sqrt_f32f(vx * vx + vy * vy + vz * vz);
    const float rp = (float)g23.y + b.ro;
    const float sr = rp * __builtin_amdgcn_rcpf(vl) * (1.0f + BEAM32_EPS) + BEAM32_EPS;
    const float cr = sqrt_f32f(fmaxf(1.0f - sr * sr, 0.0f)) - BEAM32_EPS;
    const float thr = b.c * cr - b.s * sr;
    const float av = b.ax * vx + b.ay * vy + b.az * vz;
    const bool keep = (vl <= rp * (1.0f + BEAM32_EPS) + BEAM32_EPS) | (sr >= 1.0f) | !(av + BEAM32_EPS * vl < thr * vl);
    return __ballot(in & keep);
}

// Tabled origin `org` (camera, lights): the host's binary32 cone rows (SPH_OB32_W); a sphere whose
// nearest surface point is farther than tmax from the origin is dropped too.
__device__ __forceinline__ unsigned long long cull_chunk32_org(const Scene &S, const Beam32 &b, int chunk, int org,
                                                               float tmax = __builtin_inff()) {
    const SceneHdr &h = S.h;
    const int k = chunk + (int)(threadIdx.x & 63);
    const bool in = k < h.n_sph;
    const int kk = in ? k : 0;
    const float4 *q = reinterpret_cast<const float4 *>(S.tab + h.o_sph_ob32) + (size_t)(org * h.n_sph + kk) * 2;
    const float4 v = q[0], w = q[1]; // (vx vy vz |v|) (sin, cos, near, dlow)
    const float thr = b.c * w.y - b.s * w.x;
    const float av = b.ax * v.x + b.ay * v.y + b.az * v.z;
    const bool keep = ((w.z != 0.0f) | !(av + BEAM32_EPS * v.w < thr * v.w)) & !(w.w > tmax);
    return __ballot(in & keep);
}

// Beam of a wave holding two primary rays per lane (an 8x16 pixel block) from a tabled origin:
// make_beam32's cone over both ray sets (no origin ball).
__device__ __forceinline__ Beam32 make_beam_pair32(const SceneHdr &h, bool a0, const D3 &d0, bool a1, const D3 &d1) {
    Beam32 b;
    b.on = false;
    b.ax = b.ay = b.az = b.c = b.s = b.mx = b.my = b.mz = b.ro = 0.0f;
    const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
    if (!h.beam_ok || (m0 | m1) == 0) return b;
    const float x0 = (float)d0.x, y0 = (float)d0.y, z0 = (float)d0.z;
    const float x1 = (float)d1.x, y1 = (float)d1.y, z1 = (float)d1.z;
    // axis: the ray of pixel (3, 7) of the block (set 0, lane 59), else the first active ray
    float rx, ry, rz;
    if ((m0 >> 59) & 1) {
        rx = lane_f32(x0, 59); ry = lane_f32(y0, 59); rz = lane_f32(z0, 59);
    } else if (m0) {
        const int l = __builtin_ctzll(m0);
        rx = lane_f32(x0, l); ry = lane_f32(y0, l); rz = lane_f32(z0, l);
    } else {
        const int l = __builtin_ctzll(m1);
        rx = lane_f32(x1, l); ry = lane_f32(y1, l); rz = lane_f32(z1, l);
    }
    const float n2 = rx * rx + ry * ry + rz * rz;
    if (!(n2 > 1.0e-6f)) return b;
    const float inv = __builtin_amdgcn_rsqf(n2);
    const float ax = rx * inv, ay = ry * inv, az = rz * inv;
    constexpr float DIR_TOL = 1.0e-6f; // as in make_beam32
    auto lane_terms = [&](bool a, float dx, float dy, float dz, float &cl) {
        const float dd = dx * dx + dy * dy + dz * dz;
        cl = ax * dx + ay * dy + az * dz;
        return a && !(dd > 1.0f - 0.5f * DIR_TOL && dd < 1.0f + 0.5f * DIR_TOL);
    };
    float cl0, cl1;
    const bool bad0 = lane_terms(a0, x0, y0, z0, cl0); // both sets evaluated (no short circuit)
    const bool bad1 = lane_terms(a1, x1, y1, z1, cl1);
    const float cmin = wave_min32(fminf(a0 ? cl0 : 2.0f, a1 ? cl1 : 2.0f));
    const float c = cmin - BEAM32_EPS - 2 * DIR_TOL;
    if (__ballot(bad0 || bad1) != 0 || !(c > 0.0f)) return b;
    const float s = sqrt_f32f(fmaxf(1.0f + 4 * DIR_TOL - cmin * cmin, 0.0f)) + BEAM32_EPS + 2 * DIR_TOL; // make_beam32
    b.ax = ax; b.ay = ay; b.az = az; b.c = c; b.s = s;
    b.on = true;
    return b;
}

__device__ __forceinline__ unsigned long long chunk_all(int n_sph, int chunk) {
    const int n = n_sph - chunk;
    return n >= 64 ? ~0ull : ((1ull << n) - 1);
}

// The sphere candidates in mask m of chunk `chunk`, folded into the running nearest (bt, bid).
// Two candidates per step: the (t, list position) minimum does not depend on the order the
// candidates are visited, and the two tests are independent, which gives the wave
// instruction-level parallelism across the scalar loads and the root computations.
template <bool PRE>
__device__ __forceinline__ void sphere_BC(const Scene &S, int org, const D3 &o, const D3 &d, int k, double &B,
                                          double &C) {
    const SceneHdr &h = S.h;
    if (PRE) {
        const double *q = S.tab + h.o_sph_org + (org * h.n_sph + k) * SPH_ORG_W;
        B = 2 * (d.x * q[0] + d.y * q[1] + d.z * q[2]);
        C = q[3];
    } else {
        const double *s = S.tab + h.o_sph + k * SPH_W;
        D3 oc = {o.x - s[0], o.y - s[1], o.z - s[2]};
        B = 2 * (d.x * oc.x + d.y * oc.y + d.z * oc.z);
        C = oc.x * oc.x + oc.y * oc.y + oc.z * oc.z - s[3];
    }
}
// ILP = false: one candidate per step (the least work: dense, throughput-bound waves).
template <bool PRE, bool ILP = false, bool FAST = false>
__device__ __forceinline__ void scan_spheres(const Scene &S, int org, const D3 &o, const D3 &d, double A4, int chunk,
                                             unsigned long long m, double &bt, int &bid) {
    const SceneHdr &h = S.h;
    RT_STAT(PRE ? ST_NEAR_PRE_CAND : ST_NEAR_GEN_CAND, __popcll(m));
    // (the walk's scalar loads one candidate ahead — the next row and list position requested before
    // the current candidate is tested — measured config 3 +0.8 %, config 2 +1.3 %, config 5 neutral:
    // profiles/r05ak_ab_scan_scalar_prefetch.txt)
    while (!ILP && m) {
        const int k = chunk + __builtin_ctzll(m);
        m &= m - 1;
        double B, C;
        sphere_BC<PRE>(S, org, o, d, k, B, C);
        const int id = S.itab[h.i_sph_id + k];
        double t;
        const bool upd = (int)sph_t_wave<FAST>(B, C, A4, t) & (int)nearer(t, id, bt, bid);
        bt = upd ? t : bt;
        bid = upd ? id : bid;
    }
    while (ILP && m) {
        const int k0 = chunk + __builtin_ctzll(m);
        m &= m - 1;
        const bool two = m != 0;
        const int k1 = two ? chunk + __builtin_ctzll(m) : k0;
        if (two) m &= m - 1;
        double B0, C0, B1, C1;
        sphere_BC<PRE>(S, org, o, d, k0, B0, C0);
        sphere_BC<PRE>(S, org, o, d, k1, B1, C1);
        const int id0 = S.itab[h.i_sph_id + k0], id1 = S.itab[h.i_sph_id + k1];
        // sph_t for both, without divergent branches; the roots only if some lane can hit
        const double disc0 = B0 * B0 - A4 * C0, disc1 = B1 * B1 - A4 * C1;
        const bool ok0 = disc0 >= 0.001, ok1 = disc1 >= 0.001;
        if (__ballot(ok0 | ok1) == 0) continue;
        const double sq0 = sqrt_x<FAST>(FAST || ok0 ? disc0 : 1.0), sq1 = sqrt_x<FAST>(FAST || ok1 ? disc1 : 1.0); // (sph_t_wave)
        const double t0 = (-B0 - sq0) / 2, t1 = (-B1 - sq1) / 2; // the nearer roots (sph_t)
        const bool h0 = ok0 & (t0 >= 0), h1 = two & ok1 & (t1 >= 0);
        const bool u0 = h0 & nearer(t0, id0, bt, bid);
        bt = u0 ? t0 : bt;
        bid = u0 ? id0 : bid;
        const bool u1 = h1 & nearer(t1, id1, bt, bid);
        bt = u1 ? t1 : bt;
        bid = u1 ? id1 : bid;
    }
}

// The triangles and planes of the scene, folded into the running nearest (bt, bid).
template <bool PRE>
__device__ __forceinline__ void scan_tri_pl(const Scene &S, int org, const D3 &o, const D3 &d, double &bt, int &bid) {
    const SceneHdr &h = S.h;
    for (int k = 0; k < h.n_tri; ++k) {
        const double *g = S.tab + h.o_tri + k * TRI_W;
        D3 e1 = {g[3], g[4], g[5]}, e2 = {g[6], g[7], g[8]};
        D3 T, Q;
        if (PRE) {
            const double *q = S.tab + h.o_tri_org + (org * h.n_tri + k) * TRI_ORG_W;
            T = D3{q[0], q[1], q[2]};
            Q = D3{q[3], q[4], q[5]};
        } else {
            T = D3{o.x - g[0], o.y - g[1], o.z - g[2]};
            Q = D3{T.y * e1.z - T.z * e1.y, T.z * e1.x - T.x * e1.z, T.x * e1.y - T.y * e1.x};
        }
        double t;
        if (tri_t(d, e1, e2, T, Q, t)) {
            int id = S.itab[h.i_tri_id + k];
            if (nearer(t, id, bt, bid)) { bt = t; bid = id; }
        }
    }
    for (int k = 0; k < h.n_pl; ++k) {
        const double *p = S.tab + h.o_pl + k * PL_W;
        D3 n = {p[0], p[1], p[2]};
        double V0 = PRE ? S.tab[h.o_pl_org + org * h.n_pl + k] : -(n.x * o.x + n.y * o.y + n.z * o.z + p[3]);
        double t;
        if (pl_t(n, d, V0, t)) {
            int id = S.itab[h.i_pl_id + k];
            if (nearer(t, id, bt, bid)) { bt = t; bid = id; }
        }
    }
}

// ---- Per-lane BVH (incoherent reflection rays) ------------------------------------------------
// Deep reflection levels of large scenes leave every wave's rays pointing everywhere: a wave
// beam then keeps most spheres (S256 depth 8: ~200 of 256 candidates per scan).  Those scans
// walk the host-built sphere BVH instead, each lane on its own ray (ordered traversal: both
// children's boxes tested, the nearer visited first, the other pushed with its entry distance).
// The box tests are binary32 slab tests on boxes rounded outwards and inflated (rt_scene.cpp), a
// conservative filter with a relative tolerance of 2^-16 on every distance compared; a sphere
// leaf that passes is tested with the reference's binary64 expressions (sphere_BC + sph_t), and
// the (t, list position) minimum does not depend on the visiting order, so the result is the
// candidate walk's.  Each lane's stack holds (entry distance rounded down to bfloat16, node) in
// one word, in LDS (BVH_STACK words per lane, lane-interleaved: no bank conflicts).
__device__ __forceinline__ float bvh_inv(double d) {
    float f = (float)d;
    f = fabsf(f) < 1.0e-30f ? copysignf(1.0e-30f, f) : f; // no inf * 0 in the slab test
    return __builtin_amdgcn_rcpf(f);                       // ~1 ulp: inside the tolerance
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct BvhRay {
    f32x2 ix, iy, iz;    // 1 / d (binary32, both lanes of the pair)
    f32x2 nox, noy, noz; // -(o * (1 / d))
};
__device__ __forceinline__ BvhRay bvh_ray(const D3 &o, const D3 &d) {
    BvhRay r;
    const float ix = bvh_inv(d.x), iy = bvh_inv(d.y), iz = bvh_inv(d.z);
    r.ix = f32x2{ix, ix};
    r.iy = f32x2{iy, iy};
    r.iz = f32x2{iz, iz};
    r.nox = f32x2{-((float)o.x * ix), -((float)o.x * ix)};
    r.noy = f32x2{-((float)o.y * iy), -((float)o.y * iy)};
    r.noz = f32x2{-((float)o.z * iz), -((float)o.z * iz)};
    return r;
}
// Slab tests of both children of a node: [tn, tx] of each box along the ray, clipped to [0, tlim];
// h0/h1 true where they overlap (tolerant).  The distances are b * (1/d) - o * (1/d) (one packed fma
// per axis and bound); its cancellation error, <= 2^-23 * extent * |1/d|, is far inside the boxes'
// inflation (BVH_BOX_REL * (extent + 1) in space, i.e. that times |1/d| in distance).
__device__ __forceinline__ void bvh_slab2(const BvhRay &r, const float4 &a, const float4 &b, const float4 &c, float tlim,
                                          bool &h0, float &tn0, bool &h1, float &tn1) {
    constexpr float LO = 1.0f - 0x1p-16f, HI = 1.0f + 0x1p-16f;
    const f32x2 tlx = __builtin_elementwise_fma(f32x2{a.x, a.y}, r.ix, r.nox);
    const f32x2 tly = __builtin_elementwise_fma(f32x2{a.z, a.w}, r.iy, r.noy);
    const f32x2 tlz = __builtin_elementwise_fma(f32x2{b.x, b.y}, r.iz, r.noz);
    const f32x2 tux = __builtin_elementwise_fma(f32x2{b.z, b.w}, r.ix, r.nox);
    const f32x2 tuy = __builtin_elementwise_fma(f32x2{c.x, c.y}, r.iy, r.noy);
    const f32x2 tuz = __builtin_elementwise_fma(f32x2{c.z, c.w}, r.iz, r.noz);
    tn0 = fmaxf(fmaxf(fminf(tlx.x, tux.x), fminf(tly.x, tuy.x)), fmaxf(fminf(tlz.x, tuz.x), 0.0f));
    tn1 = fmaxf(fmaxf(fminf(tlx.y, tux.y), fminf(tly.y, tuy.y)), fmaxf(fminf(tlz.y, tuz.y), 0.0f));
    const float tx0 = fminf(fminf(fmaxf(tlx.x, tux.x), fmaxf(tly.x, tuy.x)), fminf(fmaxf(tlz.x, tuz.x), tlim));
    const float tx1 = fminf(fminf(fmaxf(tlx.y, tux.y), fmaxf(tly.y, tuy.y)), fminf(fmaxf(tlz.y, tuz.y), tlim));
    const f32x2 n = f32x2{tn0, tn1} * f32x2{LO, LO}, x = f32x2{tx0, tx1} * f32x2{HI, HI};
    h0 = n.x <= x.x;
    h1 = n.y <= x.y;
}
// Stage the BVH nodes and the sphere rows in this workgroup's LDS (every thread of the block,
// before any traversal) when the launch placed them there (l_bvh >= 0).
__device__ __forceinline__ void stage_bvh(const Scene &S) {
    const SceneHdr &h = S.h;
    if (h.l_bvh < 0) return;
    const int4 *sn = reinterpret_cast<const int4 *>(S.tab + h.o_bvh);
    int4 *dn = reinterpret_cast<int4 *>(g_lds + h.l_bvh);
    for (int i = threadIdx.x; i < h.n_bvh * 4; i += blockDim.x) dn[i] = sn[i];
    if (h.l_bsph >= 0) {
        const int4 *ss = reinterpret_cast<const int4 *>(S.tab + h.o_sph);
        int4 *ds = reinterpret_cast<int4 *>(g_lds + h.l_bsph);
        for (int i = threadIdx.x; i < h.n_sph * 2; i += blockDim.x) ds[i] = ss[i];
    }
    __syncthreads();
}
// LDS: the nodes are staged in LDS (h.l_bvh >= 0), ROWS: the sphere rows too (h.l_bsph >= 0);
// else read from HBM (L2)
template <bool LDS, bool ROWS, bool FAST = false>
__device__ __forceinline__ void scan_bvh(const Scene &S, const D3 &o, const D3 &d, double A4, bool act, double &bt,
                                         int &bid) {
    const SceneHdr &h = S.h;
    const float4 *nodes = LDS ? reinterpret_cast<const float4 *>(g_lds + h.l_bvh)
                              : reinterpret_cast<const float4 *>(S.tab + h.o_bvh);
    const double2 *rows = ROWS ? reinterpret_cast<const double2 *>(g_lds + h.l_bsph)
                               : reinterpret_cast<const double2 *>(S.tab + h.o_sph);
    unsigned *stk = reinterpret_cast<unsigned *>(g_lds + h.l_stack) + (threadIdx.x >> 6) * (64 * h.bvh_depth) +
                    (threadIdx.x & 63);
    const BvhRay ray = bvh_ray(o, d);
    constexpr float HI = 1.0f + 0x1p-16f;
    float tlim = __builtin_inff();
    // sphere k (local index, compact id id), as sphere_BC<false> + sph_t (the candidate walk's
    // expressions)
    auto leaf = [&](int k, int id) {
        RT_STAT(ST_BVH_LEAF, 1);
        RT_STAT(ST_BVH_LEAF_LANES, __popcll(__ballot(1)));
        const double2 c01 = rows[k * 2], c2r = rows[k * 2 + 1];
        const D3 oc = {o.x - c01.x, o.y - c01.y, o.z - c2r.x};
        const double B = 2 * (d.x * oc.x + d.y * oc.y + d.z * oc.z);
        const double C = oc.x * oc.x + oc.y * oc.y + oc.z * oc.z - c2r.y;
        double t;
        // (as one divergent block — sph_t_wave and the nearer test as a mask — measured neutral:
        // profiles/r05ag_ab_bvh_leaf_block.txt)
        if (sph_t<FAST>(B, C, A4, t) && nearer(t, id, bt, bid)) {
            bt = t;
            bid = id;
            tlim = (float)t * HI;
        }
    };
    int node = act ? 0 : -1, sp = 0;
    RT_STAT(ST_BVH_SCANS, 1);
    // the next node from the stack: the nearest pushed entry not beyond tlim (-1: traversal done)
    auto pop = [&]() {
        node = -1;
        while (sp > 0) {
            const unsigned en = stk[--sp * 64];
            if (__uint_as_float(en & 0xffff0000u) <= tlim) {
                node = (int)(en & 0xffffu);
                break;
            }
        }
    };
    // one visit of `node`: both children's boxes tested; the leaves among those hit are returned
    // in l0 / l1, the nearer inner child hit becomes `node` (the farther one pushed), else -1
    auto visit = [&](bool &l0, bool &l1, float4 &e) {
        RT_STAT(ST_BVH_ITER, 1);
        RT_STAT(ST_BVH_ITER_LANES, __popcll(__ballot(1)));
        const float4 a = nodes[node * 4], b = nodes[node * 4 + 1], c = nodes[node * 4 + 2];
        e = nodes[node * 4 + 3];
        float tn0, tn1;
        bool h0, h1;
        bvh_slab2(ray, a, b, c, tlim, h0, tn0, h1, tn1);
        const int c0 = __float_as_int(e.x), c1 = __float_as_int(e.y);
        l0 = h0 && c0 < 0;
        l1 = h1 && c1 < 0;
        h0 = h0 && !l0;
        h1 = h1 && !l1;
        if (h0 && h1) {
            const bool f0 = tn0 <= tn1;
            const float tf = f0 ? tn1 : tn0;
            stk[sp * 64] = (__float_as_uint(tf) & 0xffff0000u) | (unsigned)(f0 ? c1 : c0); // tf >= 0: truncation rounds down
            ++sp;
            node = f0 ? c0 : c1;
        } else {
            node = (h0 | h1) ? (h0 ? c0 : c1) : -1;
        }
    };
    // the leaves a visit returned, child 0's first: one divergent leaf test for every lane with a
    // leaf, a second only for the lanes with two.  (Postponing a lane's leaves until half of the
    // wave's unfinished lanes hold some, so that they are tested together, halved the leaf tests
    // per wave but added visits: config 5 +2 % per frame, not kept.)
    auto leaves = [&](bool l0, bool l1, const float4 &e) {
        if (l0 | l1) {
            leaf(~__float_as_int(l0 ? e.x : e.y), __float_as_int(l0 ? e.z : e.w));
            if (l0 & l1) leaf(~__float_as_int(e.y), __float_as_int(e.w));
        }
    };
    while (node >= 0) {
        bool l0, l1;
        float4 e;
        visit(l0, l1, e);
        leaves(l0, l1, e);
        if (node < 0) pop();
    }
}
