// rt_shade.inc — one hit level's work, included inside rt_render.hip's anonymous namespace: the
// nearest-object scans (nearest, nearest_pair), the hit geometry, the shadow test (HitBall,
// shadow_cone, Target, occ_cell, lit_by) and lighting_function/6 (shade).
// Expects: rt_layout.h (namespace rtl in scope), rt_math.inc and rt_cull.inc.

#ifndef RT_MAX_GROUPS
#define RT_MAX_GROUPS 3 // reflection beams per wave (lanes grouped by the object they leave)
#endif
constexpr int MAX_GROUPS = RT_MAX_GROUPS;
constexpr int UNION_CHUNKS = 4; // reflection scans of scenes up to 256 spheres walk the union of the groups' candidates
// NB: the scene has no wave beams (beam_ok = 0, host-checked): every chunk is scanned whole and
// the beam code is compiled out (registers: the fused engine's occupancy).
template <bool PRE, bool ILP = false, int SPH = 0, bool NB = false>
__device__ __forceinline__ int nearest(const Scene &S, int org, const D3 &o, const D3 &d, double &bt, bool act,
                                       int grp = -1, bool bvh = false) {
    const SceneHdr &h = S.h;
    bt = __builtin_inf();
    int bid = 0x7fffffff;
    if (__ballot(act) == 0) return -1; // nothing to trace in this wave
    const double A4 = 4 * (d.x * d.x + d.y * d.y + d.z * d.z);
    RT_STAT(PRE ? ST_NEAR_PRE : ST_NEAR_GEN, 1);
    RT_STAT(ST_NEAR_LANES, __popcll(__ballot(act)));
    if constexpr (NB) {
        for (int chunk = 0; chunk < h.n_sph; chunk += 64)
            scan_spheres<PRE, ILP, (SPH >= 1)>(S, org, o, d, A4, chunk, chunk_all(h.n_sph, chunk), bt, bid);
        scan_tri_pl<PRE>(S, org, o, d, bt, bid);
        return (act && bid != 0x7fffffff) ? bid : -1;
    }
    if (!PRE && bvh) { // (wave-uniform) per-lane BVH traversal, then the triangles and planes
        if (h.l_bvh >= 0 && h.l_bsph >= 0)
            scan_bvh<true, true, (SPH >= 1)>(S, o, d, A4, act, bt, bid);
        else if (h.l_bvh >= 0)
            scan_bvh<true, false, (SPH >= 1)>(S, o, d, A4, act, bt, bid);
        else
            scan_bvh<false, false, (SPH >= 1)>(S, o, d, A4, act, bt, bid);
        scan_tri_pl<PRE>(S, org, o, d, bt, bid);
        return (act && bid != 0x7fffffff) ? bid : -1;
    }
    unsigned long long rem = __ballot(act);
    // staged (SPH = 2) scans keep the single-chunk form (S64: fewer registers, measured faster)
    constexpr int UCH = SPH == 2 ? 1 : UNION_CHUNKS;
    if (!PRE && h.n_sph <= 64 * UCH) {
        // The union of the groups' candidate masks (per 64-sphere chunk), walked once by the whole
        // wave (a sphere outside a lane's cone cannot be hit by that lane, so testing it is
        // harmless): each candidate is tested once however many groups share it.
        unsigned long long m[UCH] = {};
        const int nch = (h.n_sph + 63) >> 6;
        bool all = false;
        for (int g = 0; g < MAX_GROUPS && rem; ++g) {
            const int gv = __builtin_amdgcn_readlane(grp, __builtin_ctzll(rem));
            const bool sel = (g == MAX_GROUPS - 1) ? ((rem >> (threadIdx.x & 63)) & 1) != 0 : (act && grp == gv);
            rem &= ~__ballot(sel);
            const Beam32 b = make_beam32<(SPH >= 1)>(h, sel, o, d);
            RT_STAT(ST_BEAM_ON, b.on ? 1 : 0);
            if (!b.on) {
                all = true;
                break;
            }
#pragma unroll
            for (int c = 0; c < UCH; ++c)
                if (c < nch) m[c] |= cull_chunk32<SPH>(S, b, c * 64);
        }
#pragma unroll
        for (int c = 0; c < UCH; ++c)
            if (c < nch) scan_spheres<false, ILP, (SPH >= 1)>(S, org, o, d, A4, c * 64, all ? chunk_all(h.n_sph, c * 64) : m[c], bt, bid);
        rem = 0;
    }
    for (int g = 0; g < MAX_GROUPS && rem; ++g) {
        bool sel = act;
        if (!PRE) {
            const int gv = __builtin_amdgcn_readlane(grp, __builtin_ctzll(rem));
            sel = (g == MAX_GROUPS - 1) ? ((rem >> (threadIdx.x & 63)) & 1) != 0 : (act && grp == gv);
        }
        rem = PRE ? 0ull : (rem & ~__ballot(sel));
        bool on;
        if constexpr (PRE) {
            const Beam b = make_beam(h, sel, o, d, true);
            on = b.on;
            RT_STAT(ST_BEAM_ON, b.on ? 1 : 0);
            for (int chunk = 0; chunk < h.n_sph; chunk += 64) {
                const unsigned long long m = b.on ? cull_chunk<SPH>(S, b, chunk, org) : chunk_all(h.n_sph, chunk);
                scan_spheres<PRE, ILP, (SPH >= 1)>(S, org, o, d, A4, chunk, m, bt, bid);
            }
        } else {
            const Beam32 b = make_beam32<(SPH >= 1)>(h, sel, o, d);
            on = b.on;
            RT_STAT(ST_BEAM_ON, b.on ? 1 : 0);
            for (int chunk = 0; chunk < h.n_sph; chunk += 64) {
                const unsigned long long m = b.on ? cull_chunk32<SPH>(S, b, chunk) : chunk_all(h.n_sph, chunk);
                scan_spheres<PRE, ILP, (SPH >= 1)>(S, org, o, d, A4, chunk, m, bt, bid);
            }
        }
        if (!on) break; // everything was scanned
    }
    scan_tri_pl<PRE>(S, org, o, d, bt, bid);
    return (act && bid != 0x7fffffff) ? bid : -1;
}

// nearest_object_intersecting_ray/6 for two rays per lane from tabled origin `org` (primary
// rays): one beam and one candidate walk serve both, and each candidate's two tests are
// independent (instruction-level parallelism for the wave).
// FAST: the scene's spheres and the camera are within CULL_EXTENT (unit primary rays: every
// discriminant in sqrt_x's range, see there).
// pm (wave-uniform, or null): this wave's candidate masks, one per 64-sphere chunk, precomputed
// for its 8x16 pixel block (k_pmask) — then no beam is built here.
template <bool FAST>
__device__ __forceinline__ void nearest_pair(const Scene &S, int org, const D3 &o, const D3 &d0, const D3 &d1, bool a0,
                                             bool a1, int &id0, double &t0, int &id1, double &t1,
                                             const unsigned long long *pm = nullptr) {
    const SceneHdr &h = S.h;
    double bt0 = __builtin_inf(), bt1 = __builtin_inf();
    int bid0 = 0x7fffffff, bid1 = 0x7fffffff;
    id0 = id1 = -1;
    t0 = t1 = 0.0;
    if (__ballot(a0 | a1) == 0) return;
    const double A40 = 4 * (d0.x * d0.x + d0.y * d0.y + d0.z * d0.z);
    const double A41 = 4 * (d1.x * d1.x + d1.y * d1.y + d1.z * d1.z);
    Beam32 b;
    b.on = false;
    if (!pm) b = make_beam_pair32(h, a0, d0, a1, d1);
    RT_STAT(ST_NEAR_PRE, 1);
    for (int chunk = 0; chunk < h.n_sph; chunk += 64) {
        // (the table's entry is the wave's: read as a uniform value, so the candidate walk below is a
        // wave-uniform loop over scalar-loaded rows — read per lane, the compiler made it a per-lane walk
        // over gathered rows: k_primary's frames 1.4-1.7 % slower, profiles/r05al_ab_uniform_primary_masks.txt)
        unsigned long long m = pm ? uniform_u64(pm[chunk >> 6]) : b.on ? cull_chunk32_org(S, b, chunk, org) : chunk_all(h.n_sph, chunk);
        RT_STAT(ST_NEAR_PRE_CAND, __popcll(m));
        while (m) {
            const int k = chunk + __builtin_ctzll(m);
            m &= m - 1;
            const double *q = S.tab + h.o_sph_org + (org * h.n_sph + k) * SPH_ORG_W;
            const double qx = q[0], qy = q[1], qz = q[2], C = q[3];
            const int id = S.itab[h.i_sph_id + k];
            double u0, u1;
            const bool h0 = sph_t_wave<FAST>(2 * (d0.x * qx + d0.y * qy + d0.z * qz), C, A40, u0);
            const bool h1 = sph_t_wave<FAST>(2 * (d1.x * qx + d1.y * qy + d1.z * qz), C, A41, u1);
            const bool up0 = h0 & nearer(u0, id, bt0, bid0), up1 = h1 & nearer(u1, id, bt1, bid1);
            bt0 = up0 ? u0 : bt0; bid0 = up0 ? id : bid0;
            bt1 = up1 ? u1 : bt1; bid1 = up1 ? id : bid1;
        }
    }
    if (h.n_tri | h.n_pl) {
        scan_tri_pl<true>(S, org, o, d0, bt0, bid0);
        scan_tri_pl<true>(S, org, o, d1, bt1, bid1);
    }
    if (a0 && bid0 != 0x7fffffff) { id0 = bid0; t0 = bt0; }
    if (a1 && bid1 != 0x7fffffff) { id1 = bid1; t1 = bt1; }
}

// Hit point and normal of object `id` at distance t (as computed inside the reference's
// intersect functions: Intersection = O + D*t, :384-390, :443-451, :471-476).
__device__ __forceinline__ void hit_geom(const Scene &S, int id, const D3 &o, const D3 &d, double t, D3 &hit,
                                         D3 &N) {
    hit = D3{o.x + d.x * t, o.y + d.y * t, o.z + d.z * t};
    const double *r = S.tab + S.h.o_obj + id * OBJ_W;
    int kind = S.itab[S.h.i_obj_meta + id * OBJ_META_W];
    if (kind == K_SPHERE)
        N = normalize3(D3{hit.x - r[0], hit.y - r[1], hit.z - r[2]});
    else
        N = D3{r[0], r[1], r[2]};
}

// Bounding ball of the active lanes' hit points (centre = their centroid), shared by the
// shadow cones of every light at this level.  Called by the converged wave.
struct HitBall {
    double cx, cy, cz, r;
    bool on;
};
__device__ __forceinline__ HitBall make_hitball(const SceneHdr &h, bool act, const D3 &hit) {
    HitBall hb;
    hb.on = false;
    hb.cx = hb.cy = hb.cz = hb.r = 0.0;
    const unsigned long long am = __ballot(act);
    if (!h.beam_ok || am == 0) return hb;
    const double inv_n = 1.0 / (double)__popcll(am);
    hb.cx = uniform(wave_sum(act ? hit.x : 0.0) * inv_n);
    hb.cy = uniform(wave_sum(act ? hit.y : 0.0) * inv_n);
    hb.cz = uniform(wave_sum(act ? hit.z : 0.0) * inv_n);
    const double ex = hit.x - hb.cx, ey = hit.y - hb.cy, ez = hit.z - hb.cz;
    const double r2 = wave_max(act ? ex * ex + ey * ey + ez * ez : 0.0);
    const double mo = wave_max(act ? fmax(fabs(hit.x), fmax(fabs(hit.y), fabs(hit.z))) : 0.0);
    if (!(mo <= CULL_EXTENT)) return hb;
    hb.r = uniform(sqrt(r2)) * (1 + CULL_EPS) + CULL_EPS;
    hb.on = true;
    return hb;
}

// The cone of shadow-ray directions from light position Lp to the hit ball, and the largest
// shadow-ray distance t* any lane can have (a target is hit no farther than its hit point).
__device__ __forceinline__ Beam shadow_cone(const HitBall &hb, const D3 &Lp, double &tmax) {
    Beam b;
    b.on = false;
    b.ax = b.ay = b.az = b.c = b.s = b.mx = b.my = b.mz = b.ro = 0.0;
    tmax = __builtin_inf();
    if (!hb.on) return b;
    const double wx = hb.cx - Lp.x, wy = hb.cy - Lp.y, wz = hb.cz - Lp.z;
    const double D = sqrt(wx * wx + wy * wy + wz * wz);
    if (!(D > hb.r * (1 + CULL_EPS) + CULL_EPS)) return b; // light inside the ball
    const double sr = hb.r / D * (1 + CULL_EPS) + CULL_EPS;
    if (!(sr < 1.0)) return b;
    const double inv = 1.0 / D;
    b.ax = wx * inv; b.ay = wy * inv; b.az = wz * inv;
    b.s = sr;
    b.c = sqrt(1.0 - sr * sr) - CULL_EPS;
    if (!(b.c > 0.0)) return b;
    tmax = (D + hb.r) * (1 + CULL_EPS) + CULL_EPS;
    b.on = true;
    return b;
}

// shadow_factor/4 (:256-267) as the exact bounded any-hit test described at the top.
// c = canonical compact id of the hit object, sd = normalize(Hit - Light).
// The shadow target of a lane at one level: canonical id, its kind and index within its type,
// and (wave-uniform) the sphere every shading lane shares, if there is one (-1 otherwise).
struct Target {
    int c, kind, loc, skip;
};
template <int SPH = 0>
__device__ __forceinline__ Target make_target(const Scene &S, int obj, bool active) {
    // one row: kind, local, canonical id, the canonical element's local index (same kind)
    const int4 mt = obj_meta<SPH>(S, obj);
    Target T;
    T.c = mt.z;
    T.kind = mt.x;
    T.loc = mt.w;
    T.skip = -1;
    const unsigned long long am = __ballot(active);
    if (am != 0) {
        const int first = __builtin_ctzll(am);
        const int cu = __builtin_amdgcn_readlane(T.c, first);
        if (__ballot(active && T.c != cu) == 0 && __builtin_amdgcn_readlane(T.kind, first) == K_SPHERE)
            T.skip = __builtin_amdgcn_readlane(T.loc, first); // uniform target: a sphere cannot block itself
    }
    return T;
}

// Direction cell of a shadow ray sd from a light towards a target sphere (q = light - centre,
// C: the target's per-origin row): along the two world axes i, j on which a = -q/|q|, the
// cone's axis, is shortest, the signs of (sd - a) and (16 cells) whether |sd - a| exceeds half
// the cone's sine r/(2|q|) (r^2 = |q|^2 - C).  Evaluated in binary32; the host's masks are built
// for the same cells, each widened by OCC_CELL_EPS, far above this evaluation's error, so a ray
// near a cell border is covered by the mask of either side.  Only the axis choice must agree
// exactly, and it is the same binary32 comparison on both sides (rt_scene.cpp).
__device__ __forceinline__ int occ_cell(const double *q, const D3 &sd) {
    const float qx = (float)q[0], qy = (float)q[1], qz = (float)q[2];
    const float D = sqrt_f32f(qx * qx + qy * qy + qz * qz); // (a filter: cells overlap by OCC_CELL_EPS)
    const float ax = __builtin_fabsf(qx), ay = __builtin_fabsf(qy), az = __builtin_fabsf(qz);
    const int drop = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float ex = (float)sd.x * D + qx, ey = (float)sd.y * D + qy, ez = (float)sd.z * D + qz;
    const float ei = drop == 0 ? ey : ex, ej = drop == 2 ? ey : ez;
    int cell = (ei >= 0.0f ? 1 : 0) + (ej >= 0.0f ? 2 : 0);
    const float t2 = (float)(((q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - q[3]) * 0.25); // (r/2)^2
    cell += (ei * ei >= t2 ? 4 : 0) + (ej * ej >= t2 ? 8 : 0);
    return cell;
}

// SPH: the scene holds only spheres and culling is on (host-checked), so every target is a
// sphere with occluder masks: the cone and triangle/plane paths are compiled out (registers).
template <int SPH = 0, bool NB = false>
__device__ __forceinline__ bool lit_by(const Scene &S, int light, const Target &T, const D3 &sd, bool active,
                                       const HitBall &hb, const D3 &Lp) {
    const SceneHdr &h = S.h;
    const int org = 1 + light;
    const int c = T.c, kind = T.kind, loc = T.loc, skip = T.skip;
    const double A4 = 4 * (sd.x * sd.x + sd.y * sd.y + sd.z * sd.z);
    // t* of the target itself along the shadow ray
    double ts = 0;
    bool valid = false;
    int cell = 0;
    if (active) {
        if (SPH || kind == K_SPHERE) {
            const double *q = org_row<SPH>(S, org, loc);
            double B = 2 * (sd.x * q[0] + sd.y * q[1] + sd.z * q[2]);
            valid = SPH ? sph_t<true>(B, q[3], A4, ts) : sph_t(B, q[3], A4, ts);
            if (SPH != 2 && h.occ_cells > 1) cell = occ_cell(q, sd); // (staged scenes: one cell)
        } else if (kind == K_TRIANGLE) {
            const double *g = S.tab + h.o_tri + loc * TRI_W;
            const double *q = S.tab + h.o_tri_org + (org * h.n_tri + loc) * TRI_ORG_W;
            valid = tri_t(sd, D3{g[3], g[4], g[5]}, D3{g[6], g[7], g[8]}, D3{q[0], q[1], q[2]}, D3{q[3], q[4], q[5]},
                          ts);
        } else {
            const double *p = S.tab + h.o_pl + loc * PL_W;
            valid = pl_t(D3{p[0], p[1], p[2]}, sd, S.tab[h.o_pl_org + org * h.n_pl + loc], ts);
        }
    }
    bool blocked = !valid; // a target the shadow ray misses is never lit
    if (__all(blocked)) return false;
    // Candidate occluders.  Sphere targets: the union of the host-precomputed occluder masks of
    // the wave's distinct targets (no reductions).  Otherwise the cone from the light to the
    // hit ball of the wave, culled lane-parallel.
    const bool sph_targets = SPH || (h.occ_ok && __ballot(!blocked && kind != K_SPHERE) == 0);
    double tmax = __builtin_inf();
    Beam b;
    b.on = false;
    if (!SPH && !NB && !sph_targets) b = shadow_cone(hb, Lp, tmax); // shadow rays all start at the light
    RT_STAT(ST_SHADOW, 1);
    RT_STAT(ST_SHADOW_CONE_ON, (sph_targets || b.on) ? 1 : 0);
    for (int chunk = 0; chunk < h.n_sph; chunk += 64) {
        unsigned long long m;
        if (sph_targets) {
            // Every lane walks its own target's occluder mask: the trip count is the largest
            // per-lane candidate count, not the size of the union over the wave's targets
            // (which grows with every distinct target an incoherent wave holds).
            const unsigned long long *occ = occ_masks<SPH>(S, light, chunk >> 6);
            const int ncell = SPH == 2 ? 1 : h.occ_cells;
            unsigned long long mine = blocked ? 0ull : occ[(loc * ncell + cell) * h.n_chunk]; // never holds the target
            // (software-pipelined — the next candidate's row loaded while the current one is tested —
            // measured config 5 +4 %, config 3 +1.3 %: profiles/r05ai_ab_occluder_prefetch.txt)
            for (;;) {
                const bool w = !blocked && mine != 0;
                if (__ballot(w) == 0) break;
                // the row from the chunk's (wave-uniform) first row: one address operation per lane
                const int lk = w ? __builtin_ctzll(mine) : 0, k = chunk + lk;
                mine &= mine - 1;
                RT_STAT(ST_SHADOW_ITER, 1);
                const double2 *q = reinterpret_cast<const double2 *>(org_row<SPH>(S, org, chunk)) + 2 * lk;
                const double2 q01 = q[0], q23 = q[1];
                const double B = 2 * (sd.x * q01.x + sd.y * q01.y + sd.z * q23.x);
                double t;
                const bool hit = sph_t_wave<(SPH >= 1)>(B, q23.y, A4, t);
                // the candidate's list position matters only at an exact tie with the target's t*
                // (next to never): it is read for such waves alone.  The branch is taken on the bare
                // compare's ballot (one v_cmp, no mask materialised): a lane off the walk that equals
                // t* by chance only takes it, and the test inside is the exact one.
                bool blk = w & hit & (t < ts);
                if (__ballot(t == ts) != 0) blk = blk | (w & hit & (t == ts) & (sph_id<SPH>(S, k) < c));
                blocked = blocked | blk;
            }
            if (__all(blocked)) return false;
            continue;
        } else if (!SPH) {
            m = (!NB && b.on) ? cull_chunk(S, b, chunk, org, tmax) : chunk_all(h.n_sph, chunk);
            if (skip >= chunk && skip < chunk + 64) m &= ~(1ull << (skip - chunk));
        }
        RT_STAT(ST_SHADOW_CAND, __popcll(m));
        while (!SPH && m) {
            const int k = chunk + __builtin_ctzll(m);
            m &= m - 1;
            RT_STAT(ST_SHADOW_ITER, 1);
            const double *q = S.tab + h.o_sph_org + (org * h.n_sph + k) * SPH_ORG_W;
            const int id = S.itab[h.i_sph_id + k];
            const double B = 2 * (sd.x * q[0] + sd.y * q[1] + sd.z * q[2]);
            double t;
            const bool hit = sph_t_wave(B, q[3], A4, t);
            blocked = blocked | (hit & ((t < ts) | ((t == ts) & (id < c))));
            if (__all(blocked)) return false;
        }
    }
    if (SPH) return !blocked;
    for (int k = 0; k < h.n_tri; ++k) {
        if (!blocked) {
            const double *g = S.tab + h.o_tri + k * TRI_W;
            const double *q = S.tab + h.o_tri_org + (org * h.n_tri + k) * TRI_ORG_W;
            double t;
            if (tri_t(sd, D3{g[3], g[4], g[5]}, D3{g[6], g[7], g[8]}, D3{q[0], q[1], q[2]}, D3{q[3], q[4], q[5]}, t)) {
                int id = S.itab[h.i_tri_id + k];
                blocked = t < ts || (t == ts && id < c);
            }
        }
        if (__all(blocked)) return false;
    }
    for (int k = 0; k < h.n_pl; ++k) {
        if (!blocked) {
            const double *p = S.tab + h.o_pl + k * PL_W;
            double t;
            if (pl_t(D3{p[0], p[1], p[2]}, sd, S.tab[h.o_pl_org + org * h.n_pl + k], t)) {
                int id = S.itab[h.i_pl_id + k];
                blocked = t < ts || (t == ts && id < c);
            }
        }
        if (__all(blocked)) return false;
    }
    return !blocked;
}

// lighting_function/6 (:209-252) for one hit.  The reflection the reference adds for every
// light is R = col * refl (col = colour of the level below); it is formed at each use — the
// same operation on the same operands, so the same bits — which keeps fewer values live
// across the shadow scans (register pressure sets this kernel's occupancy).  The material is
// re-read per light for the same reason.
// bits (optional): bit i set where light i's shadow test passed (lights 0..31; only lanes whose
// light term is not exactly zero are tested, the others' bits are 0 and never matter).
// OPQ (col a live value, not the background's constant): col is made opaque inside the light loop,
// so col * refl is formed per light as written instead of being hoisted out of the loop into three
// more live doubles (the fused kernel spilled them).
// terms, tslot, tstore (optional; k_reflect_shade's first shading of a record whose reflection was
// queued, tstore on the lanes that have such a child): light i's {dd, sp} — everything of its term
// that does not depend on the reflected colour — goes to entry tslot (the child's slot) of `terms`,
// for the chain walk to fold the child's colour in without shading the record again (walk_fold,
// rt_wave_walk.inc).
constexpr int TERM_MAX_LIGHTS = 8; // more lights: no entries, the walk reshades (walk_up)
// double2 per entry: 64-byte entries up to 4 lights, 128-byte ones up to TERM_MAX_LIGHTS
__host__ __device__ constexpr int term_stride(int n_light) { return n_light <= 4 ? 4 : 8; }

// The fold of one light into a colour, the one copy that shade, shade_bits and walk_fold share (frames
// are bit-identical to the reference because all three do these operations on these operands in this
// order).  light_term: the light's colour term from its {dd, sp} (diffuse_term/4's and specular_term/7's
// scalars), the material colour mc, the light's diffuse colour Lc and its specular colour Sc.
__device__ __forceinline__ D3 light_term(double dd, double sp, const D3 &mc, const D3 &Lc, const D3 &Sc) {
    const D3 diff = {mc.x * dd, mc.y * dd, mc.z * dd};
    const D3 spec = {Sc.x * sp, Sc.y * sp, Sc.z * sp};
    const D3 con = {diff.x + spec.x, diff.y + spec.y, diff.z + spec.z};
    return D3{Lc.x * con.x, Lc.y * con.y, Lc.z * con.z};
}
// fold_light: F = F + (c * refl + lc * lit), the reflection added once per light (:239-247).  OPQ (c a
// live value, not the background's constant): c is made opaque, so c * refl is formed per light as
// written instead of being hoisted out of the caller's loop into three more live doubles.
template <bool OPQ>
__device__ __forceinline__ void fold_light(D3 &F, D3 c, double refl, const D3 &lc, double lit) {
    if (OPQ) asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z));
    F.x = F.x + (c.x * refl + lc.x * lit);
    F.y = F.y + (c.y * refl + lc.y * lit);
    F.z = F.z + (c.z * refl + lc.z * lit);
}
template <bool GENPOW, int SPH = 0, bool NB = false, bool OPQ = false>
__device__ __forceinline__ D3 shade(const Scene &S, int id, const D3 &d, const D3 &hit, const D3 &N, const D3 &col,
                                    double refl, bool active, unsigned *bits = nullptr, double2 *terms = nullptr,
                                    int tslot = 0, bool tstore = false) {
    const SceneHdr &h = S.h;
    if (__ballot(active) == 0) return D3{0.0, 0.0, 0.0}; // no hit to shade in this wave
    const Target T = make_target<SPH>(S, id, active);
    // the hit ball is only needed for non-sphere shadow targets (see lit_by)
    HitBall hb;
    hb.on = false;
    hb.cx = hb.cy = hb.cz = hb.r = 0.0;
    // (and for every target when the scene has no occluder masks: occ_ok = 0)
    if (!SPH && !NB && (!h.occ_ok || __ballot(active && T.kind != K_SPHERE) != 0)) hb = make_hitball(h, active, hit);
    RT_STAT(ST_SHADE, 1);
    D3 F = {0.0, 0.0, 0.0};
    for (int i = 0; i < h.n_light; ++i) {
        const Scene &SL = S; // (re-reading the header per light, fresh_scene: measured neutral)
        const double *L = SL.tab + SL.h.o_light + i * LIGHT_W;
        // the material row's address formed per light from the (opaque) object id: one live
        // register instead of a 64-bit pointer across the loop
        int idl = id;
        asm volatile("" : "+v"(idl));
        const double *m = obj_row<SPH>(S, idl);
        const D3 Lc = {L[0], L[1], L[2]}, Lp = {L[3], L[4], L[5]}, Sc = {L[6], L[7], L[8]};
        const double2 m34 = *reinterpret_cast<const double2 *>(m + 4), m67 = *reinterpret_cast<const double2 *>(m + 6);
        const D3 mc = {m[3], m34.x, m34.y};
        const double spow = m67.x, shin = m67.y;
        // diffuse_term/4 (:272-279)
        const D3 ln = normalize3(D3{Lp.x - hit.x, Lp.y - hit.y, Lp.z - hit.z}, SPH && SL.h.norm_ok);
        const double dd = max0(dot3(N, ln));
        // specular_term/7 (:285-297)
        const D3 hn = normalize3(D3{ln.x + -d.x, ln.y + -d.y, ln.z + -d.z});
        const double sp = shin * pow_libm<GENPOW>(max0(dot3(hn, N)), spow, active);
        if (terms && active && tstore) terms[(size_t)tslot * term_stride(h.n_light) + i] = double2{dd, sp};
        // A lane whose light term Lc (x) con is exactly zero gets the same bits for lit = 0 and
        // lit = 1 (the factor only multiplies signed zeros by 0 or 1): skip its shadow test.
        const D3 lc = light_term(dd, sp, mc, Lc, Sc);
        const bool need = active && !(lc.x == 0.0 && lc.y == 0.0 && lc.z == 0.0);
        // shadow ray direction normalize(Hit - Light) == -normalize(Light - Hit), bit for bit
        const bool lb = lit_by<SPH, NB>(SL, i, T, D3{-ln.x, -ln.y, -ln.z}, need, hb, Lp);
        if (bits && lb && i < 32) *bits |= 1u << i;
        fold_light<OPQ>(F, col, refl, lc, lb ? 1.0 : 0.0);
    }
    return F;
}
