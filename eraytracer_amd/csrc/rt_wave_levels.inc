// rt_wave_levels.inc — the wavefront engine's per-level kernels (after rt_wave_walk.inc, whose inline
// walks k_reflect_shade calls): K1 k_reflect, L k_light, K1+L k_reflect_shade.

// K1: level k-1 -> level k.  q_prev/q_k and cnt_k are the levels' arrays.
// One level-(k-1) record: its reflection ray (lighting_function/6, :219-221: origin
// Hit_location, no offset), the nearest scan, and the hit appended to the source tile's
// level-k queue.  Returns the child's slot in q_k, or -1 (no hit).  Called by converged waves
// (it ballots).
// queue false (wave-uniform; the last level of the inline walks): the hit is not queued — its
// direction, distance and object go to *ch for the caller to shade — and the return value is 0
// for a hit, -1 otherwise.
struct ChildHit {
    D3 d;
    double t;
    int id;
};
template <bool LEVELS, bool ILP, int SPH = 0, bool BVH = false>
__device__ __forceinline__ int reflect_record(const Scene &S, int k, const HitRec &r, int slot, bool act, const D3 &h,
                                               const D3 &N, HitRec *__restrict__ q_k, int *__restrict__ cnt_k,
                                               uint8_t *__restrict__ levels, uint8_t *__restrict__ child_prev,
                                               bool queue = true, ChildHit *ch = nullptr) {
    const int lane = lane_id();
    const D3 d = bounce3(D3{r.dx, r.dy, r.dz}, N);
    double t = 0;
    const int id = nearest<false, ILP, SPH>(S, 0, h, d, t, act, r.obj, BVH);
    const bool hit = act && id >= 0;
    if (ch && !queue) {
        ch->d = d;
        ch->t = t;
        ch->id = id;
        return hit ? 0 : -1;
    }
    // does the level-(k-1) record have a child (read by the chain walks at levels >= 1 only)
    if (act && k > 1 && child_prev) child_prev[slot] = hit ? 1 : 0; // (null: no chain walk reads them)
    const unsigned long long m = __ballot(hit);
    if (m == 0) return -1;
    // Append to the source tile's level-k queue: one atomic per run of equal tiles in lane order
    // (in tile-ordered lists a run is a whole tile's share of the wave), ranks inside the run from
    // the ballot.  The shuffle runs on every lane: under `lane == 0 || ...` the compiler would
    // branch round it for lane 0, and a bpermute reads an inactive source lane as 0 — lane 1
    // would then miss its run head when its tile is 0 and lane 0's is not.
    const int tile = slot >> TILE_SHIFT;
    const int prev_tile = __shfl_up(tile, 1); // lane 0: its own
    const bool head = (lane == 0) | (prev_tile != tile);
    const unsigned long long hm = __ballot(head);
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1); // lanes <= this one
    const int start = 63 - __builtin_clzll(hm & upto);
    const unsigned long long after = hm & ~upto;
    const unsigned long long seg = (after ? ((1ull << __builtin_ctzll(after)) - 1) : ~0ull) & ~((1ull << start) - 1);
    const int nseg = __popcll(m & seg);
    int old = 0;
    if (head && nseg) old = atomicAdd(&cnt_k[tile], nseg);
    old = __shfl(old, start);
    const int cs = (tile << TILE_SHIFT) + old + __popcll(m & seg & ((1ull << lane) - 1));
    if (hit) {
        HitRec o;
        o.hx = h.x + d.x * t; o.hy = h.y + d.y * t; o.hz = h.z + d.z * t;
        o.dx = d.x; o.dy = d.y; o.dz = d.z;
        o.pix = r.pix; o.obj = id; o.parent = slot; o.pbits = 0;
        q_k[cs] = o;
        if (LEVELS) levels[r.pix] = (uint8_t)min(k + 1, 255); // (counts saturate at 255)
    }
    return hit ? cs : -1;
}

template <bool LEVELS, bool ILP>
__global__ __launch_bounds__(BLOCK) void k_reflect(SceneHdr hdr, const double *__restrict__ tab,
                                                   const int *__restrict__ itab, int k,
                                                   const HitRec *__restrict__ q_prev, const int *__restrict__ idx_prev,
                                                   const int *__restrict__ nhits_prev, HitRec *__restrict__ q_k,
                                                   int *__restrict__ cnt_k, uint8_t *__restrict__ levels,
                                                   uint8_t *__restrict__ child_prev, PassGeom g) {
    const Scene S{hdr, tab, itab};
    for_hits(idx_prev, nhits_prev, [&](int slot, bool act, int) {
        RT_STAT(ST_WAVES, 1);
        const HitRec r = k == 1 ? load_rec0(hdr, g, q_prev, slot) : q_prev[slot];
        const D3 h = {r.hx, r.hy, r.hz};
        const D3 N = hit_normal<0>(S, r.obj, h);
        reflect_record<LEVELS, ILP>(S, k, r, slot, act, h, N, q_k, cnt_k, levels, child_prev);
    });
}

// L: lighting_function/6 (:209-252) for every record of level k, the reflected colour taken
// as the background's +0.0 (exact wherever the reflection ray hits nothing; a record with a child
// is reshaded by k_walk with the child's colour).  The shadow answers go to the level's dense
// `lit` array for k_walk.
#ifndef RT_LIGHT_WAVES
#define RT_LIGHT_WAVES 0 // waves per SIMD k_light is compiled for (0: the compiler's choice)
#endif
#if RT_LIGHT_WAVES > 0
#define RT_LIGHT_BOUNDS __launch_bounds__(BLOCK, RT_LIGHT_WAVES)
#else
#define RT_LIGHT_BOUNDS __launch_bounds__(BLOCK)
#endif
template <int PREC, bool GENPOW, int SPH>
__global__ RT_LIGHT_BOUNDS void k_light(SceneHdr hdr, const double *__restrict__ tab,
                                                 const int *__restrict__ itab, int k, void *__restrict__ out,
                                                 const HitRec *__restrict__ q_k, const int *__restrict__ idx_k,
                                                 const int *__restrict__ nhits_k, double *__restrict__ col_k,
                                                 unsigned *__restrict__ lit_k, PassGeom g) {
    const Scene S{hdr, tab, itab};
    if (k >= 2 && !deep_dense(nhits_k - k)) return; // sparse deep levels: k_walk_deep shades them
    if (no_records_for_block(nhits_k)) return;      // before staging: sparse levels' idle blocks
    stage_tables<SPH>(S);
    for_hits(idx_k, nhits_k, [&](int slot, bool act, int) {
        const HitRec r = k == 0 ? load_rec0(hdr, g, q_k, slot) : q_k[slot];
        unsigned bits = 0;
        const D3 F = shade_terminal<GENPOW, SPH>(S, r, act, &bits);
        if (act) {
            int ls = slot; // the link re-read at the store, not kept live across the shading
            asm volatile("" : "+v"(ls));
            put_colour<PREC>(k, out, col_k, r, slot, F, g, reinterpret_cast<const int2 *>(&q_k[ls].parent));
            lit_k[slot] = bits; // a dense array: coalesced 4-byte stores, not a partial line per record
        }
    });
}

// K1+L fused (frames in flight, no side streams): one pass over level k-1 both shades its
// records as k_light(k-1) does and traces their reflections as k_reflect(k) does — the record
// is read and its normal computed once, and one launch per level is saved.  Level k-1 >= 2 is
// shaded here only when the deep levels are dense (as k_light decides); sparse deep levels
// are shaded by k_walk_deep.
// Waves per SIMD k_reflect_shade is compiled for: 5 (96 VGPRs, 14-28 of them spilled).  At 4 the
// spheres-only kernels without the BVH (RT_FUSED_WAVES_SPH) need 116-126 VGPRs and spill nothing,
// and run alone as fast (config 3) or 6 % faster (config 5's level 1) — but with frames in flight
// the frames were 1.5 % (config 3) and 4 % (config 5) slower (round 3 A/B), so 5 stays.
#ifndef RT_FUSED_WAVES
#define RT_FUSED_WAVES 5
#endif
#ifndef RT_FUSED_WAVES_SPH
#define RT_FUSED_WAVES_SPH 5
#endif
#ifndef RT_FUSED_WAVES_L2
#define RT_FUSED_WAVES_L2 RT_FUSED_WAVES_SPH // spheres-only tables in L2 (SPH = 1), no BVH: S256's level 1
#endif
// ... and for mixed scenes (SPH = 0: triangle / plane targets, shadow cones, general scans): at 5 they
// spilled 19-23 VGPRs (56-72 B of scratch per lane), at 4 none — 17-18 with the general pow (GENPOW:
// the device pow's footprint), which takes 3.  Spheres-only scenes with the general pow (GENPOW) take 3
// (at 5: 26-35 VGPRs spilled; see RT_FUSED_WAVES_GENPOW).  No benchmark configuration uses the general pow.
#ifndef RT_FUSED_WAVES_MIXED
#define RT_FUSED_WAVES_MIXED 4
#endif
#ifndef RT_FUSED_WAVES_MIXED_GENPOW
#define RT_FUSED_WAVES_MIXED_GENPOW 3
#endif
// (spheres-only with the general pow: 3 since the inline walks — at 4 the walk's second pow spilled
// 10-20 VGPRs, and level 1's kernel 4-6 before them)
#ifndef RT_FUSED_WAVES_GENPOW
#define RT_FUSED_WAVES_GENPOW 3
#endif
// The deepest level's launch with inline walks (LAST: it also shades the hits it finds, a second
// shading live beside the first) takes one wave per SIMD less (mixed scenes with the general pow two
// less): at 5 it spilled 30-33 VGPRs, the mixed general-pow ones 8-29 at 3.  Those launches are small
// (the deepest level), bound by their dependent chains, not by occupancy.
#ifndef RT_LAST_WAVES_SPH
#define RT_LAST_WAVES_SPH 4 // the LAST launch of spheres-only scenes without the general pow (5: config 3 +0.5 %,
                            // config 5 +0.4 % per frame, profiles/r06k_ab_walk_unroll_last_waves.txt)
#endif
// The LAST launch shades a record's child before the record, once, with the child's colour.
#if RT_FUSED_WAVES > 0
#define RT_FUSED_BOUNDS                                                                                            \
    __launch_bounds__(BLOCK, LAST ? (SPH == 0 && GENPOW ? 2 : SPH == 0 || GENPOW ? 3 : RT_LAST_WAVES_SPH) :    \
                             (SPH == 0 ? (GENPOW ? RT_FUSED_WAVES_MIXED_GENPOW : RT_FUSED_WAVES_MIXED)             \
                                       : GENPOW ? RT_FUSED_WAVES_GENPOW                                            \
                                       : (SPH == 1 && !BVH) ? RT_FUSED_WAVES_L2                                    \
                                                              : (SPH >= 1 && !BVH) ? RT_FUSED_WAVES_SPH            \
                                                                                   : RT_FUSED_WAVES))
#else
#define RT_FUSED_BOUNDS __launch_bounds__(BLOCK)
#endif
// BVH: this level's reflection scans traverse the sphere BVH (staged in LDS by every workgroup)
template <int PREC, bool GENPOW, int SPH, bool ILP, bool BVH, bool LAST = false>
__global__ RT_FUSED_BOUNDS void k_reflect_shade(SceneHdr hdr, const double *__restrict__ tab,
                                                const int *__restrict__ itab, int k, void *__restrict__ out,
                                                const HitRec *__restrict__ q_prev, const int *__restrict__ idx_prev,
                                                const int *__restrict__ nhits_prev, HitRec *__restrict__ q_k,
                                                int *__restrict__ cnt_k, uint8_t *__restrict__ child_prev,
                                                double *__restrict__ col_prev, PassGeom g, int iw,
                                                double2 *__restrict__ terms_staged) {
    const Scene S{hdr, tab, itab};
    if (no_records_for_block(nhits_prev)) return; // before staging: sparse levels' idle blocks
    stage_tables<SPH>(S);
    if (BVH) stage_bvh(S);
    // Per-light terms (shade's terms, walk_fold): launch_wavefront passes them for LDS-staged scenes
    // only, so the other instantiations are compiled without them (their registers as before)
    double2 *const terms = SPH == 2 ? terms_staged : nullptr;
    // Inline walks (iw != 0; ILP kernels, levels k - 1 >= 1, at most 32 lights): every level is shaded
    // by the launch that reflects it (the dense arrangement, whatever level 2's population), and a
    // shaded record without a child is final: its chain is walked here (walk_up, or walk_fold from the
    // stored terms) — no colour entry, no k_walk.  iw == 2 marks the deepest level's launch: its hits are not queued at all — each is
    // shaded at once (the background reflection, its shadow tests) and its chain walked.
    const bool shade_here = k - 1 < 2 || (ILP && iw != 0) || deep_dense(nhits_prev - (k - 1));
    const bool walk_here = ILP && iw != 0 && shade_here;
    // LAST kernels are launched for the deepest level only, with iw == 2 (launch_wavefront), so there the
    // deepest-level path holds throughout: a compile-time constant, the other paths left out of them
    constexpr bool last_here = LAST;
    RT_LINK_CHECK(!LAST || (walk_here && iw == 2), "k_reflect_shade: LAST launched at level %d with iw %d\n", k, iw);
    const size_t lslots = (size_t)(q_k - q_prev);         // slots per level
    const HitRec *q0 = q_prev - (size_t)(k - 1) * lslots; // level 0's records
    // level 1 (ILP = false: k == 1) of LDS-staged scenes reads level 0's 16-byte records two groups
    // ahead (5 more VGPRs: 91 -> 95, within 5 waves/SIMD; the L2-table build would spill), the other
    // kernels their list entries one group ahead
    auto group = [&](int slot, const HitRec &r, bool act) {
        const Scene SL = fresh_scene(S); // the header re-read per 64-record group (fresh_scene)
        const D3 h = {r.hx, r.hy, r.hz};
        const D3 N = hit_normal<SPH>(SL, r.obj, h);
        // the reflection first: a record whose reflection hits something is reshaded by a chain walk
        // (k_walk or a later launch's walk_up) with its child's colour, from the shadow bits kept
        // here in the child's record, so only the colours of the terminal records are written —
        // every pixel is written once per pass
        int cs = -1;
        ChildHit ch; // (last_here) the hit, not queued
        cs = reflect_record<false, ILP, SPH, BVH>(SL, k, r, slot, act, h, N, q_k, cnt_k, nullptr, child_prev,
                                                  !last_here, LAST ? &ch : nullptr);
        const bool child = cs >= 0;
        const int wslot = child ? cs : slot; // where the shading's result goes (one live register)
        if (shade_here) {
            const double refl = obj_row<SPH>(SL, r.obj)[8];
            if constexpr (ILP && LAST) {
                if (last_here) { // (wave-uniform)
                    // The deepest launch shades its hits where it finds them: the child first (as
                    // k_walk shades a record of the deepest level; the lanes without one take the
                    // lead's operands, valid reads), then this record once, with the child's colour as
                    // its reflection term and its shadow tests — shade()'s expression for every light
                    // is shade_bits()'s, with the same answers, so the bits are those of shading it with
                    // a +0.0 reflection and again with its shadow bits, without the second pass.
                    const bool cl = act && child;
                    const unsigned long long cm = __ballot(cl);
                    D3 cc = {0.0, 0.0, 0.0};
                    if (cm) {
                        const int cl_lead = __builtin_ctzll(cm);
                        const D3 hm = {h.x + ch.d.x * ch.t, h.y + ch.d.y * ch.t, h.z + ch.d.z * ch.t};
                        const D3 hl = {readlane_d(hm.x, cl_lead), readlane_d(hm.y, cl_lead), readlane_d(hm.z, cl_lead)};
                        const D3 dl = {readlane_d(ch.d.x, cl_lead), readlane_d(ch.d.y, cl_lead), readlane_d(ch.d.z, cl_lead)};
                        const int il = __builtin_amdgcn_readlane(ch.id, cl_lead);
                        const D3 hc = cl ? hm : hl, dc = cl ? ch.d : dl;
                        const int idc = cl ? ch.id : il;
                        const D3 c1 = shade_terminal<GENPOW, SPH>(SL, idc, dc, hc, cl);
                        if (cl) cc = c1;
                    }
                    const D3 c = shade<GENPOW, SPH, false, true>(SL, r.obj, D3{r.dx, r.dy, r.dz}, h, N, cc, refl, act);
                    if (terms) // (wave-uniform)
                        walk_fold<PREC, SPH>(SL, g, q0, lslots, k - 1, c, slot, r.parent, (unsigned)r.pbits, r.pix, act, out,
                                             terms);
                    else
                        walk_up<PREC, GENPOW, SPH>(SL, g, q0, lslots, k - 1, c, r.parent, (unsigned)r.pbits, r.pix, act, out);
                    return;
                }
            }
            unsigned bits = 0;
            // (terms: a record with a queued child leaves its per-light terms in the child's entry of level k;
            // wslot serves both the entry and the walk below — the child's slot or the record's own)
            const D3 F = shade<GENPOW, SPH>(SL, r.obj, D3{r.dx, r.dy, r.dz}, h, N, D3{0.0, 0.0, 0.0}, refl, act, &bits,
                                            terms ? terms + (size_t)(k - 1) * lslots * term_stride(SL.h.n_light) : nullptr,
                                            wslot, child);
            if constexpr (ILP) {
                if (walk_here) { // (wave-uniform; LAST kernels returned above)
                    // (the walk's inputs re-read from the kernel-argument segment instead, the
                    // header for level 0's rebuild too: SGPR spills 70 -> 44 (config 3), 48 -> 8
                    // (config 5), but config 5 +1.2 % per frame: each scalar reload's wait is also an
                    // LDS wait — profiles/r05z2_ab_inline_walk_variants.txt)
                    if (terms) // (wave-uniform)
                        walk_fold<PREC, SPH>(SL, g, q0, lslots, k - 1, F, wslot, r.parent, (unsigned)r.pbits, r.pix,
                                             act && !child, out, terms);
                    else
                        walk_up<PREC, GENPOW, SPH>(SL, g, q0, lslots, k - 1, F, r.parent, (unsigned)r.pbits, r.pix,
                                                   act && !child, out);
                    if (act && child) reinterpret_cast<unsigned *>(q_k + wslot)[15] = bits; // HitRec::pbits
                    return;
                }
            }
            if (act) {
                // the shadow bits are read back only to reshade a record with a child (k_walk): they
                // go into the child's record (a 4-byte store into the line reflect_record just wrote)
                if (!child) {
                    int ls = slot; // the link re-read at the store, not kept live across the shading
                    asm volatile("" : "+v"(ls));
                    put_colour<PREC>(k - 1, out, col_prev, r, wslot, F, g,
                                     reinterpret_cast<const int2 *>(&q_prev[ls].parent));
                }
                else reinterpret_cast<unsigned *>(q_k + wslot)[15] = bits; // HitRec::pbits
            }
        }
    };
    if (!ILP && SPH == 2) {
        for_rec0_pf(idx_prev, nhits_prev, reinterpret_cast<const Rec0 *>(q_prev), [&](int slot, const Rec0 &r0, bool act, int) {
            group(slot, rec0_to_rec(fresh_scene(S).h, g, r0), act);
        });
    } else {
        for_hits_pf(idx_prev, nhits_prev, [&](int slot, bool act, int, auto &&prefetch) {
            HitRec r;
            if (opq(k) == 1) {
                const Rec0 r0 = reinterpret_cast<const Rec0 *>(q_prev)[slot];
                prefetch();
                r = rec0_to_rec(fresh_scene(S).h, g, r0);
            } else {
                r = q_prev[slot];
                prefetch();
            }
            group(slot, r, act);
        });
    }
}
