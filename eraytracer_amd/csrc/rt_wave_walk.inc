// rt_wave_walk.inc — the wavefront engine's chain walks (after rt_wave_primary.inc): the inline walks
// of k_reflect_shade (walk_up, walk_fold) and the walk kernels k_walk_deep and k_walk.

// Chain-link checks of the diagnostic build (-DRT_DEBUG_LISTS, scripts/debug_lists.sh): a link
// outside its level's slots, a colour entry whose (parent, pbits) word is not its record's, or a
// parent record of another pixel prints the offending record and traps the kernel.  The product
// build keeps an out-of-range link inside the level (a wrong pixel for the parity tests to catch,
// never a wild read).
#ifdef RT_DEBUG_LISTS
#define RT_LINK_CHECK(cond, ...)                                                                                   \
    do {                                                                                                           \
        if (!(cond)) {                                                                                             \
            printf(__VA_ARGS__);                                                                                   \
            __builtin_trap();                                                                                      \
        }                                                                                                          \
    } while (0)
#else
#define RT_LINK_CHECK(cond, ...)                                                                                   \
    do {                                                                                                           \
    } while (0)
#endif

// lighting_function/6 with the shadow answers kept by k_light (bit i of `bits`).
template <bool GENPOW, int SPH = 0>
__device__ __forceinline__ D3 shade_bits(const Scene &S, int id, const D3 &d, const D3 &hit, const D3 &N, const D3 &col,
                                         double refl, unsigned bits) {
    const SceneHdr &h = S.h;
    const double *m = obj_row<SPH>(S, id);
    D3 F = {0.0, 0.0, 0.0};
    for (int i = 0; i < h.n_light; ++i) {
        const double *L = S.tab + h.o_light + i * LIGHT_W;
        const D3 Lc = {L[0], L[1], L[2]}, Lp = {L[3], L[4], L[5]}, Sc = {L[6], L[7], L[8]};
        const double2 m34 = *reinterpret_cast<const double2 *>(m + 4), m67 = *reinterpret_cast<const double2 *>(m + 6);
        const D3 mc = {m[3], m34.x, m34.y};
        const double spow = m67.x, shin = m67.y;
        // diffuse_term/4 (:272-279)
        const D3 ln = normalize3(D3{Lp.x - hit.x, Lp.y - hit.y, Lp.z - hit.z}, SPH && h.norm_ok);
        const double dd = max0(dot3(N, ln));
        // specular_term/7 (:285-297)
        const D3 hn = normalize3(D3{ln.x + -d.x, ln.y + -d.y, ln.z + -d.z});
        const double sp = shin * pow_libm<GENPOW>(max0(dot3(hn, N)), spow);
        // bits are set only where the light term is not exactly zero; elsewhere lc * 0 and
        // lc * 1 are the same signed zeros
        fold_light<true>(F, col, refl, light_term(dd, sp, mc, Lc, Sc), ((bits >> i) & 1u) ? 1.0 : 0.0);
    }
    return F;
}

// shade for a record whose reflection saw the background (+0.0): a terminal record's final colour,
// and the first colour of a record whose child a chain walk folds in later.  bits: as shade's.
template <bool GENPOW, int SPH>
__device__ __forceinline__ D3 shade_terminal(const Scene &S, int id, const D3 &d, const D3 &h, bool on,
                                             unsigned *bits = nullptr) {
    return shade<GENPOW, SPH>(S, id, d, h, hit_normal<SPH>(S, id, h), D3{0.0, 0.0, 0.0}, obj_row<SPH>(S, id)[8], on, bits);
}
template <bool GENPOW, int SPH>
__device__ __forceinline__ D3 shade_terminal(const Scene &S, const HitRec &r, bool on, unsigned *bits = nullptr) {
    return shade_terminal<GENPOW, SPH>(S, r.obj, D3{r.dx, r.dy, r.dz}, D3{r.hx, r.hy, r.hz}, on, bits);
}

// One step up a chain.  ancestor_slot: the slot at level k that `link` names — on the lanes off the
// walk (on false) the lead lane's, so every read is of a valid record (the scene reads that follow
// index by its object id; a slot no record of this frame wrote holds stale data) — kept inside the
// level's slots: a slot index by construction, and a missed writer shows up as a wrong pixel in the
// parity tests, never as a wild read (the diagnostic build traps on it, naming the caller).
__device__ __forceinline__ int ancestor_slot(const char *who, int k, int link, bool on, int lead, size_t level_slots,
                                             int pix) {
    RT_LINK_CHECK(!on || (unsigned)link < (unsigned)level_slots,
                  "%s: level %d: link %d outside the level's %d slots (pixel %d)\n", who, k, link, (int)level_slots, pix);
    const int ll = __builtin_amdgcn_readlane(link, lead);
    const int s = on ? link : ll;
    return (unsigned)s < (unsigned)level_slots ? s : 0;
}
__device__ __forceinline__ void check_ancestor_pixel(const char *who, int k, int ps, bool on, int pix, int got) {
    RT_LINK_CHECK(!on || got == pix, "%s: level %d slot %d: parent of pixel %d holds pixel %d\n", who, k, ps, pix, got);
}
// ancestor: the record at level k that `parent` names (its slot to *slot, if wanted), rebuilt from its
// Rec0 at level 0, where g is the pass's geometry (null in a walk that stops above level 0); q: level
// 0's queue; pix: the child's pixel, which the diagnostic build wants the record to hold too.
__device__ __forceinline__ HitRec ancestor(const char *who, const SceneHdr &hdr, const PassGeom *g,
                                           const HitRec *__restrict__ q, size_t level_slots, int k, int parent, bool on,
                                           int lead, int pix, int *slot = nullptr) {
    const int ps = ancestor_slot(who, k, parent, on, lead, level_slots, pix);
    const HitRec r = g && k == 0 ? load_rec0(hdr, *g, q, ps) : q[(size_t)k * level_slots + ps];
    check_ancestor_pixel(who, k, ps, on, pix, r.pix);
    if (slot) *slot = ps;
    return r;
}

// One chain walk (raytracer.erl:216-224 unwound): the final colour c of a record at
// level lv carried up its parent links to the pixel, each ancestor reshaded with its child's
// colour and its shadow answers, which sit in its child's record (pb: those of the record one
// level up; a record's pbits word is its parent's).  (Loading the next ancestor's record before the
// current one is shaded: config 5 -3 %, config 3 and small shards neutral, profiles/r06p_ab_walk_prefetch.txt)
template <int PREC, bool GENPOW, int SPH>
__device__ __forceinline__ void walk_up(const Scene &S, const PassGeom &g, const HitRec *__restrict__ q,
                                        size_t level_slots, int lv, D3 c, int parent, unsigned pb, int pix, bool on,
                                        void *__restrict__ out) {
    const unsigned long long m = __ballot(on);
    if (m == 0) return;
    const int lead = __builtin_ctzll(m);
    for (int k = lv - 1; k >= 0; --k) { // (wave-uniform: one level per step)
        const HitRec r = ancestor("walk_up", S.h, &g, q, level_slots, k, parent, on, lead, pix);
        const D3 h = {r.hx, r.hy, r.hz};
        c = shade_bits<GENPOW, SPH>(S, r.obj, D3{r.dx, r.dy, r.dz}, h, hit_normal<SPH>(S, r.obj, h), c,
                                    obj_row<SPH>(S, r.obj)[8], pb);
        parent = r.parent;
        pb = (unsigned)r.pbits;
    }
    if (on) put_pixel<PREC>(out, g, (size_t)pix, c);
}

// walk_up from stored per-light terms (LDS-staged scenes of at most TERM_MAX_LIGHTS lights): when k_reflect_shade first
// shaded an ancestor it left every light's {dd, sp} in the entry of the ancestor's queued child
// (shade's terms; entries of level k + 1 at terms + k * level_slots * stride, indexed by the child's
// slot as pbits is).  Nothing else in a light's term depends on the child's colour, so a step only
// folds the colour in — light_term and fold_light, as shade_bits calls them on the same operands, so
// the same bits — with no hit normal, normalize3 or pow, and no ray rebuilt at level 0.  A step
// reads the entry at the walk's current slot (the record at level lv is in `slot`) and the
// ancestor's last 16 bytes {pix, obj, parent, pbits} — at level 0 its Rec0.  Lanes off the walk
// follow the lead lane's slots, so every read is of a valid entry.
template <int PREC, int SPH>
__device__ __forceinline__ void walk_fold(const Scene &S, const PassGeom &g, const HitRec *__restrict__ q,
                                          size_t level_slots, int lv, D3 c, int slot, int parent, unsigned pb, int pix,
                                          bool on, void *__restrict__ out, const double2 *__restrict__ terms) {
    const unsigned long long m = __ballot(on);
    if (m == 0) return;
    const int lead = __builtin_ctzll(m);
    const SceneHdr &h = S.h;
    const int stride = term_stride(h.n_light);
    for (int k = lv - 1; k >= 0; --k) { // (wave-uniform: one level per step)
        const int ps = ancestor_slot("walk_fold", k, parent, on, lead, level_slots, pix);
        const int cs = ancestor_slot("walk_fold", k + 1, slot, on, lead, level_slots, pix);
        const double2 *e = terms + ((size_t)k * level_slots + cs) * stride;
        int4 t; // the ancestor's {pix, obj, parent, pbits}
        if (k == 0) {
            const Rec0 r0 = reinterpret_cast<const Rec0 *>(q)[ps];
            t = int4{r0.pix, r0.obj, -1, 0};
        } else {
            t = *reinterpret_cast<const int4 *>(&q[(size_t)k * level_slots + ps].pix);
        }
        check_ancestor_pixel("walk_fold", k, ps, on, pix, t.x);
        const double *mr = obj_row<SPH>(S, t.y);
        const double refl = mr[8];
        D3 F = {0.0, 0.0, 0.0};
        // four lights' terms per load (an entry holds a multiple of four): one memory wait per step
        // of the walk's dependent chain, beside the record's, instead of one per light
        for (int i0 = 0; i0 < h.n_light; i0 += 4) {
            const double2 e0 = e[i0], e1 = e[i0 + 1], e2 = e[i0 + 2], e3 = e[i0 + 3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;
                if (i >= h.n_light) break;
                const double *L = S.tab + h.o_light + i * LIGHT_W;
                const D3 Lc = {L[0], L[1], L[2]}, Sc = {L[6], L[7], L[8]};
                const double2 m34 = *reinterpret_cast<const double2 *>(mr + 4);
                const D3 mc = {mr[3], m34.x, m34.y};
                const double2 ds = j == 0 ? e0 : j == 1 ? e1 : j == 2 ? e2 : e3;
                fold_light<true>(F, c, refl, light_term(ds.x, ds.y, mc, Lc, Sc), ((pb >> i) & 1u) ? 1.0 : 0.0);
            }
        }
        c = F;
        slot = ps;
        parent = t.z;
        pb = (unsigned)t.w;
    }
    if (on) put_pixel<PREC>(out, g, (size_t)pix, c);
}

// W: the chain walk, after the reflection chain and the shading of levels 0 and 1.  One lane
// per record at level j >= 1 that has no reflection hit (a terminal record; at the deepest
// level every record): its colour — shaded here with the background's +0.0 reflection for
// j >= 2, already final from k_light for j = 1 — is carried up the parent links, every
// ancestor reshaded with its child's final colour: levels >= 2 with their shadow tests,
// levels 1 and 0 with the shadow bits k_light kept (more than 32 lights: tested again).
// Every record with a child lies on exactly one terminal record's walk, so each is shaded
// once, in the reference's order.  The waves take 64 records of one level at a time.
#ifndef RT_SHADE_WAVES
#define RT_SHADE_WAVES 0 // waves per SIMD the chain walk is compiled for (0: the compiler's choice)
#endif
// ... and for spheres-only scenes (SPH >= 1): 5 (94-95 VGPRs, no spills; round 4 A/B against the
// compiler's 4 waves: config 3 +1-2 %, config 5 -2.3 % per frame; mixed scenes spill at 5)
#ifndef RT_SHADE_WAVES_SPH
#define RT_SHADE_WAVES_SPH 5
#endif
// (with the general pow, GENPOW, spheres-only walks spilled 30-53 VGPRs at 5: they take 4)
#define RT_SHADE_BOUNDS                                                                                            \
    __launch_bounds__(BLOCK, SPH >= 1 && RT_SHADE_WAVES_SPH > 0 ? (GENPOW ? 4 : RT_SHADE_WAVES_SPH)               \
                                                                 : (RT_SHADE_WAVES > 0 ? RT_SHADE_WAVES : 1))
// Group u of the concatenated dense lists of levels [lo, hi), deepest level first: its level j
// and group g within it.  A chain walk from a deep terminal record is the longest work of the
// launch, so those waves start first and the short level-1 walks fill in behind them (in level
// order they started last and made the launch's tail).
__device__ __forceinline__ bool level_group(const int *__restrict__ nhits, int lo, int hi, int u, int &j, int &g) {
    g = u;
    for (int i = lo; i < hi; ++i) {
        j = hi - 1 - (i - lo);
        const int ng = (nhits[j] + 63) >> 6;
        if (g < ng) return true;
        g -= ng;
    }
    return false;
}


// Phase A (sparse deep levels), right after the reflection chain: every terminal record at a
// level j >= 2 is shaded and its chain carried up to level 2, each step with its shadow
// tests; the level-2 ancestor's final colour goes to col2.
template <bool GENPOW, int SPH>
__global__ RT_SHADE_BOUNDS void k_walk_deep(SceneHdr hdr, const double *__restrict__ tab,
                                            const int *__restrict__ itab, int depth, const HitRec *__restrict__ q,
                                            size_t level_slots, const int *__restrict__ idx,
                                            const int *__restrict__ nhits, const uint8_t *__restrict__ child,
                                            double *__restrict__ col2) {
    if (deep_dense(nhits)) return;
    const Scene S{hdr, tab, itab};
    const int lane = threadIdx.x & 63;
    int total = 0;
    for (int k = 2; k < depth; ++k) total += (nhits[k] + 63) >> 6;
    if ((long)blockIdx.x * (BLOCK / 64) >= (long)total) return; // idle block: leave before staging
    stage_tables<SPH>(S);
    const int nw = gridDim.x * (BLOCK / 64);
    for (int u = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); u < total; u += nw) {
        int j, g;
        level_group(nhits, 2, depth, u, j, g);
        const int p = g * 64 + lane;
        const bool in = p < nhits[j];
        int slot = idx[(size_t)j * level_slots + (in ? p : g * 64)];
        const bool term = in && (j == depth - 1 || !child[(size_t)j * level_slots + slot]);
        if (__ballot(term) == 0) continue;
        HitRec r = q[(size_t)j * level_slots + slot];
        D3 c = shade_terminal<GENPOW, SPH>(S, r, term);
        const int lead = __builtin_ctzll(__ballot(term));
        for (int k = j - 1; k >= 2; --k) { // up to level 2 (wave-uniform: one level per wave)
            r = ancestor("k_walk_deep", S.h, nullptr, q, level_slots, k, r.parent, term, lead, r.pix, &slot);
            const D3 h = {r.hx, r.hy, r.hz};
            c = shade<GENPOW, SPH, false, true>(S, r.obj, D3{r.dx, r.dy, r.dz}, h, hit_normal<SPH>(S, r.obj, h), c,
                                   obj_row<SPH>(S, r.obj)[8], term);
        }
        if (term) put_col_entry(col2, slot, c, reinterpret_cast<const int2 *>(&q[(size_t)2 * level_slots + slot].parent));
    }
}

// W: the chain walk, after the reflection chain and the shading.  Lanes: records at a level
// j >= 1 without a reflection hit (terminal; at the deepest level every record) — with
// sparse deep levels only levels 1 and 2, every level-2 record then starting from the colour
// k_walk_deep left.  Each lane's colour is final, and it is carried up the parent links,
// every ancestor reshaded with its child's final colour and the shadow bits k_light kept
// (more than 32 lights: the shadows are tested again).  Every record with a child lies on
// exactly one walk, so each is reshaded once, in the reference's order.
// Launched twice: lo = 1, hi = 2 (chains ending at level 1 — they need only the shading of
// levels 0 and 1, so this runs beside k_walk_deep) and lo = 2 (the rest).
// SRC: where an ancestor's shadow answers come from —
//   ANS_TEST  nowhere: more than 32 lights, the shadows are tested again;
//   ANS_LIT   k_light's dense `lit` array;
//   ANS_REC   (after k_reflect_shade, which comes with the merged launch only) its child's record
//             (HitRec::pbits), which the walk has just read — no per-level answer array; a terminal
//             record whose colour is already known is read only for its (parent, pbits) word, from
//             the colour entry's last word.
// DEEP: the merged launch (one after the chain, no k_walk_deep).
constexpr int ANS_TEST = 0, ANS_LIT = 1, ANS_REC = 2;
template <int PREC, bool GENPOW, int SPH, int SRC, bool DEEP>
__global__ RT_SHADE_BOUNDS void k_walk(SceneHdr hdr, const double *__restrict__ tab, const int *__restrict__ itab,
                                       int depth, void *__restrict__ out, const HitRec *__restrict__ q,
                                       size_t level_slots, const int *__restrict__ idx, const int *__restrict__ nhits,
                                       const double *__restrict__ col, const uint8_t *__restrict__ child,
                                       const unsigned *__restrict__ lit, int lo,
                                       int hi_max, PassGeom pg) {
    static_assert(SRC == ANS_TEST || SRC == ANS_LIT || SRC == ANS_REC, "k_walk: SRC is one of the three answer sources");
    static_assert(SRC != ANS_REC || DEEP, "k_walk: the answers are in the records only after k_reflect_shade, the merged launch");
    constexpr bool BITS = SRC != ANS_TEST, PAD = SRC == ANS_REC;
    const Scene S{hdr, tab, itab};
    const int lane = threadIdx.x & 63;
    const bool sparse = depth > 2 && !deep_dense(nhits);
    // DEEP (one launch after the chain, no k_walk_deep): sparse deep levels are walked here too,
    // their records shaded with their shadow tests (k_reflect_shade left them unshaded)
    const bool deep_here = DEEP && sparse;
    const int hi = min(hi_max, (sparse && !DEEP) ? 3 : depth); // levels [lo, hi)
    int total = 0;
    for (int k = lo; k < hi; ++k) total += (nhits[k] + 63) >> 6;
    if ((long)blockIdx.x * (BLOCK / 64) >= (long)total) return; // idle block: leave before staging
    stage_tables<SPH>(S);
    const int nw = gridDim.x * (BLOCK / 64);
    for (int u = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); u < total; u += nw) {
        const Scene &SL = S; // (re-reading the header per group here, fresh_scene: measured neutral)
        int j, g;
        level_group(nhits, lo, hi, u, j, g);
        const int p = g * 64 + lane;
        const bool in = p < nhits[j];
        const int slot = idx[(size_t)j * level_slots + (in ? p : g * 64)];
        const bool on = in && ((sparse && !DEEP && j == 2) || j == depth - 1 || !child[(size_t)j * level_slots + slot]);
        if (__ballot(on) == 0) continue;
        const HitRec *tr = q + (size_t)j * level_slots + slot;
        D3 c;
        int parent;      // the next record up the chain
        unsigned pb = 0; // PAD: its shadow answers
        if (j >= 2 && (deep_here || (!sparse && j == depth - 1))) {
            // the deepest level when dense, every sparse deep level with DEEP: shaded here
            // (background reflection, its shadow tests) — no k_light launch for it
            const HitRec r = *tr;
            c = shade_terminal<GENPOW, SPH>(SL, r, on);
            parent = r.parent;
            pb = (unsigned)r.pbits;
        } else {
            const double2 *cc = reinterpret_cast<const double2 *>(col + ((size_t)(j - 1) * level_slots + slot) * COL_W);
            const double2 c01 = cc[0], c2l = cc[1];
            c = D3{c01.x, c01.y, c2l.x};
            if (PAD) { // (parent, pbits) from the colour entry's last word
                const int2 pp = __builtin_bit_cast(int2, c2l.y);
                RT_LINK_CHECK(!on || (tr->parent == pp.x && tr->pbits == pp.y),
                              "k_walk: level %d slot %d: colour entry link (%d, %d), record (%d, %d)\n", j, slot, pp.x,
                              pp.y, tr->parent, tr->pbits);
                // (kept inside the level here too, as ancestor does at every step: without it the
                // general-pow kernels of spheres-only scenes spill 4-5 more VGPRs)
                parent = (unsigned)pp.x < (unsigned)level_slots ? pp.x : 0;
                pb = (unsigned)pp.y;
            } else {
                parent = tr->parent;
            }
        }
        const int lead = __builtin_ctzll(__ballot(on));
        int pix = 0; // the pixel, from the last record read
#ifdef RT_DEBUG_LISTS
        pix = on ? tr->pix : 0; // the chain's pixel: every ancestor's
#endif
        for (int k = j - 1; k >= 0; --k) { // up the chain (wave-uniform: one level per wave)
            int ps;
            const HitRec r = ancestor("k_walk", SL.h, &pg, q, level_slots, k, parent, on, lead, pix, &ps);
            const D3 h = {r.hx, r.hy, r.hz};
            const D3 N = hit_normal<SPH>(SL, r.obj, h);
            const double refl = obj_row<SPH>(SL, r.obj)[8];
            const D3 d = {r.dx, r.dy, r.dz};
            if (BITS && !(deep_here && k >= 2)) // (wave-uniform)
                c = shade_bits<GENPOW, SPH>(SL, r.obj, d, h, N, c, refl, PAD ? pb : lit[(size_t)k * level_slots + ps]);
            else
                c = shade<GENPOW, SPH, false, true>(SL, r.obj, d, h, N, c, refl, on);
            parent = r.parent;
            pb = (unsigned)r.pbits;
            pix = r.pix;
        }
        if (on) put_pixel<PREC>(out, pg, (size_t)pix, c);
    }
}
