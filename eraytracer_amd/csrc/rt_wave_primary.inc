// rt_wave_primary.inc — the wavefront engine's primary pass (after rt_wave.inc): the candidate masks
// and active-tile list of a frame geometry (k_pmask), level 0's records rebuilt from 16 bytes
// (rec0_to_rec, load_rec0) and K0, k_primary.

// ---- Primary rays' candidate masks, per frame geometry (k_pmask) ------------------------------
// The primary rays of a k_primary wave (an 8x16 pixel block) depend only on the pixels, the
// camera and the frame geometry, so their beam and its cull test against every 64-sphere chunk
// (make_beam_pair32 + cull_chunk32_org: most of k_primary's non-binary64 work) are evaluated once
// per (frame geometry, scene) into a table instead of every frame.  With supersampling (JITTER)
// the beam covers the four corners of every pixel: a jittered sample's screen point lies in its
// pixel's rectangle, and the cone's section by the screen plane is an ellipse (convex), so every
// sample ray of the block lies inside the beam.
// (W, H, x, gy0, gy1: the image's, as primary_dir takes them)
__device__ __forceinline__ Beam32 make_beam_corners32(const SceneHdr &h, int W, int H, int x, int gy0, bool a0,
                                                      int gy1, bool a1) {
    Beam32 b;
    b.on = false;
    b.ax = b.ay = b.az = b.c = b.s = b.mx = b.my = b.mz = b.ro = 0.0f;
    const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
    if (!h.beam_ok || (m0 | m1) == 0) return b;
    // axis: the block's centre ray (lane 59's first pixel, else the first active one)
    const int l = ((m0 >> 59) & 1) ? 59 : (m0 ? __builtin_ctzll(m0) : __builtin_ctzll(m1));
    const bool use1 = !((m0 >> l) & 1);
    const D3 da = primary_dir(h, W, H, 1, 0, 0, x, use1 ? gy1 : gy0);
    const float rx = lane_f32((float)da.x, l), ry = lane_f32((float)da.y, l), rz = lane_f32((float)da.z, l);
    const float n2 = rx * rx + ry * ry + rz * rz;
    if (!(n2 > 1.0e-6f)) return b;
    const float inv = __builtin_amdgcn_rsqf(n2);
    const float ax = rx * inv, ay = ry * inv, az = rz * inv;
    constexpr float DIR_TOL = 1.0e-6f; // as in make_beam32
    float cmin = 2.0f;
    bool bad = false;
    for (int c = 0; c < 8; ++c) { // the 4 corners of both pixels
        const bool a = (c < 4) ? a0 : a1;
        const D3 d = primary_dir(h, W, H, 1, 0, 0, x + (c & 1), ((c < 4) ? gy0 : gy1) + ((c >> 1) & 1));
        const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
        const float dd = dx * dx + dy * dy + dz * dz;
        const float cl = ax * dx + ay * dy + az * dz;
        bad = bad || (a && !(dd > 1.0f - 0.5f * DIR_TOL && dd < 1.0f + 0.5f * DIR_TOL));
        cmin = a ? fminf(cmin, cl) : cmin;
    }
    cmin = wave_min32(cmin);
    const float c = cmin - BEAM32_EPS - 2 * DIR_TOL;
    if (__ballot(bad) != 0 || !(c > 0.0f)) return b;
    b.ax = ax; b.ay = ay; b.az = az; b.c = c;
    b.s = sqrt_f32f(fmaxf(1.0f + 4 * DIR_TOL - cmin * cmin, 0.0f)) + BEAM32_EPS + 2 * DIR_TOL; // make_beam32
    b.on = true;
    return b;
}

// The active tiles of the slab — a tile is active when either of its halves has a candidate — as a
// compact list in tile-row order, built from the empty flags by three further launches of k_pmask
// (the flags come from many workgroups: a launch boundary makes them visible, no fence or atomic):
//   phase 1  a wave per tile row counts the row's active tiles into rowoff[row + 1]
//   phase 2  one workgroup turns the counts into offsets in place: rowoff[row] = active tiles in the
//            rows before `row`, rowoff[tile_rows] = their number in the slab
//   phase 3  a wave per tile row ballot-compacts the row's active tiles into list[rowoff[row] ...):
//            x = tile column | half 0 empty << 30 | half 1 empty << 31, y = tile row
// so the active tiles of any range of tile rows (a row pass) are one contiguous range of the list,
// complete and without duplicates; k_primary's ray phase strides over it.
constexpr unsigned PE_BOTH = 0x0101u; // a tile's two flag bytes read as one 16-bit word: both halves empty
__device__ __forceinline__ void pmask_list(int phase, int tiles_x, int tile_rows, const unsigned short *pe2,
                                           int *rowoff, uint2 *list) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (phase == 2) {
        __shared__ int s_part[256];
        const int per = (tile_rows + 255) / 256, b = min(t * per, tile_rows), e = min(b + per, tile_rows);
        int s = 0;
        for (int r = b; r < e; ++r) s += rowoff[r + 1];
        s_part[t] = s;
        __syncthreads();
        if (t == 0) {
            int run = 0;
            for (int i = 0; i < 256; ++i) {
                const int x = s_part[i];
                s_part[i] = run;
                run += x;
            }
            rowoff[0] = 0;
        }
        __syncthreads();
        int run = s_part[t];
        for (int r = b; r < e; ++r) {
            run += rowoff[r + 1];
            rowoff[r + 1] = run;
        }
        return;
    }
    const unsigned long long lt = (1ull << lane) - 1;
    for (int row = blockIdx.x * 4 + wave; row < tile_rows; row += gridDim.x * 4) { // (wave-uniform)
        int n = phase == 3 ? rowoff[row] : 0;
        for (int c0 = 0; c0 < tiles_x; c0 += 64) {
            const int bx = c0 + lane;
            const unsigned f = bx < tiles_x ? (unsigned)pe2[(size_t)row * tiles_x + bx] : PE_BOTH;
            const bool act = f != PE_BOTH;
            const unsigned long long m = __ballot(act);
            if (phase == 3 && act)
                list[n + __popcll(m & lt)] = uint2{(unsigned)bx | (f & 1u) << 30 | ((f >> 8) & 1u) << 31, (unsigned)row};
            n += __popcll(m);
        }
        if (phase == 1 && lane == 0) rowoff[row + 1] = n;
    }
}

// One wave per 8x16 pixel block (k_primary's half-tiles, numbered 2 * tile + half over the whole
// slab); masks[block * n_chunk + chunk], and pe[block] = 1 when every one of them is zero.
// phase 0: the masks and flags; phases 1-3: the list of active tiles from the flags (pmask_list).
template <bool JITTER>
__global__ __launch_bounds__(256) void k_pmask(SceneHdr hdr, const double *__restrict__ tab, const int *__restrict__ itab,
                                               int W, int H, int rb, int shard, int nshards, int slab_rows, int nhalf,
                                               unsigned long long *__restrict__ pm, unsigned char *pe,
                                               ImageGeom im, int phase, int *rowoff, uint2 *list) {
    const Scene S{hdr, tab, itab};
    const int lane = threadIdx.x & 63;
    const int tiles_x = (W + TILE - 1) / TILE;
    if (phase != 0) {
        pmask_list(phase, tiles_x, (slab_rows + TILE - 1) / TILE, reinterpret_cast<const unsigned short *>(pe), rowoff, list);
        return;
    }
    for (int hw = blockIdx.x * 4 + (threadIdx.x >> 6); hw < nhalf; hw += gridDim.x * 4) { // (wave-uniform)
        const int tile = hw >> 1, half = hw & 1;
        const int by = tile / tiles_x, bx = tile - by * tiles_x;
        const int x = bx * TILE + half * 8 + (lane & 7);
        const int lr0 = by * TILE + (lane >> 3), lr1 = lr0 + 8;
        const int q0 = lr0 / rb, q1 = lr1 / rb; // slab row -> image row (the shard interleave)
        const int gy0 = (q0 * nshards + shard) * rb + (lr0 - q0 * rb), gy1 = (q1 * nshards + shard) * rb + (lr1 - q1 * rb);
        // every lane k_primary might trace (a superset: any pass's rows, any depth)
        const bool a0 = x < W && lr0 < slab_rows && gy0 < H, a1 = x < W && lr1 < slab_rows && gy1 < H;
        Beam32 b;
        if (JITTER) {
            b = make_beam_corners32(hdr, im.IW, im.IH, im.x0 + x, im.y0 + gy0, a0, im.y0 + gy1, a1);
        } else {
            const D3 d0 = primary_dir(hdr, im.IW, im.IH, 1, 0, 0, im.x0 + x, im.y0 + gy0),
                     d1 = primary_dir(hdr, im.IW, im.IH, 1, 0, 0, im.x0 + x, im.y0 + gy1);
            b = make_beam_pair32(hdr, a0, d0, a1, d1);
        }
        unsigned long long any = 0;
        for (int chunk = 0; chunk < hdr.n_sph; chunk += 64) {
            const unsigned long long m = b.on ? cull_chunk32_org(S, b, chunk, 0) : chunk_all(hdr.n_sph, chunk);
            if (lane == 0) pm[(size_t)hw * hdr.n_chunk + (chunk >> 6)] = m;
            any |= m;
        }
        if (lane == 0) pe[hw] = any == 0; // no candidate in any chunk: k_primary reads the tile's two bytes at once
    }
}

// The level-0 record in slot `slot`, rebuilt from its Rec0 (q0 = level 0's queue).  The integer
// divisions are done in binary64: a correctly rounded quotient of integers below 2^31 by a
// divisor up to 2^20 truncates to the exact integer quotient.  Converged waves only.
__device__ __forceinline__ HitRec rec0_to_rec(const SceneHdr &hdr, const PassGeom &g, const Rec0 &r0) {
    const int lr = idiv_dim(r0.pix, g.W);
    const int x = r0.pix - lr * g.W;
    const int sr = g.row0 + lr; // slab row
    const int qq = idiv_dim(sr, g.rb);
    const int iy = qq * g.step + (sr - qq * g.rb) + g.yoff; // image row
    const unsigned long long img = opq(g.img);
    const int IW = (int)((unsigned)img & 0xFFFFFu) + 1, IH = (int)((unsigned)(img >> 20) & 0xFFFFFu) + 1;
    const D3 d = primary_dir(hdr, IW, IH, geom_spp(g), geom_sample(g), g.seed, (int)(img >> 40) + x, iy);
    HitRec r;
    r.hx = hdr.cam_x + d.x * r0.t; r.hy = hdr.cam_y + d.y * r0.t; r.hz = hdr.cam_z + d.z * r0.t;
    r.dx = d.x; r.dy = d.y; r.dz = d.z;
    r.pix = r0.pix; r.obj = r0.obj; r.parent = -1; r.pbits = 0;
    return r;
}
__device__ __forceinline__ HitRec load_rec0(const SceneHdr &hdr, const PassGeom &g, const HitRec *q0, int slot) {
    return rec0_to_rec(hdr, g, reinterpret_cast<const Rec0 *>(q0)[slot]);
}

// K0: q0/cnt point at level 0 of the pass; counts of levels 1..depth-1 are zeroed here too.
// One 16x16 tile per 128-thread block: each wave covers an 8x16 half, two pixels per lane
// (rows r and r + 8), so the wave-uniform part of the scan — beam, cull, candidate walk,
// compaction — is paid once per 128 pixels.
constexpr int PRIMARY_BLOCK = 128;
constexpr int LEVEL_COUNTS = 64; // per-level record counts ahead of the dense lists: at least this many
// ints for nlev levels (launch_wavefront's list0; a multiple of 64, so the lists stay 256-byte aligned)
inline size_t level_counts(int nlev) { return (size_t)std::max(LEVEL_COUNTS, (nlev + 63) / 64 * 64); }
// Blocks of k_primary: a grid-stride loop over the tiles (RT_PRIMARY_GRID blocks at most) instead
// of one block per tile, so the dispatcher launches a few thousand blocks, not one per 16x16 tile.
#ifndef RT_PRIMARY_GRID
#define RT_PRIMARY_GRID 8192
#endif
constexpr int PRIMARY_GRID = RT_PRIMARY_GRID;
#ifndef RT_PRIMARY_WAVES
#define RT_PRIMARY_WAVES 0 // waves per SIMD k_primary is compiled for (0: the compiler's choice, 79-80 VGPRs = 6;
                           // 7 spills 3-4 VGPRs to scratch)
#endif
#if RT_PRIMARY_WAVES > 0
#define RT_PRIMARY_BOUNDS __launch_bounds__(PRIMARY_BLOCK, RT_PRIMARY_WAVES)
#else
#define RT_PRIMARY_BOUNDS __launch_bounds__(PRIMARY_BLOCK)
#endif
template <int PREC, bool LEVELS>
__global__ RT_PRIMARY_BOUNDS void k_primary(SceneHdr hdr, const double *__restrict__ tab,
                                                           const int *__restrict__ itab, int W, int Hend, int depth,
                                                           int rb, int yoff, int nshards, int rows, int row0,
                                                           void *__restrict__ out, uint8_t *__restrict__ levels,
                                                           HitRec *__restrict__ q, int *__restrict__ cnt, int ntiles,
                                                           int spp, int sample, unsigned long long seed,
                                                           double *__restrict__ acc,
                                                           const unsigned long long *__restrict__ pmask,
                                                           const unsigned short *__restrict__ pempty, int *__restrict__ nitems,
                                                           unsigned long long img, const int *__restrict__ prow,
                                                           const uint2 *__restrict__ alist) {
    // prow, alist (with pmask, or null): k_pmask's list of active tiles, prow at the pass's first tile
    // row — the pass's active tiles are alist[prow[0] .. prow[tile rows of the pass])
    // W: the raster's width; the image's geometry as PassGeom carries it (yoff, img; Hend = y0 + the
    // raster's height: the first image row past the raster), in two scalars more than a whole frame took.
    // this pass covers slab rows [row0, row0 + rows); out/levels point at slab row row0; pmask (or
    // null): k_pmask's candidate masks over the whole slab, pempty its all-zero flags per tile (both halves')
    __shared__ int s_cnt[2][PRIMARY_BLOCK / 64]; // per tile, alternating (one barrier per tile)
    const Scene S{hdr, tab, itab};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the pass's per-level record counts start at 0 (k_items adds to them; every reader of them runs
    // after this launch): no memset launch of their own
    if (blockIdx.x == 0)
        for (int i = tid; i < LEVEL_COUNTS || i < depth; i += PRIMARY_BLOCK) nitems[i] = 0; // level_counts(depth)
    const D3 cam = {hdr.cam_x, hdr.cam_y, hdr.cam_z};
    const int tiles_x = (W + TILE - 1) / TILE;
    const PassGeom geom{W, rb, nshards * rb, row0, yoff, (spp - 1) | (sample << 12), img, seed, acc};
    // Sphere-only scenes with masks: a half-tile whose candidate masks are all zero has no ray that
    // can hit anything (the walk would visit nothing, and there is nothing else to scan), so its wave
    // traces none.  Without masks (brute force, no beams) and in mixed scenes no half-tile is empty.
    const bool may_skip = pmask != nullptr && hdr.cull_ok && (hdr.n_tri | hdr.n_pl) == 0;
    // A tile with both halves empty is written with 16-byte stores when the pass writes the frame
    // itself (no running sum) and every row of it starts on a 16-byte boundary.
    constexpr int ESZ = PREC == RT_OUT_F64 ? 8 : 4;
    const size_t pitch = (size_t)W * 3 * ESZ;
    const bool wide_ok = acc == nullptr && ((reinterpret_cast<uintptr_t>(out) | pitch) & 15) == 0;
    int it = 0;
    const int tile0 = (row0 / TILE) * tiles_x; // the pass's first tile in the slab's numbering (masks, flags)
    // One shard: image row = slab row + yoff, no row block to split (wave-uniform).
    const bool single = nshards == 1;
    // One tile of the pass (tile = by * tiles_x + bx) with its halves' empty flags, by both waves of the
    // block.  LEAN (the two-phase pass below): the counts of levels >= 1 are zeroed wholesale and a tile
    // with both halves empty is never filled wide here.
    auto do_tile = [&](auto lean_c, int tile, int by, int bx, bool empty0, bool empty1) {
        constexpr bool LEAN = decltype(lean_c)::value;
        const int x = bx * TILE + wave * 8 + (lane & 7);
        // slab row -> image row (the shard interleave, then the window's first row) without a per-lane integer division:
        // the tile's first slab row is split once (wave-uniform), the lane's offset (< 16) added
        const int ly_base = row0 + by * TILE;
        const int q_base = single ? 0 : ly_base / rb, r_base = ly_base - q_base * rb;
        auto image_row = [&](int lr) {
            int rr = r_base + (lr - by * TILE), qq = q_base; // slab row row0 + lr
            while (!single && rr >= rb) { // offset < 16: at most 16 / rb + 1 steps
                rr -= rb;
                ++qq;
            }
            return qq * nshards * rb + rr + yoff;
        };
        // slab rows past the image (the last row block's tail) are never written: a
        // single-shard caller's buffer need only hold the image's rows
        auto row_inside = [&](int lr) { return lr < rows && image_row(lr) < Hend; };
        const int lr0 = by * TILE + (lane >> 3), lr1 = lr0 + 8;
        // (the wave's entry at a wave-uniform address; both waves read both halves' flags)
        const int wv = __builtin_amdgcn_readfirstlane(wave); // (a scalar: what it selects stays wave-uniform)
        const unsigned long long *pm = pmask ? pmask + ((size_t)(tile0 + tile) * 2 + wv) * hdr.n_chunk : nullptr;
        const bool mine_empty = wv ? empty1 : empty0, other_empty = wv ? empty0 : empty1;
        RT_STAT(ST_WAVES, 1);
        RT_STAT(ST_PRIM_WAVES, 1);
        if (mine_empty) {
            RT_STAT(ST_PRIM_EMPTY, 1);
            const bool fill = (!LEAN || LEVELS) && other_empty && wide_ok;
            if (fill) {
                RT_STAT(ST_PRIM_FILL, 1);
                // the tile's columns inside the image: a multiple of 16 bytes per row, as the pitch is
                const int nvec = min(TILE, W - bx * TILE) * 3 * ESZ / 16; // 12 (f32) or 24 (f64) for a full tile
                constexpr int LPR = PREC == RT_OUT_F64 ? 32 : 16;         // lanes per row: the first nvec of them store
                // (the lane's place from an opaque lane index: row offsets derived from tid were hoisted out of
                // the tile loop into VGPRs that stay live across the ray work: 85-88 VGPRs, 5 waves per SIMD)
                const int ft = wv * 64 + lane_id();
                const int v = ft & (LPR - 1);
                char *const col0 = static_cast<char *>(out) + (size_t)bx * TILE * 3 * ESZ;
                // (image rows grow with slab rows: the tile's last row inside means all of them, a scalar test)
                const bool all_rows = row_inside(by * TILE + TILE - 1);
                for (int r = ft / LPR; r < TILE; r += PRIMARY_BLOCK / LPR) {
                    const int lr = by * TILE + r;
                    if (v < nvec && (all_rows || row_inside(lr)))
                        *reinterpret_cast<uint4 *>(col0 + (size_t)lr * pitch + (size_t)v * 16) = uint4{0u, 0u, 0u, 0u};
                }
            }
            if (!fill || LEVELS) {
                const bool in0 = x < W && row_inside(lr0), in1 = x < W && row_inside(lr1);
                const size_t pix0 = (size_t)lr0 * W + x, pix1 = (size_t)lr1 * W + x;
                if (!fill) {
                    if (in0) put_background<PREC>(out, geom, pix0);
                    if (in1) put_background<PREC>(out, geom, pix1);
                }
                if (LEVELS && in0) levels[pix0] = 0;
                if (LEVELS && in1) levels[pix1] = 0;
            }
            // (an empty wave has no count to give, and needs the other's only for the tile's total:
            // the live wave of such a tile writes the counts)
            if (other_empty) {
                if (LEAN) {
                    if (tid == 0) cnt[tile] = 0;
                } else {
                    for (int l = tid; l < depth; l += PRIMARY_BLOCK) cnt[(size_t)l * ntiles + tile] = 0;
                }
            }
            return;
        }
        auto pixel = [&](int lr, bool &inside, bool &active, D3 &d) {
            const int iy = image_row(lr);
            inside = x < W && lr < rows && iy < Hend;
            active = inside && depth > 0;
            const unsigned long long im = opq(img); // (unpacked here, not held across the tile loop)
            const int IW = (int)((unsigned)im & 0xFFFFFu) + 1, IH = (int)((unsigned)(im >> 20) & 0xFFFFFu) + 1;
            // (sample is a sample_arg: its index unpacked here, not held across the tile loop)
            d = primary_dir(hdr, IW, IH, spp, opq(sample) >> 1, seed, (int)(im >> 40) + x, iy);
        };
        bool in0, in1, a0, a1;
        D3 d0, d1;
        pixel(lr0, in0, a0, d0);
        pixel(lr1, in1, a1, d1);
        int id0, id1;
        double t0, t1;
        if (hdr.cull_ok)
            nearest_pair<true>(S, 0, cam, d0, d1, a0, a1, id0, t0, id1, t1, pm);
        else
            nearest_pair<false>(S, 0, cam, d0, d1, a0, a1, id0, t0, id1, t1, pm);
        const bool h0 = id0 >= 0, h1 = id1 >= 0;
        // compact the tile's hits: wave counts in LDS, prefix over the two waves.  A tile with an
        // empty half has one wave's hits only: no exchange and no barrier (both waves see both
        // halves' masks, so they agree on which tiles meet at the barrier, and `it` alternates
        // over those tiles only).
        const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
        const int mine = __popcll(m0) + __popcll(m1);
        int before = 0, total = mine;
        if (!other_empty) {
            if (lane == 0) s_cnt[it][wave] = mine;
            __syncthreads();
            const int c0 = s_cnt[it][0], c1 = s_cnt[it][1];
            before = wave ? c0 : 0;
            total = c0 + c1;
            it ^= 1;
        }
        const unsigned long long lt = (1ull << lane) - 1;
        auto emit = [&](bool hit, bool inside, const D3 &d, int id, double t, int lr, int slot) {
            const size_t pix = (size_t)lr * W + x;
            if (hit) {
                Rec0 r;
                r.pix = (int)pix; r.obj = id; r.t = t;
                reinterpret_cast<Rec0 *>(q)[slot] = r; // the rest is rebuilt by load_rec0
            } else if (inside) {
                put_background<PREC>(out, geom, pix);
            }
            if (LEVELS && inside) levels[pix] = hit ? 1 : 0;
        };
        const int base = tile * TILE_SLOTS + before;
        emit(h0, in0, d0, id0, t0, lr0, base + __popcll(m0 & lt));
        emit(h1, in1, d1, id1, t1, lr1, base + __popcll(m0) + __popcll(m1 & lt));
        // (the tile's counts: by both waves' lanes, or by the live wave's alone; LEAN: level 0's only)
        if (LEAN) {
            if ((other_empty ? lane : tid) == 0) cnt[tile] = total;
        } else {
            for (int l = other_empty ? lane : tid; l < depth; l += other_empty ? 64 : PRIMARY_BLOCK)
                cnt[(size_t)l * ntiles + tile] = l == 0 ? total : 0;
        }
    };
    // Sphere-only scenes with masks, one sample per pixel: the pass in two phases that share nothing but
    // the kernel's arguments.  (Masks exist only at depth >= 1.)
    if (may_skip && spp == 1 && prow != nullptr) {
        const int gtid = blockIdx.x * PRIMARY_BLOCK + tid, gthreads = gridDim.x * PRIMARY_BLOCK;
        // The tile counts k_items and the appends start from: levels >= 1 are zeroed here, coalesced and
        // spread over the grid; level 0 of a tile has one writer, the phase that owns the tile, so no
        // zero races an active tile's total.
        if (depth > 1) {
            int *const z = cnt + ntiles;
            const size_t n = (size_t)(depth - 1) * ntiles;
            const size_t head = min(n, (size_t)((0 - (reinterpret_cast<uintptr_t>(z) >> 2)) & 3)); // ints up to 16 bytes
            const size_t nv = (n - head) >> 2;
            for (size_t i = gtid; i < nv; i += gthreads) reinterpret_cast<int4 *>(z + head)[i] = int4{0, 0, 0, 0};
            if ((size_t)gtid < head) z[gtid] = 0;
            if (head + nv * 4 + gtid < n) z[head + nv * 4 + gtid] = 0; // (fewer than 4 left)
        }
        const int trows = (rows + TILE - 1) / TILE; // tile rows of the pass
        // Background phase: the tiles with both halves empty are written black.
        if (!LEVELS && wide_ok) {
            // Streamed: a wave takes 64 consecutive 16-byte vectors of a tile row's raster rows and writes
            // those inside empty tiles down the tile row's rows, so runs of adjacent empty tiles are
            // written as whole lines; the lane of a tile's first vector zeroes the tile's level-0 count.
            // The units (tile row, chunk of 64 vectors) advance by adding: nothing is divided per unit.
            constexpr int VPT = TILE * 3 * ESZ / 16; // vectors per tile and row: 12 (f32) or 24 (f64)
            const int vrow = (int)(pitch >> 4), chunks = (vrow + 63) >> 6;
            const int wv = __builtin_amdgcn_readfirstlane(wave);
            const int ustep = (int)gridDim.x * (PRIMARY_BLOCK / 64), dq = ustep / chunks, dr = ustep - dq * chunks;
            const int u0 = (int)blockIdx.x * (PRIMARY_BLOCK / 64) + wv;
            int by = u0 / chunks, c = u0 - by * chunks;
            while (by < trows) {
                // the tile row's rows inside the pass and the image (image rows grow with slab rows)
                int nr;
                if (single) {
                    nr = min(TILE, min(rows, Hend - yoff - row0) - by * TILE);
                } else {
                    for (nr = 0; nr < TILE; ++nr) {
                        const int lr = by * TILE + nr, sr = row0 + lr, qq = sr / rb;
                        if (!(lr < rows && qq * nshards * rb + (sr - qq * rb) + yoff < Hend)) break;
                    }
                }
                const int v = c * 64 + lane_id();
                const int bx = v / VPT;
                const unsigned f = v < vrow ? (unsigned)pempty[tile0 + by * tiles_x + bx] : 0u;
                if (f == PE_BOTH) {
                    char *ptr = static_cast<char *>(out) + (size_t)by * TILE * pitch + (size_t)v * 16;
                    for (int r = 0; r < nr; ++r, ptr += pitch) *reinterpret_cast<uint4 *>(ptr) = uint4{0u, 0u, 0u, 0u};
                    if (v == bx * VPT) cnt[by * tiles_x + bx] = 0;
                }
                by += dq;
                c += dr;
                if (c >= chunks) {
                    c -= chunks;
                    ++by;
                }
            }
        } else {
            // Narrow (unaligned rasters, running sums, levels): the empty tiles one by one.
            for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
                const unsigned f = __builtin_amdgcn_readfirstlane((unsigned)pempty[tile0 + tile]);
                if (f != PE_BOTH) continue;
                const int by = tile / tiles_x;
                do_tile(std::true_type{}, tile, by, tile - by * tiles_x, true, true);
            }
        }
        // Ray phase: the active tiles, from k_pmask's list.
        const int a0 = prow[0], nact = prow[trows] - a0;
        for (int i = blockIdx.x; i < nact; i += gridDim.x) {
            const uint2 e = alist[a0 + i];
            const int ex = __builtin_amdgcn_readfirstlane((int)e.x), ey = __builtin_amdgcn_readfirstlane((int)e.y);
            const int bx = ex & 0x3fffffff, by = ey - row0 / TILE;
            do_tile(std::true_type{}, by * tiles_x + bx, by, bx, ((unsigned)ex >> 30 & 1u) != 0, (unsigned)ex >> 31 != 0);
        }
        return;
    }
    // Everything else (brute force, mixed and beam-free scenes, supersampled passes): every tile in turn.
    // The next tile's flags are loaded a tile ahead of their use (the two halves' in one 16-bit word: one
    // VGPR holds them across the ray work).  (A block taking two adjacent tiles in a row, so that one CU
    // writes whole 128-byte lines of a binary32 frame, measured no better: profiles/primary_tiles_ab.txt.)
    auto flags_of = [&](int t) { return may_skip && t < ntiles ? (unsigned)pempty[tile0 + t] : 0u; };
    unsigned flags = flags_of(blockIdx.x), flags_next;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, flags = flags_next) {
        flags_next = flags_of(tile + (int)gridDim.x);
        const int by = tile / tiles_x;
        const unsigned fl = __builtin_amdgcn_readfirstlane(flags);
        do_tile(std::false_type{}, tile, by, tile - by * tiles_x, (fl & 0xffu) != 0, (fl >> 8) != 0);
    }
}
