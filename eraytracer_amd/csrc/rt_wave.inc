// rt_wave.inc — the wavefront engine (default), included inside rt_render.hip's anonymous
// namespace.  The reflection chains become per-level queues of hit records kept LOCAL TO
// EACH 16x16 TILE: tile b owns slots [b*256, b*256+256) of every level; k_items turns a
// level's per-tile queues into a dense list of slots, 64 records per consumer wave.
//
//   K0  k_primary      every pixel: primary ray + nearest scan; misses are written black;
//                      the tile's hits are compacted through LDS (no atomics) into level 0.
//   K1  k_reflect(k)   over level k-1: reflection ray, nearest scan; a hit becomes a level-k
//                      record in the same tile's queue, linked to its parent record.
//   L   k_light(k)     (second, low-priority stream, as soon as level k's list exists)
//                      lighting_function/6 for every level-k record as if its reflection saw
//                      the background (+0.0 colour): final for the records without a child,
//                      provisional for the others; keeps the shadow answers in the record.
//   B   k_back(k)      after the chain, k = depth-2 .. 0: over level k+1's records, reshade
//                      each parent with its child's final colour and the kept shadow answers.
//
// Only records with a child are shaded twice (at 4096^2 S64 about one in six at level 0); the
// bulk of the shading runs beside the latency-bound reflection chain, and every record is
// shaded by one lane with the reference's summation order (the reflection added once per
// light, raytracer.erl:239-247).  Per-level kernels are persistent grids striding over
// 64-record groups; counts live on the device — no host sync inside a frame.

struct HitRec {
    double hx, hy, hz; // hit point (Intersection, as the reference's intersect computes it)
    double dx, dy, dz; // direction of the ray that hit
    int pix;           // pixel index within the pass
    int obj;           // compact object id of the hit
    int parent;        // slot of the record one level up whose reflection this is (-1 at level 0)
    int pbits;         // k_reflect_shade: the PARENT's shadow answers (bit i: light i), stored here when
                       // it shades the parent, so the chain walk gets them with the record it reads
                       // anyway; 0 otherwise (the side-stream kernels keep them in a dense array)
};
static_assert(sizeof(HitRec) == 64, "HitRec is one 64-byte record");
static_assert(offsetof(HitRec, parent) == 56 && offsetof(HitRec, pbits) == 60, "HitRec: (parent, pbits) in one 8-byte word");

// Level 0 keeps only what the primary hit cannot recompute: its pixel (pass-relative), object and
// distance.  The ray direction is a function of the pixel (primary_dir) and the hit point is
// Camera + Direction*t (:384-387 with the origin at the camera), so a consumer rebuilds the
// 64-byte record bit for bit (load_rec0) from 16 bytes: a quarter of level 0's queue traffic.
struct Rec0 {
    int pix;  // pixel index within the pass
    int obj;  // compact object id
    double t; // distance along the primary ray
};
static_assert(sizeof(Rec0) == 16, "Rec0 is one 16-byte record");

// (ImageGeom, splitmix64, primary_dir and hit_normal: rt_primary.inc, shared with rt_attrs.hip)

// Where a pass sits in the frame (what primary_dir needs besides the pixel): the raster's width W,
// its rows dealt to shards by raster row, and the image the raster is a window of.  The kernels that
// rebuild level-0 rays hold these scalars across their record loops, where every one of them is
// spilled to VGPR lanes, so the image's geometry is carried in as many registers as the raster's
// height took before there were windows (nothing downstream of k_primary reads H: make_pass_geom):
//   step  nshards * rb, yoff  y0 + shard * rb — raster row sr = qq * rb + rr is image row
//         qq * step + rr + yoff (the shard interleave, then the window's first row)
//   smp   (spp - 1) | keep << 12 | sample << 13            (spp <= RT_MAX_SPP = 4096)
//         keep: RT_PROGRESSIVE, the pass only folds its sample into acc — what the last sample of
//         a frame does differently (divide, write `out`) is never done
//   img   (IW - 1) | (IH - 1) << 20 | x0 << 40            (IW, IH <= 2^20, x0 < IW)
// unpacked where they are used (opq: a few SALU instructions there, not hoisted).
struct PassGeom {
    int W, rb, step, row0, yoff, smp;
    unsigned long long img;
    unsigned long long seed;
    // RT_SUPERSAMPLING with one write per pixel and pass: the binary64 running sum of the
    // samples (at the pass's first row, like the output), or null — the pass writes `out` as is
    double *acc;
};

static_assert(RT_MAX_SPP <= (1 << 12), "PassGeom::smp holds spp - 1 and the sample in 12 bits each");
// The `sample` argument of make_pass_geom and k_primary: the sample's index above the keep bit.
__host__ __device__ inline int sample_arg(int sample, bool keep) { return (sample << 1) | (keep ? 1 : 0); }
__host__ __device__ inline PassGeom make_pass_geom(int W, const ImageGeom &im, int rb, int shard, int nshards, int row0,
                                                   int spp, int sample, unsigned long long seed, double *acc) {
    return PassGeom{W, rb, nshards * rb, row0, im.y0 + shard * rb, (spp - 1) | (sample << 12),
                    (unsigned long long)(im.IW - 1) | ((unsigned long long)(im.IH - 1) << 20) |
                        ((unsigned long long)im.x0 << 40),
                    seed, acc};
}
__device__ __forceinline__ int geom_spp(const PassGeom &g) { return (opq(g.smp) & 0xFFF) + 1; }
__device__ __forceinline__ int geom_sample(const PassGeom &g) { return opq(g.smp) >> 13; }
__device__ __forceinline__ bool geom_keep(const PassGeom &g) { return (opq(g.smp) & 0x1000) != 0; }

constexpr int TILE_SLOTS = TILE * TILE;      // 256 records per tile and level
constexpr int TILE_SHIFT = 8;                // slot -> tile

constexpr int ITEMS_BLOCK = 256;             // tiles per k_items workgroup
#ifndef RT_STRIDE_BLOCKS
#define RT_STRIDE_BLOCKS 2048 // measured: 2048 +3 % over 4096 (configs 3 and 5), 1280 between
#endif
constexpr int STRIDE_BLOCKS = RT_STRIDE_BLOCKS; // persistent grid of the per-level kernels
// The level-1 kernel (k_reflect_shade(1), the dense, dominant one) takes a finer grid: three
// workgroups per resident slot (1,280 at 5 waves/SIMD on 256 CUs), so its tail is shorter —
// measured alone -5 % (config 3) and -9 % (config 5), frames -0.5 % and -1 %; 2,560 / 5,120 /
// 7,680 measured no better for the frames (config 3 slower at 7,680: every workgroup stages
// the scene tables in LDS)
#ifndef RT_STRIDE_BLOCKS_L1
#define RT_STRIDE_BLOCKS_L1 3840
#endif
constexpr int STRIDE_BLOCKS_L1 = RT_STRIDE_BLOCKS_L1;
#ifndef RT_STRIDE_BLOCKS_WALK
#define RT_STRIDE_BLOCKS_WALK RT_STRIDE_BLOCKS // the chain walk's (k_walk) grid
#endif
constexpr int STRIDE_BLOCKS_WALK = RT_STRIDE_BLOCKS_WALK;
// The BVH levels' grid: each of their workgroups stages the BVH nodes and sphere rows (24 KB for S256) in
// LDS before its first group, and LDS admits four of them per CU, so 1,024 are resident: a grid of that
// size stages the BVH once per resident slot (2,048 staged it twice; config 5 -1.3 % per frame, 1,536
// -0.6 %: profiles/r05an_ab_bvh_grid.txt)
#ifndef RT_STRIDE_BLOCKS_BVH
#define RT_STRIDE_BLOCKS_BVH 1024
#endif
constexpr int STRIDE_BLOCKS_BVH = RT_STRIDE_BLOCKS_BVH;
constexpr int DEEP_LIGHT_BLOCKS = 1024;      // k_light grid for levels >= 2 (4 waves per SIMD)

// Dense work list of one level: the slot (tile*256 + i) of every record in the level's
// per-tile queues, tiles in ascending order inside each 256-tile block (blocks in any
// order), so consumer waves get 64 records each however sparse the level is — a deep level
// with a few hits per tile would otherwise make one nearly empty wave per tile.
// Block-level scan in LDS, one atomic per 256 tiles for the block's offset.  Each wave then
// writes the runs of its own 64 tiles with coalesced stores.
__global__ __launch_bounds__(ITEMS_BLOCK) void k_items(const int *__restrict__ cnt, int ntiles,
                                                      int *__restrict__ idx, int *__restrict__ nhits) {
    __shared__ int s_wave[ITEMS_BLOCK / 64];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile = blockIdx.x * ITEMS_BLOCK + t;
    const int c = tile < ntiles ? cnt[tile] : 0;
    // inclusive scan inside the wave (6 shuffle steps), then over the 16 wave totals
    int v = c;
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off);
        if (lane >= off) v += u;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int w = 0; w < ITEMS_BLOCK / 64; ++w) {
            const int x = s_wave[w];
            s_wave[w] = run;
            run += x;
        }
        s_base = run ? atomicAdd(nhits, run) : 0;
    }
    __syncthreads();
    const int pos = s_base + s_wave[wave] + v - c; // where this lane's tile run starts
    // Four non-empty tiles per step, 16 lanes each (the wave's loop over its tiles is a chain of
    // scalar reads: a quarter of the steps of one tile at a time).
    unsigned long long m = __ballot(c > 0);
    const int grp = lane >> 4, sub = lane & 15;
    while (m) {
        int tl[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            tl[g] = m ? __builtin_ctzll(m) : -1;
            m &= m ? m - 1 : 0ull;
        }
        const int mine = grp == 0 ? tl[0] : grp == 1 ? tl[1] : grp == 2 ? tl[2] : tl[3];
        const int src = mine >= 0 ? mine : 0;
        const int c_src = __shfl(c, src), p_src = __shfl(pos, src); // every lane takes part
        const int ct = mine >= 0 ? c_src : 0;
        const int pt = p_src;
        const int slot0 = (blockIdx.x * ITEMS_BLOCK + wave * 64 + src) << TILE_SHIFT;
        for (int i = sub; i < ct; i += 16) idx[pt + i] = slot0 + i;
    }
}

// True when no wave of this workgroup gets a record from for_hits (workgroup-uniform): such a
// block leaves before it stages the scene tables in LDS — the persistent grid (STRIDE_BLOCKS)
// is sized for dense levels, and a sparse level would otherwise copy the tables thousands of
// times for nothing.
__device__ __forceinline__ bool no_records_for_block(const int *__restrict__ nhits) {
    return (long)blockIdx.x * BLOCK >= (long)*nhits;
}

// Each wave of the persistent grid takes the 64-record groups j, j + nwaves, ... of a dense
// list: body(slot, act, j) with act false on the lanes past the end.
template <typename F>
__device__ __forceinline__ void for_hits(const int *__restrict__ idx, const int *__restrict__ nhits, F &&body) {
    const int n = *nhits;
    const int nw = gridDim.x * (BLOCK / 64);
    const int lane = threadIdx.x & 63;
    for (int j = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); j * 64 < n; j += nw) {
        const int p = j * 64 + lane;
        const bool act = p < n;
        body(idx[act ? p : j * 64], act, j);
    }
}

// for_hits with the next group's list entry prefetched: body(slot, act, j, pf) calls pf() right
// after it has issued its own record load, so that load's wait does not also wait for the list
// load of the wave's next group (loads complete in order for s_waitcnt), which then arrives while
// the group is being shaded instead of stalling the start of the next one.
template <typename F>
__device__ __forceinline__ void for_hits_pf(const int *__restrict__ idx, const int *__restrict__ nhits, F &&body) {
    const int n = *nhits;
    const int nw = gridDim.x * (BLOCK / 64);
    const int lane = threadIdx.x & 63;
    int j = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (j * 64 >= n) return;
    int cur = idx[j * 64 + lane < n ? j * 64 + lane : j * 64];
    for (; j * 64 < n; j += nw) {
        const int p = j * 64 + lane;
        const int jn = j + nw;
        int nxt = 0;
        body(cur, p < n, j, [&]() {
            asm volatile("" ::: "memory"); // after the body's record load
            // (unconditional, at a valid index: a load under a branch makes the next wait a full vmcnt(0))
            const int q = jn * 64 + lane < n ? jn * 64 + lane : jn * 64 < n ? jn * 64 : 0;
            nxt = idx[q];
        });
        cur = nxt;
    }
}

// Level 0's records (16-byte Rec0) two groups deep: while a wave shades group j, the Rec0 of its
// group j + nw and the list entry of group j + 2 nw are in flight, so a group starts with its record
// already in registers.  body(slot, rec0, act, j).
template <typename F>
__device__ __forceinline__ void for_rec0_pf(const int *__restrict__ idx, const int *__restrict__ nhits,
                                            const Rec0 *__restrict__ q0, F &&body) {
    const int n = *nhits;
    const int nw = gridDim.x * (BLOCK / 64);
    const int lane = threadIdx.x & 63;
    int j = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (j * 64 >= n) return;
    // list index of group g's lane, clamped to a valid entry (loads issued unconditionally)
    auto at = [&](int g) { return g * 64 + lane < n ? g * 64 + lane : g * 64 < n ? g * 64 : 0; };
    int slot = idx[at(j)];
    int nslot = idx[at(j + nw)];
    Rec0 rec = q0[slot];
    for (; j * 64 < n; j += nw) {
        const int cs = slot;
        const Rec0 cr = rec;
        slot = nslot;
        rec = q0[nslot];           // group j + nw's record
        nslot = idx[at(j + 2 * nw)]; // group j + 2 nw's list entry
        body(cs, cr, j * 64 + lane < n, j);
    }
}

// Deep levels (>= 2) are shaded one of two ways, chosen on the device from the population of
// level 2 (every kernel involved reads it, so all agree):
//  * sparse (a few waves per level, S64): k_light for them exits at once; k_walk_deep shades
//    them right after the reflection chain, carrying each chain up to level 2 — no launches
//    queued behind the shading of level 1, no per-level ramp;
//  * dense (S256 depth 8): k_light shades each deep level beside the chain as it appears and
//    keeps its shadow bits; k_walk_deep exits; k_walk walks every chain from its terminal.
#ifndef RT_DEEP_DENSE_RECORDS
#define RT_DEEP_DENSE_RECORDS (512 * 1024)
#endif
constexpr int DEEP_DENSE_RECORDS = RT_DEEP_DENSE_RECORDS;
__device__ __forceinline__ bool deep_dense(const int *__restrict__ nhits) { return nhits[2] > DEEP_DENSE_RECORDS; }

__device__ __forceinline__ void store_rgb(void *out, int prec, size_t pix, const D3 &c) {
    if (prec == RT_OUT_F64) {
        double *o = reinterpret_cast<double *>(out) + pix * 3;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    } else {
        float *o = reinterpret_cast<float *>(out) + pix * 3;
        o[0] = (float)c.x; o[1] = (float)c.y; o[2] = (float)c.z;
    }
}

// lane l's value of a double (two scalar reads)
__device__ __forceinline__ double readlane_d(double v, int l) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// A pixel's final colour for this pass.  Supersampled passes that write every pixel exactly once
// (acc != null) fold the sample into the running sum right here, with k_accum's operations:
// sum = acc + c (sample 0: c), kept in acc; the last sample writes sum / spp to the output
// (a pass with the keep bit is never the last: it keeps the sum, whatever its sample).
template <int PREC>
__device__ __forceinline__ void put_pixel(void *out, const PassGeom &g, size_t pix, const D3 &c) {
    double *const acc = opq(g.acc);
    if (acc == nullptr) {
        store_rgb(out, PREC, pix, c);
        return;
    }
    double *a = acc + pix * 3;
    D3 s = c;
    const int sample = geom_sample(g), spp = geom_spp(g);
    if (sample > 0) s = D3{a[0] + c.x, a[1] + c.y, a[2] + c.z};
    if (sample < spp - 1 || geom_keep(g)) {
        a[0] = s.x; a[1] = s.y; a[2] = s.z;
    } else {
        const double n = (double)spp;
        store_rgb(out, PREC, pix, D3{s.x / n, s.y / n, s.z / n});
    }
}

// A background pixel (+0.0 in every channel: ?BACKGROUND_COLOUR, :82, or depth 0).  In the middle
// samples of a supersampled frame (with the keep bit: in every sample behind the first, sample 0
// having stored the sum's +0.0) its sum is left as it is: acc + (+0.0) == acc bit for bit, since
// acc is never -0.0 (each colour is a sum that starts from +0.0, which no rounded addition turns
// into -0.0, and so is each running sum) — the pass neither reads nor writes the pixel's 24 bytes.
template <int PREC>
__device__ __forceinline__ void put_background(void *out, const PassGeom &g, size_t pix) {
    if (opq(g.acc) != nullptr && geom_sample(g) > 0 && (geom_sample(g) < geom_spp(g) - 1 || geom_keep(g))) return;
    put_pixel<PREC>(out, g, pix, D3{0.0, 0.0, 0.0});
}

// RT_SUPERSAMPLING: fold sample `s` (a binary64 slab) into the running sum in sample order;
// the last sample divides by spp and writes the output precision.
template <int PREC>
__global__ __launch_bounds__(256) void k_accum(size_t n, const double *__restrict__ sample, double *__restrict__ acc,
                                               void *__restrict__ out, int s, int spp) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double c = sample[i];
        const double a = s == 0 ? c : acc[i] + c;
        if (s < spp - 1) {
            acc[i] = a;
        } else {
            const double m = a / (double)spp;
            if (PREC == RT_OUT_F64)
                reinterpret_cast<double *>(out)[i] = m;
            else
                reinterpret_cast<float *>(out)[i] = (float)m;
        }
    }
}

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
        const D3 diff = {mc.x * dd, mc.y * dd, mc.z * dd};
        // specular_term/7 (:285-297)
        const D3 hn = normalize3(D3{ln.x + -d.x, ln.y + -d.y, ln.z + -d.z});
        const double sp = shin * pow_libm<GENPOW>(max0(dot3(hn, N)), spow);
        const D3 spec = {Sc.x * sp, Sc.y * sp, Sc.z * sp};
        const D3 con = {diff.x + spec.x, diff.y + spec.y, diff.z + spec.z};
        const D3 lc = {Lc.x * con.x, Lc.y * con.y, Lc.z * con.z};
        // bits are set only where the light term is not exactly zero; elsewhere lc * 0 and
        // lc * 1 are the same signed zeros
        const double lit = ((bits >> i) & 1u) ? 1.0 : 0.0;
        D3 c = col; // opaque: col * refl formed per light, not hoisted (see shade)
        asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z));
        F.x = F.x + (c.x * refl + lc.x * lit);
        F.y = F.y + (c.y * refl + lc.y * lit);
        F.z = F.z + (c.z * refl + lc.z * lit);
    }
    return F;
}

// One chain walk (k_walk's loop, raytracer.erl:216-224 unwound): the final colour c of a record at
// level lv carried up its parent links to the pixel, each ancestor reshaded with its child's
// colour and its shadow answers, which sit in its child's record (pb: those of the record one
// level up; a record's pbits word is its parent's).  Lanes off the walk (on false) follow the lead
// lane's chain, so every read is of a valid record.  (Loading the next ancestor's record before the
// current one is shaded: config 5 -3 %, config 3 and small shards neutral, profiles/r06p_ab_walk_prefetch.txt)
template <int PREC, bool GENPOW, int SPH>
__device__ __forceinline__ void walk_up(const Scene &S, const PassGeom &g, const HitRec *__restrict__ q,
                                        size_t level_slots, int lv, D3 c, int parent, unsigned pb, int pix, bool on,
                                        void *__restrict__ out) {
    const unsigned long long m = __ballot(on);
    if (m == 0) return;
    const int lead = __builtin_ctzll(m);
    for (int k = lv - 1; k >= 0; --k) { // (wave-uniform: one level per step)
        RT_LINK_CHECK(!on || (unsigned)parent < (unsigned)level_slots,
                      "walk_up: level %d: parent link %d outside the level's %d slots (pixel %d, from level %d)\n", k,
                      parent, (int)level_slots, pix, lv);
        const int lp = __builtin_amdgcn_readlane(parent, lead);
        int ps = on ? parent : lp;
        ps = (unsigned)ps < (unsigned)level_slots ? ps : 0; // kept inside the level (see RT_LINK_CHECK)
        const HitRec r = k == 0 ? load_rec0(S.h, g, q, ps) : q[(size_t)k * level_slots + ps];
        RT_LINK_CHECK(!on || r.pix == pix, "walk_up: level %d slot %d: parent of pixel %d holds pixel %d\n", k, ps, pix,
                      r.pix);
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
// folds the colour in — from diff on, shade_bits's operations on the same operands in the same order,
// so the same bits — with no hit normal, normalize3 or pow, and no ray rebuilt at level 0.  A step
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
        RT_LINK_CHECK(!on || (unsigned)parent < (unsigned)level_slots,
                      "walk_fold: level %d: parent link %d outside the level's %d slots (pixel %d, from level %d)\n", k,
                      parent, (int)level_slots, pix, lv);
        RT_LINK_CHECK(!on || (unsigned)slot < (unsigned)level_slots,
                      "walk_fold: level %d: slot %d outside the level's %d slots (pixel %d, from level %d)\n", k + 1,
                      slot, (int)level_slots, pix, lv);
        const int lp = __builtin_amdgcn_readlane(parent, lead), lcs = __builtin_amdgcn_readlane(slot, lead);
        int ps = on ? parent : lp, cs = on ? slot : lcs;
        ps = (unsigned)ps < (unsigned)level_slots ? ps : 0; // kept inside the level (see RT_LINK_CHECK)
        cs = (unsigned)cs < (unsigned)level_slots ? cs : 0;
        const double2 *e = terms + ((size_t)k * level_slots + cs) * stride;
        int4 t; // the ancestor's {pix, obj, parent, pbits}
        if (k == 0) {
            const Rec0 r0 = reinterpret_cast<const Rec0 *>(q)[ps];
            t = int4{r0.pix, r0.obj, -1, 0};
        } else {
            t = *reinterpret_cast<const int4 *>(&q[(size_t)k * level_slots + ps].pix);
        }
        RT_LINK_CHECK(!on || t.x == pix, "walk_fold: level %d slot %d: parent of pixel %d holds pixel %d\n", k, ps, pix,
                      t.x);
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
                const double dd = ds.x, sp = ds.y;
                const D3 diff = {mc.x * dd, mc.y * dd, mc.z * dd};
                const D3 spec = {Sc.x * sp, Sc.y * sp, Sc.z * sp};
                const D3 con = {diff.x + spec.x, diff.y + spec.y, diff.z + spec.z};
                const D3 lc = {Lc.x * con.x, Lc.y * con.y, Lc.z * con.z};
                const double lit = ((pb >> i) & 1u) ? 1.0 : 0.0;
                D3 cc = c; // opaque: c * refl formed per light, not hoisted (see shade)
                asm volatile("" : "+v"(cc.x), "+v"(cc.y), "+v"(cc.z));
                F.x = F.x + (cc.x * refl + lc.x * lit);
                F.y = F.y + (cc.y * refl + lc.y * lit);
                F.z = F.z + (cc.z * refl + lc.z * lit);
            }
        }
        c = F;
        slot = ps;
        parent = t.z;
        pb = (unsigned)t.w;
    }
    if (on) put_pixel<PREC>(out, g, (size_t)pix, c);
}

// Where a level-k colour goes: the frame at level 0, the level's colour array otherwise — one
// 32-byte entry per slot (COL_W doubles): the colour and, in the last word, the record's
// (parent, pbits) word copied from `link` (the record's own), so the chain walk starts a terminal
// record's walk from this entry alone instead of also gathering 8 bytes of its 64-byte record.
// Every writer of an entry the walk reads this way (k_reflect_shade, k_light for the deepest
// level 1 of depth-2 frames, k_walk_deep) passes the link.
constexpr int COL_W = 4;
__device__ __forceinline__ void put_col_entry(double *col_k, int slot, const D3 &F, const int2 *link) {
    double2 *w = reinterpret_cast<double2 *>(col_k + COL_W * (size_t)slot);
    w[0] = double2{F.x, F.y};
    w[1] = double2{F.z, __builtin_bit_cast(double, *link)};
}
template <int PREC>
__device__ __forceinline__ void put_colour(int k, void *out, double *col_k, const HitRec &r, int slot, const D3 &F,
                                           const PassGeom &g, const int2 *link) {
    if (k > 0) {
        put_col_entry(col_k, slot, F, link);
    } else {
        put_pixel<PREC>(out, g, (size_t)r.pix, F);
    }
}

// L: lighting_function/6 (:209-252) for every record of level k, the reflected colour taken
// as the background's +0.0 (exact wherever the reflection ray hits nothing, which k_back
// corrects elsewhere).  The shadow answers stay in the record for k_back.
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
        const D3 h = {r.hx, r.hy, r.hz};
        const D3 N = hit_normal<SPH>(S, r.obj, h);
        const double refl = obj_row<SPH>(S, r.obj)[8];
        unsigned bits = 0;
        const D3 F = shade<GENPOW, SPH>(S, r.obj, D3{r.dx, r.dy, r.dz}, h, N, D3{0.0, 0.0, 0.0}, refl, act, &bits);
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
                        const D3 c1 = shade<GENPOW, SPH>(SL, idc, dc, hc, hit_normal<SPH>(SL, idc, hc), D3{0.0, 0.0, 0.0},
                                                         obj_row<SPH>(SL, idc)[8], cl);
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
        D3 h = {r.hx, r.hy, r.hz};
        D3 c = shade<GENPOW, SPH>(S, r.obj, D3{r.dx, r.dy, r.dz}, h, hit_normal<SPH>(S, r.obj, h), D3{0.0, 0.0, 0.0},
                                  obj_row<SPH>(S, r.obj)[8], term);
        // lanes off the walk follow the lead lane's chain (valid records: the scene reads below
        // index by their object ids; a slot no record of this frame wrote holds stale data)
        const int lead = __builtin_ctzll(__ballot(term));
        for (int k = j - 1; k >= 2; --k) { // up to level 2 (wave-uniform: one level per wave)
            const int lp = __builtin_amdgcn_readlane(r.parent, lead);
            RT_LINK_CHECK(!term || (unsigned)r.parent < (unsigned)level_slots,
                          "k_walk_deep: level %d slot %d: parent link %d outside the level's %d slots\n", k + 1, slot,
                          r.parent, (int)level_slots);
            const int cpix = r.pix;
            slot = term ? r.parent : lp;
            r = q[(size_t)k * level_slots + slot];
            RT_LINK_CHECK(!term || r.pix == cpix, "k_walk_deep: level %d slot %d: parent of pixel %d holds pixel %d\n",
                          k, slot, cpix, r.pix);
            (void)cpix;
            h = D3{r.hx, r.hy, r.hz};
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
// PAD (after k_reflect_shade): a record's shadow answers are in its child's record (HitRec::pbits),
// which the walk has just read — no per-level answer array; a terminal record whose colour is
// already known is read only for its (parent, pbits) word.
template <int PREC, bool GENPOW, int SPH, bool BITS, bool DEEP, bool PAD>
__global__ RT_SHADE_BOUNDS void k_walk(SceneHdr hdr, const double *__restrict__ tab, const int *__restrict__ itab,
                                       int depth, void *__restrict__ out, const HitRec *__restrict__ q,
                                       size_t level_slots, const int *__restrict__ idx, const int *__restrict__ nhits,
                                       const double *__restrict__ col, const uint8_t *__restrict__ child,
                                       const unsigned *__restrict__ lit, int lo,
                                       int hi_max, PassGeom pg) {
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
            const D3 h = {r.hx, r.hy, r.hz};
            c = shade<GENPOW, SPH>(SL, r.obj, D3{r.dx, r.dy, r.dz}, h, hit_normal<SPH>(SL, r.obj, h), D3{0.0, 0.0, 0.0},
                                   obj_row<SPH>(SL, r.obj)[8], on);
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
                // a slot index by construction; kept inside the level's slots regardless, so a
                // missed writer shows up as a wrong pixel in the parity tests, not a wild read
                parent = (unsigned)pp.x < (unsigned)level_slots ? pp.x : 0;
                pb = (unsigned)pp.y;
            } else {
                parent = tr->parent;
            }
        }
        // lanes off the walk follow the lead lane's chain (valid records: the scene reads below
        // index by their object ids; a slot no record of this frame wrote holds stale data)
        const int lead = __builtin_ctzll(__ballot(on));
        int pix = 0;
#ifdef RT_DEBUG_LISTS
        int dpix = on ? tr->pix : 0; // the chain's pixel: every ancestor's
#endif
        for (int k = j - 1; k >= 0; --k) { // up the chain (wave-uniform: one level per wave)
            const int lp = __builtin_amdgcn_readlane(parent, lead);
            RT_LINK_CHECK(!on || (unsigned)parent < (unsigned)level_slots,
                          "k_walk: level %d: parent link %d outside the level's %d slots (walk from level %d slot %d)\n",
                          k, parent, (int)level_slots, j, slot);
            const int ps = on ? parent : lp;
            const HitRec r = k == 0 ? load_rec0(SL.h, pg, q, ps) : q[(size_t)k * level_slots + ps];
            RT_LINK_CHECK(!on || r.pix == dpix, "k_walk: level %d slot %d: parent of pixel %d holds pixel %d (walk from level %d slot %d)\n",
                          k, ps, dpix, r.pix, j, slot);
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
