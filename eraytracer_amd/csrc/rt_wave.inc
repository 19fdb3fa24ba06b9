// rt_wave.inc — the wavefront engine (default), in four fragments included one after the other
// inside rt_render.hip's anonymous namespace.  The reflection chains become per-level queues of hit
// records kept LOCAL TO EACH 16x16 TILE: tile b owns slots [b*256, b*256+256) of every level;
// k_items turns a level's per-tile queues into a dense list of slots, 64 records per consumer wave.
//
//   K0  k_primary        every pixel: primary ray + nearest scan; misses are written black; the
//                        tile's hits are compacted through LDS (no atomics) into level 0.
//   K1  k_reflect(k)     over level k-1: reflection ray, nearest scan; a hit becomes a level-k
//                        record in the same tile's queue, linked to its parent record.
//       k_reflect_shade(k)  (no side streams) k_reflect(k) and the shading of level k-1 in one pass;
//                        with inline walks a shaded record without a child is final and its chain
//                        is walked at once (walk_up, or walk_fold from stored per-light terms).
//   L   k_light(k)       (side streams: second, low-priority stream, as soon as level k's list
//                        exists) lighting_function/6 for every level-k record as if its reflection
//                        saw the background (+0.0 colour): final for the records without a child;
//                        the shadow answers of the others go to the level's dense `lit` array.
//   W   k_walk_deep      (side streams) sparse deep levels: terminal records at levels >= 2 shaded
//                        and carried up to level 2, every step with its shadow tests.
//       k_walk           from every terminal record up the parent links to the pixel, each ancestor
//                        reshaded with its child's final colour and its kept shadow answers.
//
// Only records with a child are shaded twice (at 4096^2 S64 about one in six at level 0); with side
// streams the bulk of the shading runs beside the latency-bound reflection chain, and every record
// is shaded by one lane with the reference's summation order (the reflection added once per light,
// raytracer.erl:239-247).  Per-level kernels are persistent grids striding over 64-record groups;
// counts live on the device — no host sync inside a frame.
//
//   rt_wave.inc          (this file) records, pass geometry, the per-level lists, pixel output
//   rt_wave_primary.inc  k_pmask, k_primary, level 0's records rebuilt
//   rt_wave_walk.inc     the chain walks: walk_up, walk_fold, k_walk_deep, k_walk
//   rt_wave_levels.inc   k_reflect, k_light, k_reflect_shade (which calls the inline walks)

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
