// rt_attrs.hip — the primary-hit attribute pass (RT_ATTRIBUTES in include/rt_mi355x.h): which
// object a pixel's primary ray hits, how far away, where, with what normal and what albedo.
//
// One kernel, k_attrs, in k_primary's shape (rt_wave.inc): one 16x16 tile per 128-thread block, one
// wave per 8x16 half, two pixels per lane (rows r and r + 8), a grid-stride loop over the tiles.  It
// traces the ray rt_launch_window traces (primary_dir, rt_primary.inc) through the same nearest
// scan (nearest_pair, the wave building its own binary32 beam: no cached masks, no queues, none of
// the wavefront engine's work space), and derives the hit's geometry with the primitives the
// shading kernels use (Camera + Direction*t, hit_normal, the OBJ_W row: hit_attrs, rt_planes.inc,
// shared with rt_query.hip like the stores), so every value is the one the renderer itself would
// shade.  Everything is binary64; RT_OUT_F32 rounds at the store.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"
#include "rt_pick.h"

using namespace rtl;

namespace {

constexpr int TILE = 16;

#include "rt_math.inc"    // binary64 primitives, the primitive tests
#include "rt_cull.inc"    // scene access, wave culling, candidate scans
#include "rt_shade.inc"   // nearest-object scans
#include "rt_primary.inc" // primary rays, the jitter, hit normals
#include "rt_planes.inc"  // the attribute planes: a hit's attributes, the stores

constexpr int ATTR_BLOCK = 128; // two waves: the halves of a 16x16 tile
constexpr int ATTR_GRID = 8192; // blocks at most (k_primary's grid)
// Tiles per launch: a slab with more (a column of 2^20 rows, 2^16 tiles wide) takes several.
constexpr int ATTR_MAX_TILES = 1 << 30;

// Slab rows [row0, row0 + ntiles / tiles_x * 16) of the raster (W pixels wide, slab_rows rows; its
// rows dealt to shards as k_primary's: rb, yoff = y0 + shard * rb, nshards; Hend = y0 + the raster's
// height); every plane points at slab row 0.  FAST: the scene lies within CULL_EXTENT (nearest_pair).
// The wave stays converged from the rays to the end of the geometry (normalize3 ballots); only the
// stores are predicated, by the pixel being inside the image and by the planes asked for — the
// latter wave-uniform, from the kernel's arguments.
template <int PREC, bool FAST>
__global__ __launch_bounds__(ATTR_BLOCK) void k_attrs(SceneHdr hdr, const double *__restrict__ tab,
                                                     const int *__restrict__ itab, const int *__restrict__ elem_of,
                                                     int W, int Hend, int rb, int yoff, int nshards, int slab_rows,
                                                     int row0, int ntiles, int spp, int sample, unsigned long long seed,
                                                     ImageGeom im, HitPlanes pl) {
    const Scene S{hdr, tab, itab};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const D3 cam = {hdr.cam_x, hdr.cam_y, hdr.cam_z};
    const int tiles_x = (W + TILE - 1) / TILE;
    const bool want_geom = pl.point != nullptr || pl.normal != nullptr;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int by = tile / tiles_x, bx = tile - by * tiles_x;
        const int x = bx * TILE + wave * 8 + (lane & 7);
        // slab row -> image row as in k_primary: the tile's first slab row is split once
        // (wave-uniform), the lane's offset (< 16) added
        const int sr_base = row0 + by * TILE;
        const int q_base = sr_base / rb, r_base = sr_base - q_base * rb;
        auto image_row = [&](int off) { // of slab row sr_base + off
            int rr = r_base + off, qq = q_base;
            while (rr >= rb) { // off < 16: at most 16 / rb + 1 steps
                rr -= rb;
                ++qq;
            }
            return qq * nshards * rb + rr + yoff;
        };
        const int off0 = lane >> 3, off1 = off0 + 8;
        const int iy0 = image_row(off0), iy1 = image_row(off1);
        // slab rows past the image (the last row block's tail) are never written
        const bool in0 = x < W && sr_base + off0 < slab_rows && iy0 < Hend;
        const bool in1 = x < W && sr_base + off1 < slab_rows && iy1 < Hend;
        const D3 d0 = primary_dir(hdr, im.IW, im.IH, spp, sample, seed, im.x0 + x, iy0);
        const D3 d1 = primary_dir(hdr, im.IW, im.IH, spp, sample, seed, im.x0 + x, iy1);
        int id0, id1;
        double t0, t1;
        nearest_pair<FAST>(S, 0, cam, d0, d1, in0, in1, id0, t0, id1, t1, nullptr);
        const bool any_hit = __ballot(id0 >= 0 || id1 >= 0) != 0; // (then the scene has an object: row 0 exists)
        auto emit = [&](bool inside, const D3 &d, int id, double t, int off) {
            const HitAttrs a = hit_attrs(S, elem_of, cam, d, id, t, any_hit, want_geom);
            if (inside) put_hit<PREC>(pl, (size_t)(sr_base + off) * W + x, id, t, a);
        };
        emit(in0, d0, id0, t0, off0);
        emit(in1, d1, id1, t1, off1);
    }
}

} // namespace

extern "C" int rt_launch_attrs(rt_prepared *p, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t win_w,
                               uint32_t win_h, uint32_t row_block, uint32_t shard, uint32_t nshards, uint32_t spp,
                               uint64_t seed, uint32_t sample, const rt_attr_planes *planes, void *stream) {
    if (!p || !planes) return RT_EBADARG;
    HitPlanes hp;
    int prec;
    const int planes_ok = rt_hit_planes(planes, &hp, &prec);
    if (prec < 0) return planes_ok;
    if (spp == 0) return RT_EBADARG;
    if (spp > RT_MAX_SPP) return RT_ETOOBIG; // (reported before a misaligned plane)
    if (sample >= spp) return RT_EBADARG;
    if (planes_ok != RT_OK) return planes_ok;
    rt_frame f = {};
    f.img_w = width;
    f.img_h = height;
    f.win = rt_window{x0, y0, win_w, win_h};
    f.depth = 1;
    f.row_block = row_block;
    f.shard = shard;
    f.nshards = nshards;
    f.precision = prec;
    f.order = RT_ORDER_EXACT;
    f.spp = spp;
    f.seed = seed;
    const int ok = rt_frame_check(f);
    if (ok != RT_OK) return ok;

    const rt_scene_view v = rt_prepared_scene(p);
    DevGuard g(v.device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int W = (int)win_w, rb = (int)row_block, slab_rows = (int)f.slab_rows();
    const int tiles_x = (W + TILE - 1) / TILE;
    // rows per launch: whole tile rows, ATTR_MAX_TILES tiles at most
    const int pass_rows = (int)std::min<long long>(slab_rows, (long long)std::max(1, ATTR_MAX_TILES / tiles_x) * TILE);
    const ImageGeom im = {(int)width, (int)height, (int)x0, (int)y0};
    for (int row0 = 0; row0 < slab_rows; row0 += pass_rows) {
        const int rows = std::min(pass_rows, slab_rows - row0);
        const int ntiles = tiles_x * ((rows + TILE - 1) / TILE);
        const dim3 grid(std::min(ntiles, ATTR_GRID));
        with_int<RT_OUT_F64, RT_OUT_F32>(prec, [&](auto pc) {
            with_bool(v.hdr->cull_ok != 0, [&](auto fast) {
                hipLaunchKernelGGL((k_attrs<decltype(pc)::value, decltype(fast)::value>), grid, dim3(ATTR_BLOCK), 0, st,
                                   *v.hdr, v.tab, v.itab, v.elem_of, W, (int)(y0 + win_h), rb,
                                   (int)(y0 + shard * row_block), (int)nshards, slab_rows, row0, ntiles, (int)spp,
                                   (int)sample, (unsigned long long)seed, im, hp);
            });
        });
        if (hipGetLastError() != hipSuccess) return RT_EHIP;
    }
    return RT_OK;
}
