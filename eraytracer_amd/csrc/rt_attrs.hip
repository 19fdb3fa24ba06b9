// rt_attrs.hip — the primary-hit attribute pass (RT_ATTRIBUTES in include/rt_mi355x.h): which
// object a pixel's primary ray hits, how far away, where, with what normal and what albedo.
//
// One kernel, k_attrs, in k_primary's shape (rt_wave.inc): one 16x16 tile per 128-thread block, one
// wave per 8x16 half, two pixels per lane (rows r and r + 8), a grid-stride loop over the tiles.  It
// traces the ray rt_launch_window traces (primary_dir, rt_primary.inc) through the same nearest
// scan (nearest_pair, the wave building its own binary32 beam: no cached masks, no queues, none of
// the wavefront engine's work space), and derives the hit's geometry with the primitives the
// shading kernels use (Camera + Direction*t, hit_normal, the OBJ_W row), so every value is the one
// the renderer itself would shade.  Everything is binary64; RT_OUT_F32 rounds at the store.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_internal.h"

using namespace rtl;

namespace {

constexpr int TILE = 16;

#include "rt_math.inc"    // binary64 primitives, the primitive tests
#include "rt_cull.inc"    // scene access, wave culling, candidate scans
#include "rt_shade.inc"   // nearest-object scans
#include "rt_primary.inc" // primary rays, the jitter, hit normals

constexpr int ATTR_BLOCK = 128; // two waves: the halves of a 16x16 tile
constexpr int ATTR_GRID = 8192; // blocks at most (k_primary's grid)
// Tiles per launch: a slab with more (a column of 2^20 rows, 2^16 tiles wide) takes several.
constexpr int ATTR_MAX_TILES = 1 << 30;

// The caller's planes as the kernel takes them; a null pointer is a plane not wanted.
struct AttrPlanes {
    int *elem;
    void *t, *point, *normal, *albedo;
};

template <int PREC>
__device__ __forceinline__ void put1(void *plane, size_t pix, double v) {
    if (PREC == RT_OUT_F64)
        reinterpret_cast<double *>(plane)[pix] = v;
    else
        reinterpret_cast<float *>(plane)[pix] = (float)v;
}
template <int PREC>
__device__ __forceinline__ void put3(void *plane, size_t pix, const D3 &c) {
    if (PREC == RT_OUT_F64) {
        double *o = reinterpret_cast<double *>(plane) + pix * 3;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    } else {
        float *o = reinterpret_cast<float *>(plane) + pix * 3;
        o[0] = (float)c.x; o[1] = (float)c.y; o[2] = (float)c.z;
    }
}

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
                                                     ImageGeom im, AttrPlanes pl) {
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
            const bool hit = id >= 0;
            const int row = hit ? id : 0; // a lane without a hit goes through the geometry of object 0, unstored
            D3 h = {0.0, 0.0, 0.0}, n = h, a = h;
            int e = -1;
            if (any_hit) { // (wave-uniform)
                if (want_geom) {
                    // Intersection = Camera + Direction*t (:384-387 and its kin), the normal of that hit record
                    h = D3{cam.x + d.x * t, cam.y + d.y * t, cam.z + d.z * t};
                    n = hit_normal<0>(S, row, h);
                }
                const double *m = obj_row<0>(S, row);
                a = D3{m[3], m[4], m[5]}; // #material.colour
                e = elem_of[row];
            }
            if (!inside) return;
            const size_t pix = (size_t)(sr_base + off) * W + x;
            const D3 zero = {0.0, 0.0, 0.0};
            if (pl.elem) pl.elem[pix] = hit ? e : -1;
            if (pl.t) put1<PREC>(pl.t, pix, hit ? t : __builtin_inf());
            if (pl.point) put3<PREC>(pl.point, pix, hit ? h : zero);
            if (pl.normal) put3<PREC>(pl.normal, pix, hit ? n : zero);
            if (pl.albedo) put3<PREC>(pl.albedo, pix, hit ? a : zero);
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
    if (planes->struct_size < offsetof(rt_attr_planes, d_albedo) + sizeof(planes->d_albedo)) return RT_EBADARG;
    const rt_attr_planes pl = *planes;
    if (!pl.d_elem && !pl.d_t && !pl.d_point && !pl.d_normal && !pl.d_albedo) return RT_EBADARG;
    if (pl.precision != RT_OUT_F64 && pl.precision != RT_OUT_F32) return RT_EBADARG;
    if (spp == 0) return RT_EBADARG;
    if (spp > RT_MAX_SPP) return RT_ETOOBIG;
    if (sample >= spp) return RT_EBADARG;
    const uintptr_t esz = pl.precision == RT_OUT_F64 ? 8 : 4;
    if ((uintptr_t)pl.d_elem % 4) return RT_EBADARG;
    for (const void *f : {pl.d_t, pl.d_point, pl.d_normal, pl.d_albedo})
        if ((uintptr_t)f % esz) return RT_EBADARG;
    rt_frame f = {};
    f.img_w = width;
    f.img_h = height;
    f.win = rt_window{x0, y0, win_w, win_h};
    f.depth = 1;
    f.row_block = row_block;
    f.shard = shard;
    f.nshards = nshards;
    f.precision = pl.precision;
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
    const AttrPlanes ap = {pl.d_elem, pl.d_t, pl.d_point, pl.d_normal, pl.d_albedo};
    for (int row0 = 0; row0 < slab_rows; row0 += pass_rows) {
        const int rows = std::min(pass_rows, slab_rows - row0);
        const int ntiles = tiles_x * ((rows + TILE - 1) / TILE);
        const dim3 grid(std::min(ntiles, ATTR_GRID));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(ATTR_BLOCK), 0, st, *v.hdr, v.tab, v.itab, v.elem_of, W,
                               (int)(y0 + win_h), rb, (int)(y0 + shard * row_block), (int)nshards, slab_rows, row0, ntiles,
                               (int)spp, (int)sample, (unsigned long long)seed, im, ap);
        };
        const bool fast = v.hdr->cull_ok != 0;
        if (pl.precision == RT_OUT_F64) {
            if (fast) launch(k_attrs<RT_OUT_F64, true>);
            else launch(k_attrs<RT_OUT_F64, false>);
        } else {
            if (fast) launch(k_attrs<RT_OUT_F32, true>);
            else launch(k_attrs<RT_OUT_F32, false>);
        }
        if (hipGetLastError() != hipSuccess) return RT_EHIP;
    }
    return RT_OK;
}
