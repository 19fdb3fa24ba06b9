// rt_primary.inc — what every unit that traces primary rays shares (rt_render.hip ahead of
// rt_wave.inc, rt_attrs.hip): the image a raster is a window of, the jitter of RT_SUPERSAMPLING,
// the primary ray of a pixel and the normal of a hit.
// Expects: rt_layout.h (namespace rtl in scope), rt_math.inc and rt_cull.inc.

// The image a raster is a window of: the raster's pixel (x, row gy) is the image's (x0 + x, y0 + gy),
// the image IW x IH pixels.  The whole frame is {W, H, 0, 0}.  Only primary_dir's callers read it:
// tiles, queues, masks and stores work on the raster.
struct ImageGeom {
    int IW, IH, x0, y0;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The primary ray direction of pixel (x, image row gy) of the W x H image — image coordinates: the
// callers add the raster's origin (ImageGeom, PassGeom) — ray_through_pixel/3 (:510-511) at
// {X/Width, Y/Height} (:112), or the jittered sample position of RT_SUPERSAMPLING
// (include/rt_mi355x.h).  Called by converged waves (normalize3 ballots).
__device__ __forceinline__ D3 primary_dir(const SceneHdr &hdr, int W, int H, int spp, int sample,
                                          unsigned long long seed, int x, int gy) {
    double X, Y;
    if (opq(spp) > 1) {
        const unsigned long long pixel = (unsigned long long)gy * (unsigned)W + (unsigned)x;
        const unsigned long long r = splitmix64(seed ^ (pixel * (unsigned)spp + (unsigned)sample));
        // (24-bit values: one 32-bit conversion each, the same values as the 64-bit conversions)
        const double u = (double)(unsigned)(r >> 40) * 0x1p-24, v = (double)(unsigned)((r >> 16) & 0xFFFFFFull) * 0x1p-24;
        X = div_dim((double)x + u, W); // == / : W, H <= 2^20 (rt_launch_spp checks); x + u is exact
        Y = div_dim((double)gy + v, H);
    } else {
        X = div_dim((double)x, W);
        Y = div_dim((double)gy, H);
    }
    const double px = 0.0 + ((X - 0.5) * hdr.screen_w + hdr.sx);
    const double py = (Y - 0.5) * hdr.screen_h + hdr.sy;
    return normalize3(D3{px - hdr.cam_x, py - hdr.cam_y, hdr.dz}, hdr.prim_ok);
}

// Normal of object `id` at hit point h (as the reference's intersect functions compute it).
template <int SPH = 0>
__device__ __forceinline__ D3 hit_normal(const Scene &S, int id, const D3 &h) {
    const double *r = obj_row<SPH>(S, id);
    if (SPH || S.itab[S.h.i_obj_meta + id * OBJ_META_W] == K_SPHERE) // SPH: every object is a sphere
        return normalize3(D3{h.x - r[0], h.y - r[1], h.z - r[2]}, S.h.norm_ok); // (norm_ok: spheres only)
    return D3{r[0], r[1], r[2]};
}
