// rt_fused.inc — the fused engine, included inside rt_render.hip's anonymous namespace: k_render,
// one work-item per pixel running the whole reflection chain (launched by launch_t).
// Expects: BLOCK, TILE and RT_WAVES_PER_SIMD (rt_render.hip), rt_math.inc, rt_cull.inc and
// rt_shade.inc.

// The beam-free build (NB) needs fewer registers: its own occupancy target.
#ifndef RT_FUSED_NB_WAVES
#define RT_FUSED_NB_WAVES 5
#endif
template <int ORDER, int PREC, bool LEVELS, bool GENPOW, bool NB>
__global__ __launch_bounds__(256, NB ? RT_FUSED_NB_WAVES : RT_WAVES_PER_SIMD) void k_render(SceneHdr hdr, const double *__restrict__ tab,
                                                  const int *__restrict__ itab, int W, int H, int depth, int rb,
                                                  int shard, int nshards, int row0, int row_end, void *__restrict__ out,
                                                  uint8_t *__restrict__ levels, int levels_hit, int IW, int IH, int x0,
                                                  int y0) {
    // this launch covers slab rows [row0, row_end); out / levels point at slab row 0.  W x H is the
    // raster, a window of the IW x IH image at (x0, y0): only the primary ray reads the image's geometry
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Scene S{hdr, tab, itab};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = blockIdx.x * TILE + (wave & 1) * 8 + (lane & 7);
    const int ly = row0 + blockIdx.y * TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = x < W && ly < row_end;
    // slab row -> image row: the tile's first row split once (wave-uniform), the offset (< 16) added
    const int ly_base = row0 + blockIdx.y * TILE, q_base = ly_base / rb;
    int rr = ly_base - q_base * rb + (ly - ly_base), qq = q_base;
    while (rr >= rb) {
        rr -= rb;
        ++qq;
    }
    const int gy = (qq * nshards + shard) * rb + rr;
    const bool active = inside && gy < H;
    RT_STAT(ST_WAVES, 1);

    // primary ray: ray_through_pixel/3 (:510-511) at {X/Width, Y/Height} (:112)
    const double X = div_n((double)(x0 + x), (double)IW), Y = div_n((double)(y0 + gy), (double)IH); // == / (IW, IH <= 2^20)
    const double px = 0.0 + ((X - 0.5) * hdr.screen_w + hdr.sx);
    const double py = (Y - 0.5) * hdr.screen_h + hdr.sy;
    const D3 cam = {hdr.cam_x, hdr.cam_y, hdr.cam_z};
    const D3 d0 = normalize3(D3{px - hdr.cam_x, py - hdr.cam_y, hdr.dz}, hdr.prim_ok);

    D3 col = {0.0, 0.0, 0.0};
    int nlev = 0;
    if (ORDER == RT_ORDER_EXACT) {
        double *st = reinterpret_cast<double *>(smem);               // [depth][BLOCK] distances
        int *so = reinterpret_cast<int *>(smem + (size_t)depth * BLOCK * 8); // [depth][BLOCK] object ids
        // [3][BLOCK] the primary direction, read back by each level's replay instead of being kept
        // live (spilled) across the chain
        double *sd0 = reinterpret_cast<double *>(smem + (size_t)depth * BLOCK * 12);
        sd0[tid] = d0.x;
        sd0[BLOCK + tid] = d0.y;
        sd0[2 * BLOCK + tid] = d0.z;
        // forward: the reflection chain's nearest-object scans
        D3 o = cam, d = d0;
        bool alive = active;
        int prev = -1;
        for (int k = 0; k < depth; ++k) {
            const Scene SL = fresh_scene(S); // the header re-read per level (fresh_scene)
            double t = 0;
            int id = -1;
            id = (k == 0) ? nearest<true, false, 0, NB>(SL, 0, o, d, t, alive)
                           : nearest<false, false, 0, NB>(SL, 0, o, d, t, alive, prev);
            if (id < 0) alive = false;
            prev = id;
            if (alive) {
                st[k * BLOCK + tid] = t;
                so[k * BLOCK + tid] = id;
                nlev = k + 1;
                if (k == depth - 1 || hdr.n_light == 0) alive = false;
            }
            if (alive) {
                D3 hit, N;
                hit_geom(SL, id, o, d, t, hit, N);
                d = bounce3(d, N);
                o = hit;
            }
            if (__all(!alive)) break;
        }
        // backward: shade each level with the colour of the level below it (:216-247)
        int maxlev = 0;
        while (maxlev < depth && __ballot(nlev > maxlev) != 0) ++maxlev; // wave-wide max level
        for (int m = 0; m < maxlev; ++m) {
            const Scene SL = fresh_scene(S); // the header re-read per level (fresh_scene)
            const int k = nlev - 1 - m;
            const bool on = k >= 0;
            D3 o2 = cam, d2 = D3{sd0[tid], sd0[BLOCK + tid], sd0[2 * BLOCK + tid]}, hit = cam, N = cam;
            int id = 0;
            if (on) {
                for (int j = 0; j < k; ++j) { // replay the chain to level k
                    hit_geom(SL, so[j * BLOCK + tid], o2, d2, st[j * BLOCK + tid], hit, N);
                    d2 = bounce3(d2, N);
                    o2 = hit;
                }
                id = so[k * BLOCK + tid];
                hit_geom(SL, id, o2, d2, st[k * BLOCK + tid], hit, N);
            }
            const double refl = SL.tab[SL.h.o_obj + id * OBJ_W + 8];
            const D3 F = shade<GENPOW, 0, NB, true>(SL, id, d2, hit, N, col, refl, on);
            if (on) col = F;
        }
    } else {
        // ORDER_FAST: colour = sum_k W_k * S_k with W_0 = 1, W_{k+1} = W_k * (L * refl_k)
        D3 o = cam, d = d0;
        double w = 1.0;
        bool alive = active;
        int prev = -1;
        for (int k = 0; k < depth; ++k) {
            double t = 0;
            int id = -1;
            id = (k == 0) ? nearest<true, false, 0, NB>(S, 0, o, d, t, alive)
                           : nearest<false, false, 0, NB>(S, 0, o, d, t, alive, prev);
            if (id < 0) alive = false;
            prev = id;
            D3 hit = cam, N = cam;
            if (alive) {
                nlev = k + 1;
                hit_geom(S, id, o, d, t, hit, N);
            }
            if (__all(!alive)) break;
            const D3 F = shade<GENPOW, 0, NB>(S, alive ? id : 0, d, hit, N, D3{0.0, 0.0, 0.0}, 0.0, alive);
            if (alive) {
                col.x = col.x + w * F.x;
                col.y = col.y + w * F.y;
                col.z = col.z + w * F.z;
                w = w * (hdr.n_light_d * S.tab[hdr.o_obj + id * OBJ_W + 8]);
                if (k == depth - 1 || hdr.n_light == 0) alive = false;
                d = bounce3(d, N);
                o = hit;
            }
        }
    }
    if (!active) return; // slab rows past the image are not written
    // the pixel's address recomputed from an opaque thread index rather than kept live (spilled)
    // across the chain
    int t2 = threadIdx.x;
    asm volatile("" : "+v"(t2));
    const int x2 = blockIdx.x * TILE + ((t2 >> 6) & 1) * 8 + (t2 & 7);
    const int ly2 = row0 + blockIdx.y * TILE + ((t2 >> 6) >> 1) * 8 + ((t2 & 63) >> 3);
    const size_t pix = (size_t)ly2 * W + x2;
    if (PREC == RT_OUT_F64) {
        double *o = reinterpret_cast<double *>(out) + pix * 3;
        o[0] = col.x; o[1] = col.y; o[2] = col.z;
    } else {
        float *o = reinterpret_cast<float *>(out) + pix * 3;
        o[0] = (float)col.x; o[1] = (float)col.y; o[2] = (float)col.z;
    }
    if (LEVELS) levels[pix] = (uint8_t)(levels_hit ? (nlev > 0) : min(nlev, 255)); // (counts saturate at 255)
}
