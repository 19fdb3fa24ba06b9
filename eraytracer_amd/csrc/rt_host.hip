// rt_host.hip — the host side of the boundary: the process's render contexts and rt_render,
// the one-shot drop-in for raytraced_pixel_list_{simple,concurrent,distributed}/4
// (raytracer.erl:86-178).
//
// The reference calls its strategy fun once per frame (raytrace/5, raytracer.erl:723-733), so
// what a call costs besides the kernels matters: compiling and uploading the scene, allocating
// the device frame and the wavefront work space (GBs at 4096^2), and moving the frame to the
// caller's host memory.  Here:
//  * contexts persist for the life of the process (per device, up to RT_CTX_PER_DEVICE
//    concurrent callers): streams, events, device buffers and work space are created once and
//    grown on demand; the scene is recompiled only when its bytes change;
//  * the frame is rendered in row bands, and each band's copy to the host runs on a second
//    stream while the next band renders; an integer frame's band is quantised (rt_quant.hip)
//    behind its render on the render stream, and the copy moves the 1- or 2-byte samples;
//  * a pinned destination (rt_host_alloc, or memory the caller registered with HIP) is written
//    by DMA directly; a pageable one goes through a pinned staging ring of two bands, copied
//    out by host threads while the next band's DMA is in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_bands.h"
#include "rt_internal.h"
#include "rt_scene.h"

namespace {

constexpr int RT_CTX_PER_DEVICE = 4;
// target output bytes per band (RT_BAND_MB overrides, for A/B runs)
size_t band_bytes() {
    static const size_t b = [] {
        const char *e = std::getenv("RT_BAND_MB");
        const long v = e ? std::atol(e) : 24;
        return (size_t)(v > 0 ? v : 24) << 20;
    }();
    return b;
}
// Test hook: RT_DEVICE_ALIAS=N makes rt_render see N devices that are all device first_dev, so
// its multi-device path (a context, work space and band pipeline per device, every device's
// slabs scattered into the one frame) runs on a one-GPU machine (0, the default: off)
int device_alias() {
    static const int n = [] {
        const char *e = std::getenv("RT_DEVICE_ALIAS");
        const int v = e ? std::atoi(e) : 0;
        return v > 0 && v <= RT_CTX_PER_DEVICE ? v : 0;
    }();
    return n;
}
// DMA queues a pinned frame's band copies alternate over (RT_COPY_STREAMS = 1, the default, or 2)
int copy_streams() {
    static const int n = [] {
        const char *e = std::getenv("RT_COPY_STREAMS");
        return e && std::atoi(e) == 2 ? 2 : 1;
    }();
    return n;
}
// the contexts' shading side streams: off (RT_CTX_SIDE_STREAMS=1 turns them on, for A/B runs)
int side_streams_env() {
    static const int v = [] {
        const char *e = std::getenv("RT_CTX_SIDE_STREAMS");
        return e && std::strcmp(e, "1") == 0 ? 1 : 0;
    }();
    return v;
}

} // namespace

struct rt_ctx {
    int device = -1;
    bool busy = false;
    hipStream_t render = nullptr, copy = nullptr, copy2 = nullptr; // copy2: a second DMA queue for pinned frames
    hipEvent_t e0 = nullptr, e1 = nullptr;      // timing: around the render launches
    hipEvent_t band[MAX_BANDS] = {};             // band rt_bands::event(i, b) rendered
    hipEvent_t copied[MAX_BANDS] = {};           // ... and copied to the host (staging or pinned)
    rt_prepared *p = nullptr;
    std::vector<unsigned char> key;              // bytes of the scene p was prepared from
    void *d_buf[3] = {};
    size_t d_cap[3] = {};
    uint64_t *d_clamped = nullptr;               // integer frames: values stored as 0 (negative or NaN)
    void *h_stage = nullptr;
    size_t h_cap = 0;
};

namespace {

std::mutex g_mu;
std::condition_variable g_cv;
std::vector<rt_ctx *> &pool() {
    static std::vector<rt_ctx *> *v = new std::vector<rt_ctx *>(); // never destroyed: contexts live with the process
    return *v;
}

void destroy_ctx(rt_ctx *c) {
    DevGuard g(c->device);
    if (c->p) rt_release(c->p);
    for (void *b : c->d_buf)
        if (b) (void)hipFree(b);
    if (c->d_clamped) (void)hipFree(c->d_clamped);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (hipEvent_t e : c->band)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->copied)
        if (e) (void)hipEventDestroy(e);
    if (c->e0) (void)hipEventDestroy(c->e0);
    if (c->e1) (void)hipEventDestroy(c->e1);
    if (c->render) (void)hipStreamDestroy(c->render);
    if (c->copy) (void)hipStreamDestroy(c->copy);
    if (c->copy2) (void)hipStreamDestroy(c->copy2);
    delete c;
}

int create_ctx(int device, rt_ctx **out) {
    rt_ctx *c = new (std::nothrow) rt_ctx();
    if (!c) return RT_ENOMEM;
    c->device = device;
    DevGuard g(device);
    int rc = g.ok ? RT_OK : RT_ENODEV;
    if (rc == RT_OK && (hipStreamCreateWithFlags(&c->render, hipStreamNonBlocking) != hipSuccess ||
                        hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking) != hipSuccess ||
                        hipStreamCreateWithFlags(&c->copy2, hipStreamNonBlocking) != hipSuccess ||
                        hipEventCreate(&c->e0) != hipSuccess || hipEventCreate(&c->e1) != hipSuccess))
        rc = RT_EHIP;
    for (int i = 0; rc == RT_OK && i < MAX_BANDS; ++i)
        if (hipEventCreateWithFlags(&c->band[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->copied[i], hipEventDisableTiming) != hipSuccess)
            rc = RT_EHIP;
    if (rc != RT_OK) {
        destroy_ctx(c);
        return rc;
    }
    *out = c;
    return RT_OK;
}

// The pinned staging ring's copy-out: rows [0, rows) of `src` (slab rows b0.., row pitch
// rowbytes) to their image rows in `dst` through the shard interleave, split over host threads.
void host_scatter(const char *src, uint32_t b0, uint32_t rows, uint32_t rowbytes, const rt_shard_map &m, char *dst) {
    auto body = [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const uint64_t g = rt_shard_image_row(m, (uint64_t)b0 + i);
            if (g < m.height) std::memcpy(dst + g * rowbytes, src + (uint64_t)i * rowbytes, rowbytes);
        }
    };
    const uint64_t bytes = (uint64_t)rows * rowbytes;
    unsigned nt = std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
    if (bytes < (4u << 20) || nt <= 1 || rows < 2 * nt) {
        body(0, rows);
        return;
    }
    std::vector<std::thread> th;
    const uint32_t per = (rows + nt - 1) / nt;
    for (unsigned t = 1; t < nt && t * per < rows; ++t) th.emplace_back(body, t * per, std::min(rows, (t + 1) * per));
    body(0, std::min(rows, per));
    for (std::thread &x : th) x.join();
}

bool is_pinned(const void *p, size_t bytes) {
    auto one = [](const void *q) {
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError(); // pageable memory: not an error of the call
            return false;
        }
        return a.type == hipMemoryTypeHost;
    };
    return bytes > 0 && one(p) && one(static_cast<const char *>(p) + bytes - 1);
}

} // namespace

// Slab rows [b0, b1) of shard m to their image rows (rt_internal.h).  The rows inside the image are
// a prefix of the slab, so the copies stop at the shard's valid rows.
int rt_scatter_rows_async(const char *slab, uint32_t b0, uint32_t b1, uint32_t rowbytes, const rt_shard_map &m,
                          char *image, hipMemcpyKind kind, hipStream_t st) {
    const uint32_t rb = m.row_block, ns = m.nshards, end = std::min(b1, rt_shard_valid_rows(m));
    for (uint32_t r = b0; r < end;) {
        char *dst = image + rt_shard_image_row(m, r) * rowbytes;
        const char *src = slab + (uint64_t)r * rowbytes;
        // whole row blocks inside [r, end): one strided copy
        const uint32_t nblk = ns > 1 && r % rb == 0 ? (end - r) / rb : 0;
        if (nblk > 0) {
            const size_t w = (size_t)rb * rowbytes;
            if (hipMemcpy2DAsync(dst, w * ns, src, w, w, nblk, kind, st) != hipSuccess) return RT_EHIP;
            r += nblk * rb;
            continue;
        }
        // the rest of this row block (contiguous in both); one shard: slab rows are image rows
        const uint32_t n = ns == 1 ? end - r : std::min(end - r, rb - r % rb);
        if (hipMemcpyAsync(dst, src, (size_t)n * rowbytes, kind, st) != hipSuccess) return RT_EHIP;
        r += n;
    }
    return RT_OK;
}

int rt_ctx_acquire(int device, const rt_elem *scene, uint32_t n, rt_ctx **out) {
    *out = nullptr;
    rt_ctx *c = nullptr;
    {
        std::unique_lock<std::mutex> lk(g_mu);
        for (;;) {
            rt_ctx *free_any = nullptr;
            int count = 0;
            const size_t kb = (size_t)n * sizeof(rt_elem);
            for (rt_ctx *x : pool()) {
                if (x->device != device) continue;
                ++count;
                if (x->busy) continue;
                if (x->key.size() == kb && std::memcmp(x->key.data(), scene, kb) == 0) {
                    c = x; // same scene already prepared
                    break;
                }
                if (!free_any) free_any = x;
            }
            if (!c) c = free_any;
            if (c) {
                c->busy = true;
                break;
            }
            if (count < RT_CTX_PER_DEVICE) {
                const int rc = create_ctx(device, &c);
                if (rc != RT_OK) return rc;
                c->busy = true;
                pool().push_back(c);
                break;
            }
            g_cv.wait(lk);
        }
    }
    const size_t kb = (size_t)n * sizeof(rt_elem);
    if (!(c->p && c->key.size() == kb && std::memcmp(c->key.data(), scene, kb) == 0)) {
        // a different scene: compile and upload it; the context's work space is kept
        int rc = c->p ? rt_prepare_scene(c->p, scene, n) : rt_prepare(scene, n, device, &c->p);
        // every kernel on the context's render stream: with the library's two shading side
        // streams beside the render and copy streams a process exceeds its 4 hardware queues,
        // and streams sharing a queue serialise behind each other's event waits (measured:
        // each row band then cost ~0.7 ms of render time whatever its size)
        if (rc == RT_OK) rc = rt_configure(c->p, RT_CFG_SIDE_STREAMS, side_streams_env());
        if (rc != RT_OK) {
            c->key.clear();
            rt_ctx_release(c);
            return rc;
        }
        c->key.assign(reinterpret_cast<const unsigned char *>(scene), reinterpret_cast<const unsigned char *>(scene) + kb);
    }
    *out = c;
    return RT_OK;
}

void rt_ctx_release(rt_ctx *c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        c->busy = false;
    }
    g_cv.notify_all();
}

rt_prepared *rt_ctx_prepared(rt_ctx *c) { return c->p; }
hipStream_t rt_ctx_stream(rt_ctx *c) { return c->render; }

int rt_ctx_device_buffer(rt_ctx *c, int which, size_t bytes, void **out) {
    if (which < 0 || which > 2) return RT_EBADARG;
    if (c->d_cap[which] < bytes) {
        DevGuard g(c->device);
        if (c->d_buf[which]) {
            (void)hipStreamSynchronize(c->render);
            (void)hipStreamSynchronize(c->copy);
            (void)hipStreamSynchronize(c->copy2);
            (void)hipFree(c->d_buf[which]);
        }
        c->d_buf[which] = nullptr;
        c->d_cap[which] = 0;
        if (hipMalloc(&c->d_buf[which], bytes) != hipSuccess) {
            c->d_buf[which] = nullptr;
            return RT_ENOMEM;
        }
        c->d_cap[which] = bytes;
    }
    *out = c->d_buf[which];
    return RT_OK;
}

int rt_ctx_clamped(rt_ctx *c, uint64_t **out) {
    if (!c->d_clamped) {
        DevGuard g(c->device);
        if (hipMalloc(reinterpret_cast<void **>(&c->d_clamped), sizeof(uint64_t)) != hipSuccess) {
            c->d_clamped = nullptr;
            return RT_ENOMEM;
        }
    }
    *out = c->d_clamped;
    return RT_OK;
}

int rt_ctx_host_buffer(rt_ctx *c, size_t bytes, void **out) {
    if (c->h_cap < bytes) {
        if (c->h_stage) {
            (void)hipStreamSynchronize(c->copy);
            (void)hipHostFree(c->h_stage);
        }
        c->h_stage = nullptr;
        c->h_cap = 0;
        if (hipHostMalloc(&c->h_stage, bytes, hipHostMallocPortable) != hipSuccess) {
            c->h_stage = nullptr;
            return RT_ENOMEM;
        }
        c->h_cap = bytes;
    }
    *out = c->h_stage;
    return RT_OK;
}

// rt_host_alloc keeps freed blocks for reuse (pinning is slow: a fresh 200 MB block costs
// milliseconds to tens of them, a NIF allocates one per frame): up to HOST_CACHE_BLOCKS blocks
// and HOST_CACHE_BYTES in all; a request takes the smallest cached block that fits and is at
// most twice its size.
namespace {
constexpr size_t HOST_CACHE_BLOCKS = 8;
constexpr size_t HOST_CACHE_BYTES = (size_t)4 << 30;
struct HostBlock {
    void *p;
    size_t n;
};
std::mutex g_host_mu;
std::vector<HostBlock> &host_live() { // blocks handed out (their sizes)
    static std::vector<HostBlock> *v = new std::vector<HostBlock>();
    return *v;
}
std::vector<HostBlock> &host_free() {
    static std::vector<HostBlock> *v = new std::vector<HostBlock>();
    return *v;
}
} // namespace

extern "C" {

void *rt_host_alloc(size_t bytes) {
    if (bytes == 0) return nullptr;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto &fr = host_free();
        int best = -1;
        for (size_t i = 0; i < fr.size(); ++i)
            if (fr[i].n >= bytes && fr[i].n / 2 <= bytes && (best < 0 || fr[i].n < fr[best].n)) best = (int)i;
        if (best >= 0) {
            HostBlock b = fr[best];
            fr.erase(fr.begin() + best);
            host_live().push_back(b);
            return b.p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_host_mu);
    host_live().push_back(HostBlock{p, bytes});
    return p;
}

int rt_host_free(void *p) {
    if (!p) return RT_OK;
    std::vector<void *> release;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto &lv = host_live();
        auto it = std::find_if(lv.begin(), lv.end(), [&](const HostBlock &b) { return b.p == p; });
        if (it == lv.end()) return RT_EBADARG; // not from rt_host_alloc (or freed twice)
        const HostBlock b = *it;
        lv.erase(it);
        auto &fr = host_free();
        fr.push_back(b);
        size_t total = 0;
        for (const HostBlock &x : fr) total += x.n;
        while (!fr.empty() && (fr.size() > HOST_CACHE_BLOCKS || total > HOST_CACHE_BYTES)) {
            total -= fr.front().n; // oldest first
            release.push_back(fr.front().p);
            fr.erase(fr.begin());
        }
    }
    for (void *q : release) (void)hipHostFree(q);
    return RT_OK;
}

// Device memory held by the idle contexts of `device` (their work space and output buffers), freed
// so that a caller whose allocation failed can retry: the pool caps contexts by count, and each
// keeps what its largest frame needed (about 5 GB at 4096^2 depth 5), so idle ones can crowd out
// a busy one.  Returns the bytes freed (0: nothing to free, the failure stands).
static size_t trim_idle(int device) {
    std::vector<rt_ctx *> idle;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (rt_ctx *c : pool())
            if (c->device == device && !c->busy) {
                c->busy = true; // claimed while trimmed
                idle.push_back(c);
            }
    }
    size_t freed = 0;
    for (rt_ctx *c : idle) {
        DevGuard g(c->device);
        (void)hipStreamSynchronize(c->render);
        (void)hipStreamSynchronize(c->copy);
        (void)hipStreamSynchronize(c->copy2);
        if (c->p) freed += rt_trim(c->p);
        for (int i = 0; i < 3; ++i) {
            if (c->d_buf[i]) (void)hipFree(c->d_buf[i]);
            freed += c->d_cap[i];
            c->d_buf[i] = nullptr;
            c->d_cap[i] = 0;
        }
    }
    if (!idle.empty()) {
        {
            std::lock_guard<std::mutex> lk(g_mu);
            for (rt_ctx *c : idle) c->busy = false;
        }
        g_cv.notify_all();
    }
    return freed;
}

int rt_reset_contexts(void) {
    std::vector<rt_ctx *> dead;
    int busy = 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        std::vector<rt_ctx *> keep;
        for (rt_ctx *c : pool()) (c->busy ? keep : dead).push_back(c);
        busy = (int)keep.size();
        pool().swap(keep);
    }
    {
        std::vector<HostBlock> fr;
        {
            std::lock_guard<std::mutex> lk(g_host_mu);
            fr.swap(host_free());
        }
        for (const HostBlock &b : fr) (void)hipHostFree(b.p);
    }
    for (rt_ctx *c : dead) {
        DevGuard g(c->device);
        (void)hipStreamSynchronize(c->render);
        (void)hipStreamSynchronize(c->copy);
        (void)hipStreamSynchronize(c->copy2);
        destroy_ctx(c);
    }
    return busy;
}

} // extern "C"

// ---- rt_render, in stages ---------------------------------------------------------------------
namespace {

struct RenderDev { // a used device: its context and its buffers, for all of the device's shards
    rt_ctx *c = nullptr;
    char *d_ren = nullptr, *d_out = nullptr; // the slabs the kernels render into, the slabs the copies read
    char *stage = nullptr;
    uint8_t *d_lv = nullptr;
    uint64_t *d_cl = nullptr;
};
// What the stages share: the call, its plan and its devices.
struct Render {
    const rt_elem *scene;
    uint32_t n, img_w, img_h, depth;
    char *out;     // the caller's frame
    rt_opts o;     // the options, loaded; ndev resolved
    rt_window win; // the raster this call renders and returns
    bool integer, pinned;
    rt_bands plan;
    // an integer frame is rendered in binary64 (frame.precision, rrow bytes per row) and quantised band
    // by band into the integer slab; rowbytes / slab_bytes describe what is copied to the host
    uint32_t rowbytes;
    size_t rrow, rslab_bytes, slab_bytes;
    rt_frame frame; // what every shard renders (its index filled in per shard): the window, in the render precision
    std::vector<RenderDev> dev;
    rt_shard_map map(uint32_t shard) const { return rt_shard_map{win.h, o.row_block, shard, plan.nshards}; }
};

// The argument checks in their documented order, then the plan.  No HIP call before the device count.
int render_plan(Render &r, const rt_opts *opts, void *out_rgb) {
    if (r.img_w == 0 && r.img_h == 0) return RT_DONE;
    if (r.img_w == 0 || r.img_h == 0) return RT_EBADARG;
    if (!out_rgb) return RT_EBADARG;
    rt_opts &o = r.o;
    rt_opts_load(opts, &o);
    if (!rt_format_ok(o.precision)) return RT_EBADARG;
    r.integer = rt_is_int(o.precision);
    if (r.integer && o.max_value > rt_max_value_of(o.precision)) return RT_ETOOBIG;
    if (o.order != RT_ORDER_EXACT && o.order != RT_ORDER_FAST) return RT_EBADARG;
    if (o.spp > RT_MAX_SPP) return RT_ETOOBIG;
    if (r.img_w > (1u << 20) || r.img_h > (1u << 20)) return RT_ETOOBIG;
    // The window (opts->win_*): from here on win is the raster this call renders and returns —
    // slabs, bands, staging, levels and the scatter are sized on it — and only rt_launch_rows is
    // handed the image's (img_w, img_h) and the origin.
    int rc = rt_opts_window(o, r.img_w, r.img_h, &r.win);
    if (rc != RT_OK) return rc;
    rc = rtl::check_scene(r.scene, r.n);
    if (rc != RT_OK) return rc;
    int navail = 0;
    if (hipGetDeviceCount(&navail) != hipSuccess || navail <= 0) return RT_ENODEV;
    if (device_alias() > 0) {
        if (o.first_dev < 0 || o.first_dev >= navail) return RT_ENODEV;
        navail = o.first_dev + device_alias();
    }
    if (o.ndev < 0) o.ndev = navail - o.first_dev;
    if (o.first_dev < 0 || o.ndev <= 0 || o.first_dev + o.ndev > navail) return RT_ENODEV;
    const uint32_t ns = o.nshards ? o.nshards : (uint32_t)o.ndev;
    if (ns > RT_MAX_SHARDS) return RT_ETOOBIG;
    const uint32_t nd = std::min<uint32_t>(ns, (uint32_t)o.ndev); // devices used; shard s on device s % nd
    r.frame = rt_opts_frame(o, r.img_w, r.img_h, r.win, r.depth);
    r.frame.nshards = ns;
    r.frame.precision = r.integer ? RT_OUT_F64 : o.precision;
    r.rowbytes = r.win.w * 3 * (uint32_t)rt_elem_size(o.precision);
    r.plan = rt_band_plan(r.win.h, o.row_block, ns, nd, r.rowbytes, band_bytes());
    r.rrow = (size_t)r.win.w * 3 * rt_elem_size(r.frame.precision);
    r.rslab_bytes = (size_t)r.plan.slab * r.rrow;
    r.slab_bytes = (size_t)r.plan.slab * r.rowbytes;
    r.out = static_cast<char *>(out_rgb);
    r.pinned = is_pinned(out_rgb, (size_t)r.win.h * r.rowbytes);
    r.dev.assign(nd, RenderDev());
    return RT_OK;
}

// an allocation that fails while other contexts of the device sit idle on their memory is
// retried once after those are trimmed (trim_idle)
template <typename F>
int retry_trimmed(int dev, F &&alloc) {
    int e = alloc();
    if (e == RT_ENOMEM && trim_idle(dev) > 0) e = alloc();
    return e;
}

// Device d's context, made current, and its buffers.
int render_acquire(Render &r, uint32_t d) {
    RenderDev &v = r.dev[d];
    const int dev = device_alias() > 0 ? r.o.first_dev : r.o.first_dev + (int)d;
    int err = rt_ctx_acquire(dev, r.scene, r.n, &v.c);
    if (err != RT_OK) return err;
    (void)hipSetDevice(dev);
    const uint32_t k = r.plan.shards_of(d);
    auto buffer = [&](int which, size_t bytes, void *out) {
        return retry_trimmed(dev, [&] { return rt_ctx_device_buffer(v.c, which, bytes, static_cast<void **>(out)); });
    };
    err = buffer(0, k * r.rslab_bytes, &v.d_ren);
    v.d_out = v.d_ren;
    if (err == RT_OK && r.integer) {
        err = buffer(2, k * r.slab_bytes, &v.d_out);
        if (err == RT_OK) err = rt_ctx_clamped(v.c, &v.d_cl);
        if (err == RT_OK && hipMemsetAsync(v.d_cl, 0, sizeof(uint64_t), v.c->render) != hipSuccess) err = RT_EHIP;
    }
    if (err == RT_OK && r.o.out_levels) err = buffer(1, (size_t)k * r.plan.slab * r.win.w, &v.d_lv);
    if (err == RT_OK && !r.pinned)
        err = rt_ctx_host_buffer(v.c, 2 * (size_t)r.plan.band * r.rowbytes, reinterpret_cast<void **>(&v.stage));
    return err;
}

// Band b of device d's i-th shard (r.frame.shard): its render on the render stream and, into a
// pinned frame, its copy on a copy stream behind it.
int render_band(Render &r, uint32_t d, uint32_t i, uint32_t b) {
    const RenderDev &v = r.dev[d];
    rt_ctx *c = v.c;
    const uint32_t slab = r.plan.slab, ev = r.plan.event(i, b);
    char *slab_out = v.d_out + i * r.slab_bytes, *slab_ren = v.d_ren + i * r.rslab_bytes;
    uint8_t *slab_lv = r.o.out_levels ? v.d_lv + (size_t)i * slab * r.win.w : nullptr;
    const uint32_t b0 = r.plan.row0(b), b1 = r.plan.row1(b);
    // image rows of the shard = its slab rows [0, valid): the rest of the slab is never rendered
    const uint32_t end = std::min(b1, r.frame.valid_rows());
    int err = retry_trimmed(c->device, [&] { // (a failed grow launches nothing)
        return rt_launch_rows(c->p, r.frame, b0, b1, slab_ren, slab_lv, c->render, (r.o.flags & RT_LEVELS_HIT) ? 1 : 0);
    });
    // integer frame: the band's image rows quantised behind its render, before its event
    if (err == RT_OK && r.integer && b0 < end)
        err = rt_quantize(slab_ren + (size_t)b0 * r.rrow, RT_OUT_F64, (uint64_t)(end - b0) * r.win.w * 3, r.o.max_value,
                          r.o.precision, slab_out + (size_t)b0 * r.rowbytes, v.d_cl, c->render);
    if (err == RT_OK && hipEventRecord(c->band[ev], c->render) != hipSuccess) err = RT_EHIP;
    if (err == RT_OK && r.pinned) {
        hipStream_t cs = (ev % copy_streams()) ? c->copy2 : c->copy;
        if (hipStreamWaitEvent(cs, c->band[ev], 0) != hipSuccess) err = RT_EHIP;
        if (err == RT_OK)
            err = rt_scatter_rows_async(slab_out, b0, b1, r.rowbytes, r.map(r.frame.shard), r.out, hipMemcpyDeviceToHost, cs);
    }
    return err;
}

// Every band of device d's shards, between the timing events.
int render_enqueue(Render &r, uint32_t d) {
    rt_ctx *c = r.dev[d].c;
    int err = hipEventRecord(c->e0, c->render) == hipSuccess ? RT_OK : RT_EHIP;
    for (uint32_t i = 0; i < r.plan.shards_of(d) && err == RT_OK; ++i) {
        r.frame.shard = d + i * r.plan.ndev;
        for (uint32_t b = 0; b < r.plan.nb && err == RT_OK; ++b) err = render_band(r, d, i, b);
    }
    if (err == RT_OK && hipEventRecord(c->e1, c->render) != hipSuccess) err = RT_EHIP;
    return err;
}

// pageable destination: DMA into a ring of two staging bands, copied out by host threads
// while the next band's DMA runs
int render_drain(Render &r, uint32_t d) {
    const RenderDev &v = r.dev[d];
    rt_ctx *c = v.c;
    (void)hipSetDevice(c->device);
    const rt_bands &pl = r.plan;
    const uint32_t nb = pl.nb, rowbytes = r.rowbytes;
    const uint32_t total = pl.shards_of(d) * nb; // bands j = event(i, b): shard i = j / nb, band b = j % nb
    auto stage = [&](uint32_t j) { return v.stage + (size_t)(j & 1) * pl.band * rowbytes; };
    auto enqueue = [&](uint32_t j) -> int {
        const uint32_t b0 = pl.row0(j % nb), b1 = pl.row1(j % nb);
        const char *src = v.d_out + (j / nb) * r.slab_bytes + (size_t)b0 * rowbytes;
        if (hipStreamWaitEvent(c->copy, c->band[j], 0) != hipSuccess ||
            hipMemcpyAsync(stage(j), src, (size_t)(b1 - b0) * rowbytes, hipMemcpyDeviceToHost, c->copy) != hipSuccess ||
            hipEventRecord(c->copied[j], c->copy) != hipSuccess)
            return RT_EHIP;
        return RT_OK;
    };
    int err = RT_OK;
    for (uint32_t j = 0; j < total && j < 2 && err == RT_OK; ++j) err = enqueue(j);
    for (uint32_t j = 0; j < total && err == RT_OK; ++j) {
        if (hipEventSynchronize(c->copied[j]) != hipSuccess) return RT_EHIP;
        const uint32_t b0 = pl.row0(j % nb), b1 = pl.row1(j % nb);
        host_scatter(stage(j), b0, b1 - b0, rowbytes, r.map(d + (j / nb) * pl.ndev), r.out);
        if (j + 2 < total) err = enqueue(j + 2);
    }
    return err;
}

// levels (1 byte per pixel) after the frame
int render_levels(Render &r, uint32_t d) {
    rt_ctx *c = r.dev[d].c;
    (void)hipSetDevice(c->device);
    const uint32_t k = r.plan.shards_of(d), slab = r.plan.slab, width = r.win.w;
    std::vector<uint8_t> tmp((size_t)k * slab * width);
    if (hipStreamSynchronize(c->render) != hipSuccess ||
        hipMemcpy(tmp.data(), r.dev[d].d_lv, tmp.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return RT_EHIP;
    for (uint32_t i = 0; i < k; ++i)
        host_scatter(reinterpret_cast<const char *>(tmp.data()) + (size_t)i * slab * width, 0, slab, width,
                     r.map(d + i * r.plan.ndev), reinterpret_cast<char *>(r.o.out_levels));
    return RT_OK;
}

// Every acquired context drained and released, whatever err the stages ended with; the stats.
int render_finish(Render &r, int err, rt_stats *stats, std::chrono::steady_clock::time_point t_begin) {
    double kms = 0;
    uint64_t clamped = 0;
    for (const RenderDev &v : r.dev) {
        rt_ctx *c = v.c;
        if (!c) continue;
        (void)hipSetDevice(c->device);
        if (hipStreamSynchronize(c->render) != hipSuccess && err == RT_OK) err = RT_EHIP;
        if (hipStreamSynchronize(c->copy) != hipSuccess && err == RT_OK) err = RT_EHIP;
        if (hipStreamSynchronize(c->copy2) != hipSuccess && err == RT_OK) err = RT_EHIP;
        float ms = 0;
        if (err == RT_OK && hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess && ms > kms) kms = ms;
        if (err == RT_OK && v.d_cl) {
            uint64_t cnt = 0;
            if (hipMemcpy(&cnt, v.d_cl, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess) err = RT_EHIP;
            clamped += cnt;
        }
        rt_ctx_release(c);
    }
    if (stats) {
        stats->kernel_ms = kms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        stats->pixels = (uint64_t)r.win.w * r.win.h;
        stats->ndev = (int32_t)r.plan.ndev;
        stats->flags = (r.pinned ? RT_STATS_PINNED : 0) | (clamped ? RT_STATS_CLAMPED : 0);
    }
    return err;
}

} // namespace

extern "C" int rt_render(const rt_elem *scene, uint32_t n, uint32_t img_w, uint32_t img_h, uint32_t depth,
                         const rt_opts *opts, void *out_rgb, rt_stats *stats) {
    const auto t_begin = std::chrono::steady_clock::now();
    Render r = {scene, n, img_w, img_h, depth};
    int err = render_plan(r, opts, out_rgb);
    if (err != RT_OK) return err;
    const uint32_t nd = r.plan.ndev;
    DevGuard restore; // (the stages select each context's device themselves)
    for (uint32_t d = 0; d < nd && err == RT_OK; ++d) {
        err = render_acquire(r, d);
        if (err == RT_OK) err = render_enqueue(r, d);
    }
    for (uint32_t d = 0; d < nd && err == RT_OK && !r.pinned; ++d) err = render_drain(r, d);
    for (uint32_t d = 0; d < nd && err == RT_OK && r.o.out_levels; ++d) err = render_levels(r, d);
    return render_finish(r, err, stats, t_begin);
}

int rt_file_render(rt_file_frame *ff, const char *path, int value_rc, const rt_elem *scene, uint32_t n, uint32_t img_w,
                   uint32_t img_h, uint32_t depth, const rt_opts *opts) {
    if (!path) return RT_EBADARG;
    if (img_w == 0 && img_h == 0) return RT_DONE;
    if (img_w == 0 || img_h == 0) return RT_EBADARG;
    if (value_rc != RT_OK) return value_rc;
    rt_opts &o = ff->o;
    rt_opts_load(opts, &o);
    int rc = rt_opts_window(o, img_w, img_h, &ff->win);
    if (rc != RT_OK) return rc;
    if (o.ndev != 1) return RT_OK;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || o.first_dev < 0 || o.first_dev >= nd) return RT_ENODEV;
    // the process's render context for this device: scene, streams, frame and text or sample
    // buffers and the pinned host buffer persist across calls
    rc = rt_ctx_acquire(o.first_dev, scene, n, &ff->ctx);
    if (rc != RT_OK) return rc;
    ff->dev.emplace(o.first_dev);
    ff->st = rt_ctx_stream(ff->ctx);
    rc = rt_ctx_device_buffer(ff->ctx, 0, ff->values() * sizeof(double), &ff->d_rgb);
    if (rc != RT_OK) return rc;
    return rt_launch_rows(rt_ctx_prepared(ff->ctx), rt_opts_frame(o, img_w, img_h, ff->win, depth), 0, ~0u, ff->d_rgb,
                          nullptr, ff->st, 0);
}
