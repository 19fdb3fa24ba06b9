// rt_quant.hip — integer frames on the GPU: the value rule of write_pixels_to_ppm/5
// (raytracer.erl:667-685) without the text, and the binary P6 file made from it.
//
// Every channel becomes min(trunc(C*MaxValue), MaxValue) in binary64, as quantise() in
// rt_ppm.hip computes it; an unsigned sample cannot hold what P3 prints as a negative number, so
// a result below 0 (C*MaxValue <= -1) or a NaN is stored as 0 and counted.  -0.0 and products in
// (-1, 0) truncate to 0 and are not counted.
//
// k_quant is bound by HBM bandwidth (24 B read, 3 B written per pixel of a binary64 frame to
// 8 bits).  The frame is a flat array: a lane takes QUANT_V = 8 consecutive values per iteration
// with 16-byte loads (four for binary64, two for binary32) and writes them with one store of
// 8 bytes (8-bit samples) or 16 bytes (16-bit samples), so a wave's stores are contiguous; a
// workgroup covers QUANT_B = 2048 values per iteration, the grid is capped at QUANT_MAX_BLOCKS
// workgroups and strides over the rest.  Up to 15 leading values (until the output is 16-byte
// aligned) and up to 7 trailing ones are done one by one by the first workgroup; when the input
// is not 16-byte aligned behind that head, the body loads element by element (same bytes).
//
// k_resolve (RT_PROGRESSIVE) is k_quant with a division in front and two more outputs: a binary64
// sum of `samples` samples becomes the frame sum / samples, stored as binary64, as binary32 or
// quantised by the rule above.  Same shape, same helpers; 24 B read per pixel and 24, 12, 3 or 6
// written.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_internal.h"

namespace {

constexpr int QUANT_BLOCK = 256;                 // work-items per workgroup
constexpr int QUANT_V = 8;                       // values per lane per iteration
constexpr int QUANT_B = QUANT_BLOCK * QUANT_V;   // values per workgroup per iteration
constexpr int QUANT_MAX_BLOCKS = 2048;           // grid cap (256 CUs x 8 workgroups)
static_assert(QUANT_V == 8 && QUANT_B == 2048, "load8 / store8 take 8 values; _native.py mirrors these as QUANT_*");

#define QCHK(x)                                                                                                    \
    do {                                                                                                           \
        hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) {                                                                                    \
            std::fprintf(stderr, "rt_mi355x: %s failed: %s\n", #x, hipGetErrorString(e_));                        \
            return RT_EHIP;                                                                                        \
        }                                                                                                          \
    } while (0)

// min(trunc(c * maxv), maxv), or 0 with *bad set when that is negative or not a number
__device__ inline unsigned quant1(double c, double maxv, unsigned maxi, bool *bad) {
    const double x = c * maxv;
    if (!(x > -1.0)) {       // trunc(x) <= -1, or NaN
        *bad = true;
        return 0u;
    }
    if (x >= maxv) return maxi; // also +inf
    return (unsigned)(int)x;    // (-1, maxv): the conversion truncates toward zero
}

template <typename TIN, bool VEC>
__device__ inline void load8(const TIN *p, double v[QUANT_V]);

template <>
__device__ inline void load8<double, true>(const double *p, double v[QUANT_V]) {
    const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
    for (int k = 0; k < QUANT_V / 2; ++k) {
        const double2 a = q[k];
        v[2 * k] = a.x;
        v[2 * k + 1] = a.y;
    }
}
template <>
__device__ inline void load8<float, true>(const float *p, double v[QUANT_V]) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int k = 0; k < QUANT_V / 4; ++k) {
        const float4 a = q[k];
        v[4 * k] = (double)a.x;
        v[4 * k + 1] = (double)a.y;
        v[4 * k + 2] = (double)a.z;
        v[4 * k + 3] = (double)a.w;
    }
}
template <>
__device__ inline void load8<double, false>(const double *p, double v[QUANT_V]) {
#pragma unroll
    for (int k = 0; k < QUANT_V; ++k) v[k] = p[k];
}
template <>
__device__ inline void load8<float, false>(const float *p, double v[QUANT_V]) {
#pragma unroll
    for (int k = 0; k < QUANT_V; ++k) v[k] = (double)p[k];
}

// p is 16-byte aligned (the host's head)
__device__ inline void store8(uint8_t *p, const unsigned q[QUANT_V]) {
    uint2 w;
    w.x = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
    w.y = q[4] | q[5] << 8 | q[6] << 16 | q[7] << 24;
    *reinterpret_cast<uint2 *>(p) = w;
}
__device__ inline void store8(uint16_t *p, const unsigned q[QUANT_V]) {
    uint4 w;
    w.x = q[0] | q[1] << 16;
    w.y = q[2] | q[3] << 16;
    w.z = q[4] | q[5] << 16;
    w.w = q[6] | q[7] << 16;
    *reinterpret_cast<uint4 *>(p) = w;
}

// the float outputs of k_resolve: one 16-byte piece, 2 binary64 or 4 binary32 values; p is 16-byte aligned
__device__ inline void store_piece(double *p, const double v[2]) { *reinterpret_cast<double2 *>(p) = double2{v[0], v[1]}; }
__device__ inline void store_piece(float *p, const double v[4]) {
    *reinterpret_cast<float4 *>(p) = float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// in/out: the whole array of n values; [head, head + nvec*QUANT_V) is the vector body, out + head
// 16-byte aligned (and in + head too when VEC).  *clamped += the values stored as 0 because they
// were negative or NaN: one atomic per wave that has any.
template <typename TIN, typename TOUT, bool VEC>
__global__ __launch_bounds__(QUANT_BLOCK) void k_quant(const TIN *__restrict__ in, TOUT *__restrict__ out, uint64_t n,
                                                       uint32_t head, uint64_t nvec, double maxv, unsigned maxi,
                                                       unsigned long long *__restrict__ clamped) {
    unsigned nbad = 0; // wave-uniform: every count below comes from a ballot
    const TIN *bin = in + head;
    TOUT *bout = out + head;
    // wave-uniform trip count, so that the ballots see the whole wave
    const uint64_t stride = (uint64_t)gridDim.x * QUANT_BLOCK;
    const uint64_t wave0 = (uint64_t)blockIdx.x * QUANT_BLOCK + (threadIdx.x & ~63u);
    for (uint64_t base = wave0; base < nvec; base += stride) {
        const uint64_t c = base + (threadIdx.x & 63u);
        unsigned badmask = 0;
        if (c < nvec) {
            double v[QUANT_V];
            unsigned q[QUANT_V];
            load8<TIN, VEC>(bin + c * QUANT_V, v);
#pragma unroll
            for (int k = 0; k < QUANT_V; ++k) {
                bool bad = false;
                q[k] = quant1(v[k], maxv, maxi, &bad);
                badmask |= (bad ? 1u : 0u) << k;
            }
            store8(bout + c * QUANT_V, q);
        }
        if (__ballot(badmask != 0)) { // rare: count value by value
#pragma unroll
            for (int k = 0; k < QUANT_V; ++k) nbad += (unsigned)__popcll(__ballot((badmask >> k) & 1u));
        }
    }
    if (blockIdx.x == 0) { // the scalar head and tail: fewer than 16 + 8 values
        const uint64_t tail0 = (uint64_t)head + nvec * QUANT_V;
        const uint64_t t = threadIdx.x;
        const uint64_t i = t < head ? t : tail0 + (t - head); // threads [head, head + tail) take the tail
        bool bad = false;
        if (i < n) out[i] = (TOUT)quant1((double)in[i], maxv, maxi, &bad);
        nbad += (unsigned)__popcll(__ballot(bad));
    }
    if (nbad && clamped && (threadIdx.x & 63u) == 0) atomicAdd(clamped, (unsigned long long)nbad);
}

template <typename TIN, typename TOUT>
void launch_quant(const void *in, void *out, uint64_t n, uint32_t head, bool vec, double maxv, unsigned maxi,
                  unsigned long long *clamped, hipStream_t st) {
    const uint64_t nvec = (n - head) / QUANT_V;
    const uint64_t want = (nvec + QUANT_BLOCK - 1) / QUANT_BLOCK;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want > QUANT_MAX_BLOCKS ? QUANT_MAX_BLOCKS : want);
    with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((k_quant<TIN, TOUT, decltype(v)::value>), dim3(grid), dim3(QUANT_BLOCK), 0, st,
                           static_cast<const TIN *>(in), static_cast<TOUT *>(out), n, head, nvec, maxv, maxi, clamped);
    });
}

// One value of a resolved frame: the mean as TOUT, quantised when TOUT is an integer.
template <typename TOUT>
__device__ inline TOUT resolve1(double m, double maxv, unsigned maxi, bool *bad) {
    if constexpr (std::is_floating_point<TOUT>::value)
        return (TOUT)m;
    else
        return (TOUT)quant1(m, maxv, maxi, bad);
}

// k_quant's arrangement (head, nvec, VEC, clamped: see there) for out[i] = in[i] / cnt, the plain
// binary64 division of k_accum and put_pixel, so that a resolved sum is the frame they write.
// Integer outputs are k_quant's body: a lane converts 8 consecutive values (its one store needs them).
// Float outputs deal the same 512 values of a wave to its lanes in 16-byte output pieces, so that each
// load and store instruction of the wave covers contiguous memory (a lane's own 8 values would put its
// four 16-byte stores 64 bytes apart).
template <typename TOUT, bool VEC>
__global__ __launch_bounds__(QUANT_BLOCK) void k_resolve(const double *__restrict__ in, TOUT *__restrict__ out,
                                                         uint64_t n, uint32_t head, uint64_t nvec, double cnt, double maxv,
                                                         unsigned maxi, unsigned long long *__restrict__ clamped) {
    constexpr bool INT = !std::is_floating_point<TOUT>::value;
    unsigned nbad = 0; // wave-uniform: every count below comes from a ballot
    const double *bin = in + head;
    TOUT *bout = out + head;
    const uint64_t stride = (uint64_t)gridDim.x * QUANT_BLOCK;
    const uint64_t wave0 = (uint64_t)blockIdx.x * QUANT_BLOCK + (threadIdx.x & ~63u);
    for (uint64_t base = wave0; base < nvec; base += stride) { // wave-uniform trip count (the ballots)
        if constexpr (!INT) {
            constexpr unsigned CH = 16 / sizeof(TOUT); // values per piece
            const uint64_t left = nvec - base;         // the wave's values: 8 per lane it would have had
            const unsigned nval = (unsigned)(left < 64 ? left : 64) * QUANT_V;
            const double *wi = bin + base * QUANT_V;
            TOUT *wo = bout + base * QUANT_V;
#pragma unroll
            for (unsigned k = 0; k < QUANT_V / CH; ++k) {
                const unsigned idx = (k * 64 + (threadIdx.x & 63u)) * CH;
                if (idx < nval) { // (nval is a multiple of 8: a piece is inside or outside as a whole)
                    double v[CH];
                    if constexpr (VEC) {
#pragma unroll
                        for (unsigned j = 0; j < CH; j += 2) {
                            const double2 a = *reinterpret_cast<const double2 *>(wi + idx + j);
                            v[j] = a.x;
                            v[j + 1] = a.y;
                        }
                    } else {
#pragma unroll
                        for (unsigned j = 0; j < CH; ++j) v[j] = wi[idx + j];
                    }
#pragma unroll
                    for (unsigned j = 0; j < CH; ++j) v[j] = v[j] / cnt;
                    store_piece(wo + idx, v);
                }
            }
            continue;
        }
        const uint64_t c = base + (threadIdx.x & 63u);
        unsigned badmask = 0;
        if (c < nvec) {
            double v[QUANT_V];
            unsigned q[QUANT_V];
            load8<double, VEC>(bin + c * QUANT_V, v);
#pragma unroll
            for (int k = 0; k < QUANT_V; ++k) {
                bool bad = false;
                q[k] = quant1(v[k] / cnt, maxv, maxi, &bad);
                badmask |= (bad ? 1u : 0u) << k;
            }
            if constexpr (INT) store8(bout + c * QUANT_V, q);
        }
        if (__ballot(badmask != 0)) { // rare: count value by value
#pragma unroll
            for (int k = 0; k < QUANT_V; ++k) nbad += (unsigned)__popcll(__ballot((badmask >> k) & 1u));
        }
    }
    if (blockIdx.x == 0) { // the scalar head and tail: fewer than 16 + 8 values
        const uint64_t tail0 = (uint64_t)head + nvec * QUANT_V;
        const uint64_t t = threadIdx.x;
        const uint64_t i = t < head ? t : tail0 + (t - head); // threads [head, head + tail) take the tail
        bool bad = false;
        if (i < n) out[i] = resolve1<TOUT>(in[i] / cnt, maxv, maxi, &bad);
        nbad += (unsigned)__popcll(__ballot(bad));
    }
    if (INT && nbad && clamped && (threadIdx.x & 63u) == 0) atomicAdd(clamped, (unsigned long long)nbad);
}

template <typename TOUT>
void launch_resolve(const double *in, void *out, uint64_t n, uint32_t head, bool vec, double cnt, double maxv,
                    unsigned maxi, unsigned long long *clamped, hipStream_t st) {
    const uint64_t nvec = (n - head) / QUANT_V;
    const uint64_t want = (nvec + QUANT_BLOCK - 1) / QUANT_BLOCK;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want > QUANT_MAX_BLOCKS ? QUANT_MAX_BLOCKS : want);
    with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((k_resolve<TOUT, decltype(v)::value>), dim3(grid), dim3(QUANT_BLOCK), 0, st, in,
                           static_cast<TOUT *>(out), n, head, nvec, cnt, maxv, maxi, clamped);
    });
}

void p6_header(char h[64], uint32_t W, uint32_t H, uint32_t maxv) { std::snprintf(h, 64, "P6\n%u %u\n%u\n", W, H, maxv); }

// the samples of a native-endian integer frame, 16-bit ones most significant byte first
int write_p6(const char *path, uint32_t W, uint32_t H, uint32_t maxv, void *samples) {
    const size_t nval = (size_t)W * H * 3;
    if (maxv > 255) {
        uint16_t *s = static_cast<uint16_t *>(samples);
        for (size_t i = 0; i < nval; ++i) {
            const unsigned char b[2] = {(unsigned char)(s[i] >> 8), (unsigned char)(s[i] & 0xFF)};
            std::memcpy(&s[i], b, 2);
        }
    }
    FILE *f = std::fopen(path, "wb");
    if (!f) return RT_EBADARG;
    char h[64];
    p6_header(h, W, H, maxv);
    const size_t bytes = nval * (maxv > 255 ? 2 : 1);
    int rc = RT_OK;
    if (std::fwrite(h, 1, std::strlen(h), f) != std::strlen(h) || std::fwrite(samples, 1, bytes, f) != bytes)
        rc = RT_EBADARG;
    if (std::fclose(f) != 0) rc = RT_EBADARG;
    return rc;
}

} // namespace

extern "C" {

int rt_quantize(const void *d_rgb, int precision, uint64_t n_values, uint32_t max_value, int out_format, void *d_out,
                uint64_t *d_clamped, void *stream) {
    if (!d_rgb || !d_out) return RT_EBADARG;
    if (!rt_is_float(precision)) return RT_EBADARG;
    if (!rt_is_int(out_format)) return RT_EBADARG;
    if (max_value == 0) return RT_EBADARG;
    if (max_value > rt_max_value_of(out_format)) return RT_ETOOBIG;
    const size_t isz = rt_elem_size(precision), osz = rt_elem_size(out_format);
    if ((uintptr_t)d_rgb % isz || (uintptr_t)d_out % osz || (uintptr_t)d_clamped % 8) return RT_EBADARG;
    if (n_values == 0) return RT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the head: values before the output's first 16-byte boundary
    uint64_t head = ((16 - (uintptr_t)d_out % 16) % 16) / osz;
    if (head > n_values) head = n_values;
    const bool vec = ((uintptr_t)d_rgb + head * isz) % 16 == 0;
    const double maxv = (double)max_value;
    unsigned long long *cl = reinterpret_cast<unsigned long long *>(d_clamped);
    with_format<RT_OUT_F64, RT_OUT_F32>(precision, [&](auto in) {
        with_format<RT_OUT_U8, RT_OUT_U16>(out_format, [&](auto out) {
            launch_quant<typename decltype(in)::type, typename decltype(out)::type>(d_rgb, d_out, n_values, (uint32_t)head, vec,
                                                                                    maxv, max_value, cl, st);
        });
    });
    QCHK(hipGetLastError());
    return RT_OK;
}

int rt_resolve(const double *d_sum, uint64_t n_values, uint32_t samples, int out_format, uint32_t max_value, void *d_out,
               uint64_t *d_clamped, void *stream) {
    if (!d_sum || !d_out) return RT_EBADARG;
    if (!rt_format_ok(out_format)) return RT_EBADARG;
    if (samples == 0) return RT_EBADARG;
    if (samples > RT_MAX_SPP) return RT_ETOOBIG;
    const bool integer = rt_is_int(out_format);
    if (integer && max_value == 0) return RT_EBADARG;
    if (integer && max_value > rt_max_value_of(out_format)) return RT_ETOOBIG;
    const size_t osz = rt_elem_size(out_format);
    if ((uintptr_t)d_sum % 8 || (uintptr_t)d_out % osz || (uintptr_t)d_clamped % 8) return RT_EBADARG;
    if (n_values == 0) return RT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the head: values before the output's first 16-byte boundary
    uint64_t head = ((16 - (uintptr_t)d_out % 16) % 16) / osz;
    if (head > n_values) head = n_values;
    const bool vec = ((uintptr_t)d_sum + head * 8) % 16 == 0;
    const double cnt = (double)samples, maxv = integer ? (double)max_value : 0.0;
    const unsigned maxi = integer ? max_value : 0u;
    unsigned long long *cl = reinterpret_cast<unsigned long long *>(d_clamped);
    with_format(out_format, [&](auto out) {
        launch_resolve<typename decltype(out)::type>(d_sum, d_out, n_values, (uint32_t)head, vec, cnt, maxv, maxi, cl, st);
    });
    QCHK(hipGetLastError());
    return RT_OK;
}

int rt_render_rawppm_file(const rt_elem *scene, uint32_t n, uint32_t img_w, uint32_t img_h, uint32_t depth,
                          const rt_opts *opts, uint32_t max_value, const char *path, rt_stats *stats) {
    const int value_rc = max_value == 0 ? RT_EBADARG : max_value > RT_MAX_INT_VALUE ? RT_ETOOBIG : RT_OK;
    rt_file_frame ff;
    int rc = rt_file_render(&ff, path, value_rc, scene, n, img_w, img_h, depth, opts);
    if (rc != RT_OK) return rc;
    const uint32_t width = ff.win.w, height = ff.win.h; // the file is the window's
    const int fmt = max_value > rt_max_value_of(RT_OUT_U8) ? RT_OUT_U16 : RT_OUT_U8;
    const size_t nval = ff.values(), bytes = nval * rt_elem_size(fmt);
    if (!ff.ctx) { // several devices: rt_render assembles the integer frame on the host
        ff.o.precision = fmt;
        ff.o.max_value = max_value;
        ff.o.out_levels = nullptr;
        std::vector<unsigned char> img(bytes);
        rt_stats st;
        std::memset(&st, 0, sizeof st);
        rc = rt_render(scene, n, img_w, img_h, depth, &ff.o, img.data(), &st);
        if (rc != RT_OK) return rc;
        if (stats) *stats = st;
        if (st.flags & RT_STATS_CLAMPED) return RT_ERANGE; // P3 would print a negative number
        return write_p6(path, width, height, max_value, img.data());
    }
    void *d_int = nullptr, *h_int = nullptr;
    uint64_t *d_clamped = nullptr;
    uint64_t clamped = 0;
    hipStream_t st = ff.st;
    do {
        if ((rc = rt_ctx_device_buffer(ff.ctx, 2, bytes, &d_int)) != RT_OK) break;
        if ((rc = rt_ctx_clamped(ff.ctx, &d_clamped)) != RT_OK) break;
        if ((rc = rt_ctx_host_buffer(ff.ctx, bytes, &h_int)) != RT_OK) break;
        if (hipMemsetAsync(d_clamped, 0, sizeof clamped, st) != hipSuccess) { rc = RT_EHIP; break; }
        if ((rc = rt_quantize(ff.d_rgb, RT_OUT_F64, nval, max_value, fmt, d_int, d_clamped, st)) != RT_OK) break;
        // the samples and the counter to pinned memory by DMA; the file is written from there
        if (hipMemcpyAsync(h_int, d_int, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(&clamped, d_clamped, sizeof clamped, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { rc = RT_EHIP; break; }
        if (clamped) { rc = RT_ERANGE; break; } // before the path is opened: no file
        rc = write_p6(path, width, height, max_value, h_int);
    } while (0);
    if (rc == RT_OK || rc == RT_ERANGE) ff.fill(stats);
    return rc;
}

} // extern "C"
