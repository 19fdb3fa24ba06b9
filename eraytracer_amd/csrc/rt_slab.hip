// rt_slab.hip — compact slabs for the multi-GPU frame gather (include/rt_mi355x.h, "compact
// slab transfer").
//
// The reference's master collects every pixel from its workers (raytracer.erl:151-161,
// :169-178); here each rank renders its interleaved rows into a slab in HBM and rank 0
// gathers the slabs over xGMI.  Rendering runs at ~27 Gpx/s per MI355X, i.e. ~325 GB/s of
// f32 RGB per GPU, so with 8 ranks the gather into rank 0 (7 inbound links) and not the
// render bounds a frame.  Most pixels are background (the reference's BACKGROUND_COLOUR,
// raytracer.erl:186-203, exactly +0.0 in every channel: 73 % of S64's pixels), so a slab
// is sent as
//     header (fixed size):  u64 count | u32 block_off[nblk] | u64 mask[4*nblk]
//     values (count*3 elements of the slab's precision): the non-zero pixels in slab order
// with one mask bit per slab pixel (a pixel is "zero" iff all three channels are +0.0
// bit for bit, so the round trip is exact) and, per 256-pixel block, the number of
// non-zero pixels before it.  Slab rows past the image are never written by rt_launch and
// are encoded as zero without being read.
//
// Pack: k_mask (one wave per 64 pixels: ballot -> mask word, block popcount), k_scan (one
// workgroup, exclusive scan of the block counts -> offsets and the count), k_compact
// (non-zero pixels copied to their rank).  Unpack on rank 0 is fused with the reorder of
// rt_unshard: one workgroup per image row and 256 columns (the row's shard and slab row are
// wave-uniform), one thread per pixel finds its mask bit and reads its value, so the full
// frame is written once.
//
// Integer slabs (RT_OUT_U8 / RT_OUT_U16: a binary64 slab quantised by rt_quantize where it was
// rendered) take the same header; their values are 3 or 6 bytes per non-zero pixel, and a pixel
// is zero iff its three samples are.  Mask and compaction are the same kernels on 1- and 2-byte
// elements; the decode of an aligned frame is k_unpack_int (48 bytes of an image row per thread).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/rt_mi355x.h"
#include "rt_format.h"
#include "rt_shard.h"

namespace {

constexpr int SLAB_BLOCK = 256;       // pixels per offset entry = threads per pack workgroup
constexpr size_t HDR_OFFS = 64;       // block offsets start here (the count sits at 0)

#define SLABCHK(x)                                                                                                 \
    do {                                                                                                           \
        hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) {                                                                                    \
            std::fprintf(stderr, "rt_mi355x: %s failed: %s\n", #x, hipGetErrorString(e_));                        \
            return RT_EHIP;                                                                                        \
        }                                                                                                          \
    } while (0)

struct Layout {
    uint64_t px;      // slab pixels (rows * width)
    uint64_t nblk;    // 256-pixel blocks
    uint64_t mask_at; // byte offset of the mask words
    uint64_t bytes;   // header size
};

__host__ __device__ inline Layout layout(uint32_t width, uint32_t rows) {
    Layout l;
    l.px = (uint64_t)width * rows;
    l.nblk = (l.px + SLAB_BLOCK - 1) / SLAB_BLOCK;
    l.mask_at = (HDR_OFFS + l.nblk * 4 + 255) / 256 * 256;
    l.bytes = l.mask_at + l.nblk * (SLAB_BLOCK / 8);
    return l;
}

template <typename T>
__device__ inline bool nonzero(const T *__restrict__ slab, uint64_t p) {
    return (slab[p * 3] | slab[p * 3 + 1] | slab[p * 3 + 2]) != 0;
}

// one thread per slab pixel: mask words (one per wave) and the block's non-zero count.  The slab
// rows inside the image are a prefix of the slab (global rows grow with slab rows), so a pixel
// is in the image iff p < valid_px.
template <typename T>
__global__ __launch_bounds__(SLAB_BLOCK) void k_mask(const T *__restrict__ slab, uint64_t valid_px,
                                                     uint32_t *__restrict__ blk_cnt, uint64_t *__restrict__ mask) {
    __shared__ uint32_t s_cnt[SLAB_BLOCK / 64];
    const uint64_t p = (uint64_t)blockIdx.x * SLAB_BLOCK + threadIdx.x;
    const bool nz = p < valid_px && nonzero(slab, p);
    const uint64_t m = __ballot(nz);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        mask[p / 64] = m;
        s_cnt[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// exclusive scan of the block counts in place (one workgroup, any count); the total to *count.
// Tiles of SCAN_T * 1024 counts go through LDS: loaded and stored coalesced, each thread sums and
// rewrites SCAN_T consecutive counts there, and a wave scan (shuffles) plus the 16 wave totals
// ranks the threads (4096^2 / 8192^2 shards at N = 8: one / four tiles).  4096^2 / 8192^2 shard
// packs 0.024 -> 0.017 / 0.103 -> 0.061 ms against one thread walking 8 / 32 counts twice
// (profiles/r06ak_codec_ab.txt).  The counts and the
// total are < 2^32: the host checks px < 2^32.
constexpr int SCAN_T = 8, SCAN_TILE = 1024 * SCAN_T;
__device__ inline uint32_t scan_pad(uint32_t i) { return i + (i >> 5); } // (spreads a thread's run over banks)
__global__ __launch_bounds__(1024) void k_scan(uint32_t *__restrict__ blk, uint64_t n, uint64_t *__restrict__ count) {
    __shared__ uint32_t s[SCAN_TILE + SCAN_TILE / 32];
    __shared__ uint32_t s_w[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += SCAN_TILE) {
#pragma unroll
        for (int j = 0; j < SCAN_T; ++j) {
            const uint64_t i = base + j * 1024 + t;
            s[scan_pad(j * 1024 + t)] = i < n ? blk[i] : 0u;
        }
        __syncthreads();
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < SCAN_T; ++j) acc += s[scan_pad(t * SCAN_T + j)];
        uint32_t inc = acc; // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += u;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        uint32_t wpre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t x = s_w[k];
            wpre += (uint32_t)k < w ? x : 0u;
            tot += x;
        }
        uint32_t run = carry + wpre + inc - acc;
#pragma unroll
        for (int j = 0; j < SCAN_T; ++j) {
            const uint32_t q = scan_pad(t * SCAN_T + j), x = s[q];
            s[q] = run;
            run += x;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SCAN_T; ++j) {
            const uint64_t i = base + j * 1024 + t;
            if (i < n) blk[i] = s[scan_pad(j * 1024 + t)];
        }
        carry += tot;
        __syncthreads(); // (s and s_w are refilled by the next tile)
    }
    if (t == 0) *count = carry;
}

// rank of slab pixel p among the non-zero pixels (its mask bit is set)
__device__ inline uint64_t rank_of(const uint32_t *__restrict__ off, const uint64_t *__restrict__ mask, uint64_t p) {
    const uint64_t w = p / 64, w0 = (p / SLAB_BLOCK) * (SLAB_BLOCK / 64);
    uint64_t r = off[p / SLAB_BLOCK];
    for (uint64_t i = w0; i < w; ++i) r += __popcll(mask[i]);
    const uint64_t below = (1ull << (p % 64)) - 1ull;
    return r + __popcll(mask[w] & below);
}

// non-zero pixels to their rank: the wave's mask word gives each lane its place
template <typename T>
__global__ __launch_bounds__(SLAB_BLOCK) void k_compact(const T *__restrict__ slab, uint64_t px,
                                                        const uint32_t *__restrict__ off,
                                                        const uint64_t *__restrict__ mask, T *__restrict__ vals) {
    const uint64_t p = (uint64_t)blockIdx.x * SLAB_BLOCK + threadIdx.x;
    if (p >= px) return;
    if (!((mask[p / 64] >> (p % 64)) & 1ull)) return;
    const uint64_t r = rank_of(off, mask, p);
    if (r >= px) return; // a consistent header never ranks past the slab (values hold px pixels)
    vals[r * 3] = slab[p * 3];
    vals[r * 3 + 1] = slab[p * 3 + 1];
    vals[r * 3 + 2] = slab[p * 3 + 2];
}

struct ShardPtrs {
    const unsigned char *hdr[RT_MAX_SHARDS];
    const void *vals[RT_MAX_SHARDS];
};

// one workgroup per (image row g, 256 columns): the row's shard and slab row are wave-uniform
// (no per-lane division), each lane finds its pixel's mask bit and value
template <typename T>
__global__ __launch_bounds__(SLAB_BLOCK) void k_unpack(ShardPtrs sp, uint64_t mask_at, uint64_t px, uint32_t W,
                                                       uint32_t ncol, uint32_t rb, uint32_t ns, T *__restrict__ image) {
    const uint32_t g = blockIdx.x / ncol, c = blockIdx.x - g * ncol;
    const uint32_t x = c * SLAB_BLOCK + threadIdx.x;
    if (x >= W) return;
    const uint32_t blk = g / rb, s = blk % ns;
    const uint64_t lr = (uint64_t)(blk / ns) * rb + (g - blk * rb);
    const uint64_t p = lr * W + x;
    const unsigned char *h = sp.hdr[s];
    const uint32_t *off = reinterpret_cast<const uint32_t *>(h + HDR_OFFS);
    const uint64_t *mask = reinterpret_cast<const uint64_t *>(h + mask_at);
    T c0 = 0, c1 = 0, c2 = 0;
    const uint64_t r = ((mask[p / 64] >> (p % 64)) & 1ull) ? rank_of(off, mask, p) : px;
    if (r < px) { // (a consistent header never ranks past the slab: values hold px pixels)
        const T *v = static_cast<const T *>(sp.vals[s]) + r * 3;
        c0 = v[0];
        c1 = v[1];
        c2 = v[2];
    }
    T *o = image + ((uint64_t)g * W + x) * 3;
    o[0] = c0;
    o[1] = c1;
    o[2] = c2;
}

// Frames whose width is a multiple of 4: each thread decodes 4 consecutive pixels of an image row
// (their mask bits share one word: p is a multiple of 4), one workgroup per (row, 1024 columns).
// The frame is the bulk of the decode's traffic (201 MB at 4096^2 f32 against ~55 MB of values
// for S64), so the stores decide its speed: each thread's 3 (binary32) or 6 (binary64) 16-byte
// pieces are staged in LDS and the workgroup writes its contiguous stretch of the frame with lane i
// of a store instruction at 16 i bytes (1 KiB per wave instruction instead of 16 B every 48 B),
// non-temporal (the frame is not read back on the device).  4096^2 f32, 8 shards: 0.068 -> 0.035 ms,
// 7.4 TB/s of algorithmic bytes (profiles/r06aj_codec_ab.txt).
constexpr int UNPACK_PX = 4;
template <typename T>
__global__ __launch_bounds__(SLAB_BLOCK) void k_unpack4(ShardPtrs sp, uint64_t mask_at, uint64_t px, uint32_t W,
                                                         uint32_t ncol, uint32_t rb, uint32_t ns, T *__restrict__ image) {
    constexpr int Q = 3 * UNPACK_PX * (int)sizeof(T) / 16; // 16-byte pieces per thread
    __shared__ uint4 s_out[SLAB_BLOCK * Q];
    const uint32_t g = blockIdx.x / ncol, c = blockIdx.x - g * ncol;
    const uint32_t x0 = c * SLAB_BLOCK * UNPACK_PX, x = x0 + threadIdx.x * UNPACK_PX;
    const uint32_t nact = (W - x0 < SLAB_BLOCK * UNPACK_PX ? W - x0 : SLAB_BLOCK * UNPACK_PX) / UNPACK_PX;
    if (x < W) {
        const uint32_t blk = g / rb, s = blk % ns;
        const uint64_t lr = (uint64_t)(blk / ns) * rb + (g - blk * rb);
        const uint64_t p = lr * W + x; // a multiple of 4 (W is)
        const unsigned char *h = sp.hdr[s];
        const uint32_t *off = reinterpret_cast<const uint32_t *>(h + HDR_OFFS);
        const uint64_t *mask = reinterpret_cast<const uint64_t *>(h + mask_at);
        const unsigned bits = (unsigned)(mask[p / 64] >> (p % 64)) & 0xFu;
        T v[3 * UNPACK_PX];
#pragma unroll
        for (int k = 0; k < 3 * UNPACK_PX; ++k) v[k] = 0;
        if (bits) {
            uint64_t r = rank_of(off, mask, p);
            if (r + __popc(bits) <= px) { // (a consistent header never ranks past the slab)
                const T *src = static_cast<const T *>(sp.vals[s]);
#pragma unroll
                for (int k = 0; k < UNPACK_PX; ++k) {
                    if ((bits >> k) & 1u) {
                        v[3 * k] = src[r * 3];
                        v[3 * k + 1] = src[r * 3 + 1];
                        v[3 * k + 2] = src[r * 3 + 2];
                        ++r;
                    }
                }
            }
        }
        uint4 *so = s_out + threadIdx.x * Q;
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                so[k] = make_uint4((unsigned)v[4 * k], (unsigned)v[4 * k + 1], (unsigned)v[4 * k + 2], (unsigned)v[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                so[k] = make_uint4((unsigned)v[2 * k], (unsigned)(v[2 * k] >> 32), (unsigned)v[2 * k + 1],
                                   (unsigned)(v[2 * k + 1] >> 32));
        }
    }
    __syncthreads();
    uint4 *o = reinterpret_cast<uint4 *>(image + ((uint64_t)g * W + x0) * 3);
    const uint32_t n16 = nact * Q;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const uint32_t i = k * SLAB_BLOCK + threadIdx.x;
        if (i < n16) {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const uint4 w = s_out[i];
            __builtin_nontemporal_store(v4u{w.x, w.y, w.z, w.w}, reinterpret_cast<v4u *>(o + i));
        }
    }
}

// ---- integer frames: 48 bytes of an image row per thread ------------------------------------
// A thread of k_unpack_int decodes INT_BYTES / PB consecutive pixels (PB = 3 or 6 bytes per pixel:
// 16 pixels of u8, 8 of u16).  Its non-zero pixels are consecutive in the values array, so they are
// one run of at most 48 bytes: read with aligned dword loads whatever the values pointer's
// alignment, brought to byte 0 with a funnel shift, and expanded by the mask bits in registers.
constexpr int INT_BYTES = 48, INT_DW = INT_BYTES / 4;

// the dword at byte `sh` (0..3) of the pair hi:lo
__host__ __device__ inline uint32_t funnel(uint32_t hi, uint32_t lo, unsigned sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

// w: a run of packed PB-byte pixels from byte 0 (what follows the popc(bits) pixels of the run is
// never used); o: the 48 / PB pixels of the mask `bits` in place, zero where a bit is clear.  Pixel
// k takes the run's first pixel and, if its bit is set, the run moves down by one pixel; only the
// dwords that the pixels still to come can reach are moved.  Every index is a compile-time
// constant, so w and o stay in registers.
template <int PB>
__host__ __device__ inline void expand_run(uint32_t (&w)[INT_DW], unsigned bits, uint32_t (&o)[INT_DW]) {
    constexpr int G = INT_BYTES / PB;
#pragma unroll
    for (int i = 0; i < INT_DW; ++i) o[i] = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const bool take = (bits >> k) & 1u;
        const int d = k * PB / 4, s = k * PB % 4 * 8; // pixel k starts at bit s of o[d]
        if constexpr (PB == 3) {
            const uint32_t v = take ? (w[0] & 0xFFFFFFu) : 0u;
            o[d] |= v << s;
            if (s > 8) o[d + 1] |= v >> (32 - s);
        } else {
            const uint32_t lo = take ? w[0] : 0u, hi = take ? (w[1] & 0xFFFFu) : 0u;
            if (s == 0) {
                o[d] |= lo;
                o[d + 1] |= hi;
            } else { // s == 16
                o[d] |= lo << 16;
                o[d + 1] |= (lo >> 16) | (hi << 16);
            }
        }
        const int need = ((G - 1 - k) * PB + 3) / 4; // dwords the remaining pixels occupy
#pragma unroll
        for (int i = 0; i < need; ++i) {
            uint32_t moved;
            if constexpr (PB == 3)
                moved = funnel(i + 1 < INT_DW ? w[i + 1] : 0u, w[i], 3);
            else
                moved = funnel(i + 2 < INT_DW ? w[i + 2] : 0u, i + 1 < INT_DW ? w[i + 1] : 0u, 2);
            w[i] = take ? moved : w[i];
        }
    }
}

// One workgroup per (image row g, 256 threads' pixels: 4096 columns of u8, 2048 of u16).  The width
// is a multiple of the thread's pixel count G, so p is one and the thread's mask bits sit in one
// word (G divides 64).  The 48 bytes go through LDS to the frame as in k_unpack4: lane i of a store
// at 16 i bytes of the workgroup's contiguous stretch, non-temporal.
template <typename T>
__global__ __launch_bounds__(SLAB_BLOCK) void k_unpack_int(ShardPtrs sp, uint64_t mask_at, uint64_t px, uint32_t W,
                                                            uint32_t ncol, uint32_t rb, uint32_t ns,
                                                            T *__restrict__ image) {
    constexpr int PB = 3 * (int)sizeof(T), G = INT_BYTES / PB, Q = INT_BYTES / 16;
    __shared__ uint4 s_out[SLAB_BLOCK * Q];
    const uint32_t g = blockIdx.x / ncol, c = blockIdx.x - g * ncol;
    const uint32_t x0 = c * SLAB_BLOCK * G, x = x0 + threadIdx.x * G;
    const uint32_t nact = (W - x0 < SLAB_BLOCK * G ? W - x0 : SLAB_BLOCK * G) / G;
    if (x < W) {
        const uint32_t blk = g / rb, s = blk % ns;
        const uint64_t lr = (uint64_t)(blk / ns) * rb + (g - blk * rb);
        const uint64_t p = lr * W + x; // a multiple of G (W is)
        const unsigned char *h = sp.hdr[s];
        const uint32_t *off = reinterpret_cast<const uint32_t *>(h + HDR_OFFS);
        const uint64_t *mask = reinterpret_cast<const uint64_t *>(h + mask_at);
        const unsigned bits = (unsigned)(mask[p / 64] >> (p % 64)) & ((1u << G) - 1u);
        uint32_t o[INT_DW];
#pragma unroll
        for (int i = 0; i < INT_DW; ++i) o[i] = 0;
        if (bits) {
            const uint64_t r = rank_of(off, mask, p);
            const uint32_t n = (uint32_t)__popc(bits);
            if (r + n <= px) { // (a consistent header never ranks past the slab)
                // the run's bytes [a, a + n PB) lie inside the values buffer; every dword loaded is
                // an aligned one that holds at least one of them
                const uintptr_t a = reinterpret_cast<uintptr_t>(sp.vals[s]) + r * PB;
                const unsigned sh = (unsigned)(a & 3);
                const uint32_t *src = reinterpret_cast<const uint32_t *>(a - sh);
                const uint32_t ndw = (sh + n * PB + 3) / 4; // <= INT_DW + 1
                uint32_t cdw[INT_DW + 1];
#pragma unroll
                for (int i = 0; i <= INT_DW; ++i) cdw[i] = (uint32_t)i < ndw ? src[i] : 0u;
                uint32_t w[INT_DW];
#pragma unroll
                for (int i = 0; i < INT_DW; ++i) w[i] = funnel(cdw[i + 1], cdw[i], sh);
                expand_run<PB>(w, bits, o);
            }
        }
        uint4 *so = s_out + threadIdx.x * Q;
#pragma unroll
        for (int k = 0; k < Q; ++k) so[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
    __syncthreads();
    uint4 *out = reinterpret_cast<uint4 *>(image + ((uint64_t)g * W + x0) * 3);
    const uint32_t n16 = nact * Q;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const uint32_t i = k * SLAB_BLOCK + threadIdx.x;
        if (i < n16) {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const uint4 v = s_out[i];
            __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u *>(out + i));
        }
    }
}

bool args_ok(uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards, int precision) {
    if (width == 0 || height == 0 || row_block == 0 || nshards == 0 || nshards > RT_MAX_SHARDS) return false;
    return rt_format_ok(precision);
}

// an integer slab, values buffer or image is aligned to its sample (the float kernels leave their
// element alignment to the caller, as they always have)
bool int_aligned(const void *p, int precision) {
    return precision != RT_OUT_U16 || (reinterpret_cast<uintptr_t>(p) & 1) == 0;
}

// rt_slab_pack's three kernels on a slab of T, the unsigned integer of the format's element size
// (a float slab goes as bit patterns): one pixel per thread
template <typename T>
int pack(const void *d_slab, const Layout &l, uint64_t valid_px, unsigned char *h, void *d_values, hipStream_t st) {
    uint32_t *off = reinterpret_cast<uint32_t *>(h + HDR_OFFS);
    uint64_t *mask = reinterpret_cast<uint64_t *>(h + l.mask_at);
    const dim3 grid((unsigned)l.nblk), blk(SLAB_BLOCK);
    hipLaunchKernelGGL(k_mask<T>, grid, blk, 0, st, static_cast<const T *>(d_slab), valid_px, off, mask);
    SLABCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, off, l.nblk, reinterpret_cast<uint64_t *>(h));
    SLABCHK(hipGetLastError());
    hipLaunchKernelGGL(k_compact<T>, grid, blk, 0, st, static_cast<const T *>(d_slab), l.px, off, mask,
                       static_cast<T *>(d_values));
    SLABCHK(hipGetLastError());
    return RT_OK;
}

// rt_slab_unpack's choice between its three kernels.  The wide one of the format decodes G pixels
// per thread with 16-byte stores, when every image row starts on a multiple of 16 bytes and holds
// whole threads: a 16-byte aligned image whose width is a multiple of G.
//   float shards: k_unpack4, G = 4 pixels (48 or 96 bytes);
//   integer shards: k_unpack_int, 48 bytes per thread (G = 16 pixels of u8, 8 of u16).
// Any other image (a view into a larger buffer) takes the element-wise kernel, k_unpack.
template <typename T>
int unpack(const ShardPtrs &sp, const Layout &l, uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards,
           void *d_image, hipStream_t st) {
    constexpr bool INT = sizeof(T) < 4;
    constexpr uint32_t G = INT ? INT_BYTES / (3 * sizeof(T)) : UNPACK_PX;
    const bool wide = width % G == 0 && (reinterpret_cast<uintptr_t>(d_image) & 15) == 0;
    const uint32_t per_wg = wide ? SLAB_BLOCK * G : SLAB_BLOCK;
    const uint32_t ncol = (uint32_t)(((uint64_t)width + per_wg - 1) / per_wg);
    const uint64_t nblocks = (uint64_t)ncol * height;
    if (nblocks >= (1ull << 31)) return RT_ETOOBIG;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(SLAB_BLOCK), 0, st, sp, l.mask_at, l.px, width, ncol,
                           row_block, nshards, static_cast<T *>(d_image));
    };
    if (!wide)
        launch(k_unpack<T>);
    else if constexpr (INT)
        launch(k_unpack_int<T>);
    else
        launch(k_unpack4<T>);
    SLABCHK(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

size_t rt_slab_header_bytes(uint32_t width, uint32_t height, uint32_t row_block, uint32_t nshards) {
    if (width == 0 || row_block == 0 || nshards == 0) return 0;
    return (size_t)layout(width, rt_shard_rows(height, row_block, nshards)).bytes;
}

int rt_slab_pack(const void *d_slab, uint32_t width, uint32_t height, uint32_t row_block, uint32_t shard,
                 uint32_t nshards, int precision, void *d_header, void *d_values, void *stream) {
    if (!d_slab || !d_header || !d_values || !args_ok(width, height, row_block, nshards, precision) ||
        shard >= nshards || !int_aligned(d_slab, precision) || !int_aligned(d_values, precision))
        return RT_EBADARG;
    const Layout l = layout(width, rt_shard_rows(height, row_block, nshards));
    if (l.px >= (1ull << 32)) return RT_ETOOBIG;
    // the slab rows inside the image are a prefix of the slab (rt_shard.h)
    const uint64_t valid_px = (uint64_t)rt_shard_valid_rows(height, row_block, shard, nshards) * width;
    return with_format(precision, [&](auto fmt) {
        return pack<typename decltype(fmt)::bits>(d_slab, l, valid_px, static_cast<unsigned char *>(d_header), d_values,
                                                  reinterpret_cast<hipStream_t>(stream));
    });
}

int rt_slab_unpack(const void *const *d_headers, const void *const *d_values, uint32_t width, uint32_t height,
                   uint32_t row_block, uint32_t nshards, int precision, void *d_image, void *stream) {
    if (!d_headers || !d_values || !d_image || !args_ok(width, height, row_block, nshards, precision) ||
        !int_aligned(d_image, precision))
        return RT_EBADARG;
    const Layout l = layout(width, rt_shard_rows(height, row_block, nshards));
    if (l.px >= (1ull << 32)) return RT_ETOOBIG;
    ShardPtrs sp = {};
    for (uint32_t s = 0; s < nshards; ++s) {
        if (!d_headers[s] || !d_values[s] || !int_aligned(d_values[s], precision)) return RT_EBADARG;
        sp.hdr[s] = static_cast<const unsigned char *>(d_headers[s]);
        sp.vals[s] = d_values[s];
    }
    return with_format(precision, [&](auto fmt) {
        return unpack<typename decltype(fmt)::bits>(sp, l, width, height, row_block, nshards, d_image,
                                                    reinterpret_cast<hipStream_t>(stream));
    });
}

} // extern "C"
