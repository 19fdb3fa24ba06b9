// rt_bands.h — how rt_render cuts a frame into shards per device and row bands, for host code (no
// HIP needed; tests/csrc/band_check.cpp sweeps it under the host sanitizers).  Shard s of nshards
// renders on device s % ndev; every shard's slab (rt_shard.h) is rendered and copied to the host
// in nb bands of `band` rows; a context holds MAX_BANDS events for the bands of all its shards.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_mi355x.h"
#include "rt_shard.h"

constexpr int MAX_BANDS = 64; // a context's band events (rt_ctx::band, rt_ctx::copied)
static_assert(RT_MAX_SHARDS <= MAX_BANDS, "a device may get every shard, and each has at least one band");

inline uint32_t lcm_u(uint32_t a, uint32_t b) {
    uint32_t x = a, y = b;
    while (y) {
        const uint32_t t = x % y;
        x = y;
        y = t;
    }
    return a / x * b;
}

struct rt_bands {
    uint32_t nshards, ndev; // ndev: the devices used, min(nshards, devices given)
    uint32_t slab;          // rows of every shard's slab
    uint32_t per_dev;       // shards of the device that has most
    uint32_t band, nb;      // rows per band, bands per slab: band b is slab rows [row0(b), row1(b))
    uint32_t row0(uint32_t b) const { return b * band; }
    uint32_t row1(uint32_t b) const { return slab - row0(b) < band ? slab : row0(b) + band; }
    uint32_t shards_of(uint32_t d) const { return (nshards - d + ndev - 1) / ndev; } // shards d, d + ndev, ...
    // the event of band b of a device's i-th shard; < MAX_BANDS (rt_band_plan)
    uint32_t event(uint32_t i, uint32_t b) const { return i * nb + b; }
};

// The plan for a window of `height` rows in blocks of row_block rows, 1 <= nshards <= RT_MAX_SHARDS
// over 1 <= ndev <= nshards devices, rows of rowbytes > 0 bytes on their way to the host.
// Bands: whole row blocks and whole 16-row tiles, about band_bytes of output each, at most
// MAX_BANDS per device over all of its shards.  That is the one place the events' index is
// bounded: i < shards_of(d) <= per_dev <= RT_MAX_SHARDS <= MAX_BANDS, so max_nb >= 1, and
// b < nb <= max_nb = MAX_BANDS / per_dev, so event(i, b) < per_dev * nb <= MAX_BANDS.
inline rt_bands rt_band_plan(uint32_t height, uint32_t row_block, uint32_t nshards, uint32_t ndev, uint32_t rowbytes,
                             size_t band_bytes) {
    rt_bands p;
    p.nshards = nshards;
    p.ndev = ndev;
    p.slab = rt_shard_slab_rows(height, row_block, nshards);
    p.per_dev = (nshards + ndev - 1) / ndev;
    const uint32_t max_nb = MAX_BANDS / p.per_dev;
    const uint32_t gran = lcm_u(row_block, 16);
    const size_t rows = band_bytes / rowbytes;
    p.band = (uint32_t)(rows > 1 ? rows : 1) / gran * gran;
    if (p.band < gran) p.band = gran;
    if ((p.slab + p.band - 1) / p.band > max_nb) p.band = ((p.slab + max_nb - 1) / max_nb + gran - 1) / gran * gran;
    p.nb = (p.slab + p.band - 1) / p.band;
    return p;
}
