// rt_shard.h — the row interleave of the shards of a frame, for host code (no HIP needed).
//
// A frame of H rows is cut into blocks of rb rows; block b belongs to shard b % ns, and a shard
// keeps its blocks in order in a slab of rt_shard_slab_rows rows (every shard's slab has the same
// size, so the last block or two of a slab may lie past the image).  Image rows grow with slab
// rows, so the slab rows inside the image are a prefix of the slab: rows [0, rt_shard_valid_rows).
// Every host-side copy, scatter and count goes through these three functions; the kernels do the
// same arithmetic on the device.  rb and ns are not zero.
#pragma once
#include <stdint.h>

struct rt_shard_map { // one shard of a frame of `height` rows
    uint32_t height, row_block, shard, nshards;
};

// rows of every shard's slab (what the exported rt_shard_rows returns for valid arguments)
inline uint32_t rt_shard_slab_rows(uint32_t H, uint32_t rb, uint32_t ns) {
    const uint64_t span = (uint64_t)rb * ns;
    return (uint32_t)((H + span - 1) / span * rb);
}

// the image row of slab row r of shard `shard` (may be >= H: a slab row past the image)
inline uint64_t rt_shard_image_row(uint64_t r, uint32_t rb, uint32_t shard, uint32_t ns) {
    return (r / rb * ns + shard) * rb + r % rb;
}

// slab rows of shard `shard` inside an image of H rows
inline uint32_t rt_shard_valid_rows(uint32_t H, uint32_t rb, uint32_t shard, uint32_t ns) {
    const uint64_t start = (uint64_t)shard * rb, period = (uint64_t)ns * rb;
    if (H <= start) return 0;
    const uint64_t full = (H - start) / period, rem = (H - start) % period;
    return (uint32_t)(full * rb + (rem < rb ? rem : rb));
}

inline uint64_t rt_shard_image_row(const rt_shard_map &m, uint64_t r) {
    return rt_shard_image_row(r, m.row_block, m.shard, m.nshards);
}
inline uint32_t rt_shard_valid_rows(const rt_shard_map &m) {
    return rt_shard_valid_rows(m.height, m.row_block, m.shard, m.nshards);
}
