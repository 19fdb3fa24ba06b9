// rt_plist.h — where the primary rays' candidate masks, the half-tiles' empty flags and the list of
// active tiles live in one buffer, for host code (no HIP needed).
//
// A slab of slab_rows rows of W pixels is cut into tile x tile pixel tiles, tiles_x per tile row, each
// of two half-tiles (8 x 16 pixel blocks, numbered 2 * tile + half).  k_pmask writes, per half-tile,
// n_chunk 64-bit candidate masks and one flag byte (1: every mask zero), and from the flags the list of
// the active tiles — those with a half whose flag is 0 — in tile-row order:
//   rowoff[r]   active tiles in the tile rows before r (r = 0 .. tile_rows: tile_rows + 1 ints)
//   list[i]     8 bytes per active tile: x = tile column | flag of half 0 << 30 | flag of half 1 << 31,
//               y = tile row; the tiles of tile row r are list[rowoff[r] .. rowoff[r + 1])
// so that the active tiles of any range of tile rows are one range of the list.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct rt_pmask_layout {
    int tiles_x, tile_rows;
    size_t nhalf;      // half-tiles of the slab
    size_t flags_off;  // bytes from the buffer's start: after the masks
    size_t rowoff_off; // 8-byte aligned
    size_t list_off;   // 8-byte aligned; room for every tile of the slab
    size_t bytes;      // the buffer's size
};

inline rt_pmask_layout rt_pmask_layout_of(int W, int slab_rows, int n_chunk, int tile) {
    rt_pmask_layout l;
    l.tiles_x = (W + tile - 1) / tile;
    l.tile_rows = (slab_rows + tile - 1) / tile;
    l.nhalf = (size_t)l.tiles_x * (size_t)l.tile_rows * 2;
    l.flags_off = l.nhalf * (size_t)n_chunk * 8;
    l.rowoff_off = (l.flags_off + l.nhalf + 7) / 8 * 8;
    l.list_off = l.rowoff_off + ((size_t)l.tile_rows + 2) / 2 * 8;
    l.bytes = l.list_off + l.nhalf / 2 * 8;
    return l;
}

// The list by its definition, from the flag bytes (flags[2 * tile + half]): what k_pmask's list
// phases leave in rowoff and list (x, y pairs).  Returns the number of active tiles.
inline int rt_pmask_list_of(const unsigned char *flags, int tiles_x, int tile_rows, int *rowoff, uint32_t *list) {
    int n = 0;
    for (int r = 0; r < tile_rows; ++r) {
        rowoff[r] = n;
        for (int c = 0; c < tiles_x; ++c) {
            const unsigned f0 = flags[2 * ((size_t)r * tiles_x + c)], f1 = flags[2 * ((size_t)r * tiles_x + c) + 1];
            if (f0 && f1) continue;
            list[2 * (size_t)n] = (uint32_t)c | (f0 ? 1u : 0u) << 30 | (f1 ? 1u : 0u) << 31;
            list[2 * (size_t)n + 1] = (uint32_t)r;
            ++n;
        }
    }
    rowoff[tile_rows] = n;
    return n;
}
