// plist_check.cpp — rt_plist.h for one geometry: plist_check W SLAB_ROWS N_CHUNK FLAGS, FLAGS one
// character ('0' or '1') per half-tile in k_pmask's numbering (2 * tile + half).  Prints the layout
// (tiles_x tile_rows nhalf flags_off rowoff_off list_off bytes), the row offsets and the list's
// (x, y) words, one line each.  The list is built inside a buffer of exactly the layout's size, so the
// host sanitizers see any entry that falls outside its region.  Run by tests/test_primary_list.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_plist.h"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int W = std::atoi(argv[1]), rows = std::atoi(argv[2]), n_chunk = std::atoi(argv[3]);
    const rt_pmask_layout l = rt_pmask_layout_of(W, rows, n_chunk, 16);
    if (std::strlen(argv[4]) != l.nhalf) return 3;
    std::vector<unsigned long long> buf((l.bytes + 7) / 8); // (8-byte aligned, as a device allocation is)
    if (l.bytes % 8 != 0 || l.rowoff_off % 8 != 0 || l.list_off % 8 != 0) return 4;
    unsigned char *const base = reinterpret_cast<unsigned char *>(buf.data());
    unsigned char *const flags = base + l.flags_off;
    for (size_t i = 0; i < l.nhalf; ++i) flags[i] = argv[4][i] == '1';
    int *const rowoff = reinterpret_cast<int *>(base + l.rowoff_off);
    uint32_t *const list = reinterpret_cast<uint32_t *>(base + l.list_off);
    const int n = rt_pmask_list_of(flags, l.tiles_x, l.tile_rows, rowoff, list);
    std::printf("%d %d %zu %zu %zu %zu %zu\n", l.tiles_x, l.tile_rows, l.nhalf, l.flags_off, l.rowoff_off, l.list_off, l.bytes);
    for (int r = 0; r <= l.tile_rows; ++r) std::printf("%d ", rowoff[r]);
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%u %u ", list[2 * i], list[2 * i + 1]);
    std::printf("\n");
    for (size_t i = 0; i < l.nhalf; ++i) // building the list left the flags alone
        if (flags[i] != (argv[4][i] == '1')) return 5;
    return 0;
}
