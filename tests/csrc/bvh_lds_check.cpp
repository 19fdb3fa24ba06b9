// bvh_lds_check.cpp — rt_layout.h's bvh_lds_place for one launch: bvh_lds_check N_BVH N_SPH BVH_DEPTH
// BASE BLOCK prints "l_bvh l_bsph l_stack total".  Every other field of the header is zero: the
// placement may read only the three it is given.  Built with the host sanitizers and run by
// tests/test_bvh_lds.py.
#include <cstdio>
#include <cstdlib>

#include "../../eraytracer_amd/csrc/rt_layout.h"

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    rtl::SceneHdr h = {};
    h.n_bvh = std::atoi(argv[1]);
    h.n_sph = std::atoi(argv[2]);
    h.bvh_depth = std::atoi(argv[3]);
    h.l_bvh = h.l_bsph = h.l_stack = -7; // (all three are set, whatever they were)
    const size_t total = rtl::bvh_lds_place(h, (size_t)std::atoll(argv[4]), std::atoi(argv[5]));
    std::printf("%d %d %d %zu\n", h.l_bvh, h.l_bsph, h.l_stack, total);
    return 0;
}
