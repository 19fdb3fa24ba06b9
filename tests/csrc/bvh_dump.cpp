// Host-only dump of the compiled sphere BVH (eraytracer_amd/csrc/rt_scene.cpp), built by
// tests/bvh_ref.py with -fsanitize=address,undefined as tests/test_host.py builds scene_check.  The
// arguments are pairs "in out": `in` a file of rt_elem records exactly as the ctypes marshal lays them
// out, `out` the file written for it:
//     int32[8]   n_sph n_bvh bvh_depth bvh_ok cull_ok n_obj n_tri n_pl
//     double     hdr.ext
//     float[16]  per node (n_bvh of them), as the kernels read them: (lx0 lx1 ly0 ly1) (lz0 lz1 ux0 ux1)
//                (uy0 uy1 uz0 uz1) (link0 link1 id0 id1 as int32)
//     double[4]  per sphere (n_sph of them): cx cy cz r2, the rows scan_bvh's leaf test reads
//     int32      per compact object id (n_obj of them): elem_of
// A scene that does not compile, or compiles without a BVH, gets the header and ext only (n_bvh = 0).
// RT_BVH_MIN in the environment is honoured as the library honours it.
#include <cstdio>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_scene.h"

int main(int argc, char **argv) {
    if (argc < 3 || argc % 2 != 1) return 2;
    for (int i = 1; i + 1 < argc; i += 2) {
        FILE *f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<rt_elem> e;
        rt_elem x;
        while (std::fread(&x, sizeof x, 1, f) == 1) e.push_back(x);
        std::fclose(f);
        const uint32_t n = (uint32_t)e.size();
        rtl::Compiled c{};
        const int rc = rtl::check_scene(e.data(), n) == RT_OK ? rtl::compile_scene(e.data(), n, c) : -1;
        const rtl::SceneHdr &h = c.hdr;
        const bool bvh = rc == RT_OK && h.bvh_ok;
        const int head[8] = {rc == RT_OK ? h.n_sph : 0, bvh ? h.n_bvh : 0, bvh ? h.bvh_depth : 0, bvh ? 1 : 0,
                             rc == RT_OK ? h.cull_ok : 0, rc == RT_OK ? h.n_obj : 0, rc == RT_OK ? h.n_tri : 0,
                             rc == RT_OK ? h.n_pl : 0};
        const double ext = rc == RT_OK ? h.ext : 0.0;
        FILE *o = std::fopen(argv[i + 1], "wb");
        if (!o) return 2;
        bool ok = std::fwrite(head, sizeof head, 1, o) == 1 && std::fwrite(&ext, sizeof ext, 1, o) == 1;
        if (bvh) {
            const size_t nb = (size_t)h.n_bvh * rtl::BVH_NODE_DOUBLES, ns = (size_t)h.n_sph * rtl::SPH_W;
            if ((size_t)h.o_bvh + nb > c.tab.size() || (size_t)h.o_sph + ns > c.tab.size() ||
                c.elem_of.size() != (size_t)h.n_obj)
                return 3;
            ok = ok && std::fwrite(c.tab.data() + h.o_bvh, 8, nb, o) == nb;
            ok = ok && std::fwrite(c.tab.data() + h.o_sph, 8, ns, o) == ns;
            ok = ok && std::fwrite(c.elem_of.data(), 4, c.elem_of.size(), o) == c.elem_of.size();
        }
        if (std::fclose(o) != 0 || !ok) return 4;
        std::printf("%d %d %d %d %d %.17g\n", rc, head[0], head[1], head[2], head[3], ext);
    }
    return 0;
}
