// Host-only sanitizer driver for the scene compiler's table from compact object id to scene-list
// index (Compiled::elem_of in eraytracer_amd/csrc/rt_scene.h: what rt_launch_attrs' d_elem reports),
// built by tests/test_attrs.py with -fsanitize=address,undefined.  Each argument is a file of
// rt_elem records as the ctypes marshal lays them out.  Per file the table must be strictly
// increasing, name only sphere, triangle and plane elements, cover every one of them and have
// hdr.n_obj entries; it prints "n_elems n_obj" and the table, or a complaint and exits 1.
#include <cstdio>
#include <vector>

#include "../../eraytracer_amd/csrc/rt_scene.h"

static bool is_object(const rt_elem &e) {
    return e.kind == RT_SPHERE || e.kind == RT_TRIANGLE || e.kind == RT_PLANE;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        FILE *f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<rt_elem> e;
        rt_elem x;
        while (std::fread(&x, sizeof x, 1, f) == 1) e.push_back(x);
        std::fclose(f);
        const uint32_t n = (uint32_t)e.size();
        rtl::Compiled c{};
        if (rtl::compile_scene(e.data(), n, c) != RT_OK) {
            std::fprintf(stderr, "%s: does not compile\n", argv[i]);
            return 1;
        }
        const std::vector<int> &t = c.elem_of;
        size_t objects = 0;
        for (const rt_elem &el : e) objects += is_object(el);
        if (t.size() != objects || (size_t)c.hdr.n_obj != objects) {
            std::fprintf(stderr, "%s: %zu entries, n_obj %d, %zu objects in the list\n", argv[i], t.size(), c.hdr.n_obj,
                         objects);
            return 1;
        }
        for (size_t k = 0; k < t.size(); ++k) {
            if (t[k] < 1 || (uint32_t)t[k] >= n || !is_object(e[t[k]]) || (k > 0 && t[k] <= t[k - 1])) {
                std::fprintf(stderr, "%s: entry %zu = %d: not an object's index, or not above entry %zu\n", argv[i], k,
                             t[k], k - 1);
                return 1;
            }
        }
        // (strictly increasing, all objects, as many as there are: every object is named exactly once)
        std::printf("%u %d", n, c.hdr.n_obj);
        for (int v : t) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
