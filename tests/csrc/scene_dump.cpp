// scene_dump.cpp — everything the scene compiler (eraytracer_amd/csrc/rt_scene.cpp) produces, as
// bytes: scene_dump OUTDIR FILE...  Each FILE holds rt_elem records exactly as the ctypes marshal
// lays them out (as for scene_check.cpp); per file it writes OUTDIR/<file's base name>.dump and
// prints "<base name> <compile_scene's host wall-clock milliseconds>".  A dump is a sequence of
// sections, each "name byte-count\n" followed by that many bytes: rc (check, canon, compile as three
// ints), then, when the scene compiled, hdr (sizeof(SceneHdr) bytes), tab, itab, elem_of, canon_of.
// scripts/scene_compile_diff.py builds it against two trees and compares the dumps.
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "rt_scene.h" // -I <a tree's eraytracer_amd/csrc>: the tree under test, not necessarily this one

static void section(FILE *f, const char *name, const void *p, size_t bytes) {
    std::fprintf(f, "%s %zu\n", name, bytes);
    if (bytes) std::fwrite(p, 1, bytes, f);
}
template <typename T>
static void section(FILE *f, const char *name, const std::vector<T> &v) {
    section(f, name, v.data(), v.size() * sizeof(T));
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string outdir = argv[1];
    for (int i = 2; i < argc; ++i) {
        FILE *f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<rt_elem> e;
        rt_elem x;
        while (std::fread(&x, sizeof x, 1, f) == 1) e.push_back(x);
        std::fclose(f);
        const uint32_t n = (uint32_t)e.size();
        const std::vector<rt_elem> as_given = e; // compile_scene gets the list before fill_canon, as rt_prepare's callers may
        int rc[3];
        rc[0] = rtl::check_scene(e.data(), n);
        rc[1] = rtl::fill_canon(e.data(), n);
        rtl::Compiled c{};
        const auto t0 = std::chrono::steady_clock::now();
        rc[2] = rtl::compile_scene(as_given.data(), n, c);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::string base = argv[i];
        base = base.substr(base.find_last_of('/') + 1);
        FILE *o = std::fopen((outdir + "/" + base + ".dump").c_str(), "wb");
        if (!o) return 2;
        section(o, "rc", rc, sizeof rc);
        if (rc[2] == RT_OK) {
            section(o, "hdr", &c.hdr, sizeof c.hdr);
            section(o, "tab", c.tab);
            section(o, "itab", c.itab);
            section(o, "elem_of", c.elem_of);
            section(o, "canon_of", c.canon_of);
        }
        if (std::fclose(o) != 0) return 2;
        std::printf("%s %.3f\n", base.c_str(), ms);
    }
    return 0;
}
