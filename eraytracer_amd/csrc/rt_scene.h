// rt_scene.h — host-side scene compiler interface (see rt_scene.cpp).
#pragma once
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"

namespace rtl {

struct Compiled {
    SceneHdr hdr;
    std::vector<double> tab; // double table (offsets in hdr.o_*)
    std::vector<int> itab;   // int table (offsets in hdr.i_*)
    // compact object id -> the object's index in the scene list (rt_launch_attrs' d_elem): strictly
    // increasing, the spheres, triangles and planes of the list and nothing else
    std::vector<int> elem_of;
    // scene list index -> the index of the element's canonical (first exactly equal) element, -1 for
    // an element that is not an object (rt_query_shadow's "same term" test): one entry per element
    std::vector<int> canon_of;
};

int check_scene(const rt_elem *e, uint32_t n);
int fill_canon(rt_elem *e, uint32_t n);
int compile_scene(const rt_elem *e, uint32_t n, Compiled &out);

} // namespace rtl
