// rt_query.inc — what the ray-query units share (rt_query.hip: nearest hits and shadow tests;
// rt_trace.hip: traced colours), included inside their anonymous namespaces after rt_math.inc: the
// names of the nearest-object scans and the test that admits a ray to the BVH walk.

enum { SCAN_BRUTE = 0, SCAN_BEAM = 1, SCAN_BVH = 2 };

// The BVH's domain (see the top of rt_query.hip); E = hdr.ext + 1.
__device__ __forceinline__ bool bvh_domain(const D3 &o, const D3 &d, double E) {
    const double lim = 4.0 * E, dd = d.x * d.x + d.y * d.y + d.z * d.z;
    return fabs(o.x) <= lim && fabs(o.y) <= lim && fabs(o.z) <= lim && fabs(dd - 1.0) <= 0x1p-20;
}
