// rt_planes.inc — the five hit-attribute planes of rt_attr_planes (RT_ATTRIBUTES in
// include/rt_mi355x.h): what a nearest hit means (hit_attrs) and how it is stored (put_hit), for
// rt_attrs.hip's primary rays and rt_query.hip's rays alike.  Included after rt_primary.inc; the
// planes themselves are HitPlanes (rt_internal.h, filled by rt_hit_planes).

template <int PREC>
__device__ __forceinline__ void put1(void *plane, size_t i, double v) {
    if (PREC == RT_OUT_F64)
        reinterpret_cast<double *>(plane)[i] = v;
    else
        reinterpret_cast<float *>(plane)[i] = (float)v;
}
template <int PREC>
__device__ __forceinline__ void put3(void *plane, size_t i, const D3 &c) {
    if (PREC == RT_OUT_F64) {
        double *o = reinterpret_cast<double *>(plane) + i * 3;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    } else {
        float *o = reinterpret_cast<float *>(plane) + i * 3;
        o[0] = (float)c.x; o[1] = (float)c.y; o[2] = (float)c.z;
    }
}

struct HitAttrs {
    D3 point, normal, albedo;
    int elem;
};

// The attributes of the hit at distance t of the ray o + d t on object id (id < 0: no hit).  Called
// by converged waves (hit_normal's normalize3 ballots), so a lane without a hit goes through the
// geometry of object 0, unstored; any_hit: some lane of the wave has a hit (wave-uniform; then the
// scene has an object: row 0 exists).  want_geom (wave-uniform): the point or the normal is wanted.
__device__ __forceinline__ HitAttrs hit_attrs(const Scene &S, const int *__restrict__ elem_of, const D3 &o, const D3 &d,
                                              int id, double t, bool any_hit, bool want_geom) {
    const int row = id >= 0 ? id : 0;
    HitAttrs a = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, -1};
    if (any_hit) {
        if (want_geom) {
            // Intersection = Origin + Direction*t (:384-387 and its kin), the normal of that hit record
            a.point = D3{o.x + d.x * t, o.y + d.y * t, o.z + d.z * t};
            a.normal = hit_normal<0>(S, row, a.point);
        }
        const double *m = obj_row<0>(S, row);
        a.albedo = D3{m[3], m[4], m[5]}; // #material.colour
        a.elem = elem_of[row];
    }
    return a;
}

// Entry i of the planes asked for (wave-uniform, from the kernel's arguments): a miss is -1, +inf
// and zeros.
template <int PREC>
__device__ __forceinline__ void put_hit(const HitPlanes &pl, size_t i, int id, double t, const HitAttrs &a) {
    const bool hit = id >= 0;
    const D3 zero = {0.0, 0.0, 0.0};
    if (pl.elem) pl.elem[i] = hit ? a.elem : -1;
    if (pl.t) put1<PREC>(pl.t, i, hit ? t : __builtin_inf());
    if (pl.point) put3<PREC>(pl.point, i, hit ? a.point : zero);
    if (pl.normal) put3<PREC>(pl.normal, i, hit ? a.normal : zero);
    if (pl.albedo) put3<PREC>(pl.albedo, i, hit ? a.albedo : zero);
}
