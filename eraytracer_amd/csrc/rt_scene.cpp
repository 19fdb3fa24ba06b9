// rt_scene.cpp — host-side scene compiler: validates an rt_elem list (the marshalled
// reference scene, raytracer.erl:618-665) and lays it out for the kernel (rt_layout.h).
//
// Every precomputed quantity is produced with the reference's operation order, in IEEE
// binary64, compiled with -ffp-contract=off, so the kernel sees bit-identical values to
// those the reference computes per ray.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_layout.h"
#include "rt_scene.h"

namespace rtl {

static bool finite3(const rt_vec3 &v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }
static bool finite_mat(const rt_material &m) {
    return finite3(m.colour) && std::isfinite(m.specular_power) && std::isfinite(m.shininess) &&
           std::isfinite(m.reflectivity);
}

static bool elem_ok(const rt_elem &e) {
    switch (e.kind) {
    case RT_CAMERA:
        return finite3(e.u.camera.location) && finite3(e.u.camera.rotation) && std::isfinite(e.u.camera.fov) &&
               std::isfinite(e.u.camera.screen_width) && std::isfinite(e.u.camera.screen_height);
    case RT_POINT_LIGHT:
        return finite3(e.u.point_light.diffuse_colour) && finite3(e.u.point_light.location) &&
               finite3(e.u.point_light.specular_colour);
    case RT_SPHERE:
        return std::isfinite(e.u.sphere.radius) && finite3(e.u.sphere.center) && finite_mat(e.u.sphere.material);
    case RT_TRIANGLE:
        return finite3(e.u.triangle.v1) && finite3(e.u.triangle.v2) && finite3(e.u.triangle.v3) &&
               finite_mat(e.u.triangle.material);
    case RT_PLANE:
        return finite3(e.u.plane.normal) && std::isfinite(e.u.plane.distance) && finite_mat(e.u.plane.material);
    case RT_OTHER:
        return true;
    default:
        return false;
    }
}

static size_t payload_bytes(int kind) {
    switch (kind) {
    case RT_CAMERA: return sizeof(((rt_elem *)0)->u.camera);
    case RT_POINT_LIGHT: return sizeof(((rt_elem *)0)->u.point_light);
    case RT_SPHERE: return sizeof(((rt_elem *)0)->u.sphere);
    case RT_TRIANGLE: return sizeof(((rt_elem *)0)->u.triangle);
    case RT_PLANE: return sizeof(((rt_elem *)0)->u.plane);
    default: return 0;
    }
}

// No count limits: the reference's scans take any list (nearest_object_intersecting_ray/6,
// raytracer.erl:300-346; lighting_function/6 folds over every light, :209-252).  What does not
// fit the device (or the 32-bit table offsets) fails with RT_ENOMEM in compile_scene.
int check_scene(const rt_elem *e, uint32_t n) {
    if (!e || n < 1) return RT_EBADARG;         // [Camera|Rest] must match (raytracer.erl:180)
    if (e[0].kind != RT_CAMERA) return RT_EBADARG; // Camera#camera.location would crash (:488)
    if (n > (uint32_t)INT32_MAX / 2) return RT_ENOMEM; // object ids are 32-bit ints in the kernels
    for (uint32_t i = 0; i < n; i++) {
        if (!elem_ok(e[i])) return RT_EBADARG;
        if (e[i].canon < -1 || e[i].canon > (int32_t)i) return RT_EBADARG;
        if (e[i].canon >= 0 && e[e[i].canon].kind != e[i].kind) return RT_EBADARG;
    }
    return RT_OK;
}

// canon[i] = the first j <= i of the same kind that is its own canonical element and has the same
// payload bytes.  One hash lookup per element (the elements so far that are their own canonical
// element, keyed by kind and payload; the first one of each key kept), not a scan of the prefix.
int fill_canon(rt_elem *e, uint32_t n) {
    if (!e) return RT_EBADARG;
    struct Key {
        const rt_elem *p;
        size_t nb;
    };
    auto hash = [](const rt_elem *p, size_t nb) {
        uint64_t h = 1469598103934665603ull ^ (uint64_t)(uint32_t)p->kind;
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&p->u);
        for (size_t k = 0; k < nb; ++k) h = (h ^ b[k]) * 1099511628211ull;
        return h;
    };
    // open addressing over indices (-1 = empty); 2x the element count, a power of two
    size_t cap = 16;
    while (cap < 2 * (size_t)n) cap <<= 1;
    std::vector<int32_t> slot(cap, -1);
    auto find_or_add = [&](uint32_t i, bool add) -> int32_t {
        const size_t nb = payload_bytes(e[i].kind);
        size_t s = hash(&e[i], nb) & (cap - 1);
        for (;; s = (s + 1) & (cap - 1)) {
            const int32_t j = slot[s];
            if (j < 0) {
                if (add) slot[s] = (int32_t)i;
                return -1;
            }
            if (e[j].kind == e[i].kind && std::memcmp(&e[j].u, &e[i].u, nb) == 0) return j;
        }
    };
    for (uint32_t i = 0; i < n; i++) {
        const bool has = payload_bytes(e[i].kind) != 0; // RT_OTHER terms are never matched
        if (e[i].canon < 0) {
            const int32_t j = has ? find_or_add(i, false) : -1;
            e[i].canon = j >= 0 ? j : (int32_t)i;
        }
        if (has && e[i].canon == (int32_t)i) (void)find_or_add(i, true); // keeps the first of its key
    }
    return RT_OK;
}

// resolve canon chains to the first element of each equality class
static int root(const std::vector<rt_elem> &e, int i) {
    while (e[i].canon >= 0 && e[i].canon != i) i = e[i].canon;
    return i;
}

// binary32 bounds that contain the binary64 value: rounded down (lo) or up (hi)
static float f32_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, -INFINITY);
    return f;
}
static float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafterf(f, INFINITY);
    return f;
}

// The three environment knobs, read once per process (by the first scene that is compiled).
struct Knobs {
    int bvh_min;   // RT_BVH_MIN: fewer spheres, no BVH (the wave beams are cheaper; BVH_MIN_SPHERES)
    int bvh_level; // RT_BVH_LEVEL: first reflection level that walks the BVH (BVH_LEVEL; level 1,
                   // coherent rays from the primary hits, keeps the beams); below 1 counts as 1
    int beam_min;  // RT_BEAM_MIN: fewer spheres, no wave beams (BEAM_MIN_SPHERES; for A/B runs)
};
static const Knobs &knobs() {
    static const Knobs k = [] {
        auto env = [](const char *name, int dflt) {
            const char *s = std::getenv(name);
            return s ? std::atoi(s) : dflt;
        };
        return Knobs{env("RT_BVH_MIN", BVH_MIN_SPHERES), env("RT_BVH_LEVEL", BVH_LEVEL),
                     env("RT_BEAM_MIN", BEAM_MIN_SPHERES)};
    }();
    return k;
}

// The compile in progress: compile_scene's stages, below, read and extend it in order.
struct Build {
    std::vector<rt_elem> e;                      // the list, canon filled in
    std::vector<int> compact;                    // list index -> compact object id (-1: not an object)
    std::vector<int> objs, lights, sph, tri, pl; // list indices; sph / tri / pl in table order
    std::vector<rt_vec3> org;                    // slot 0 = camera location, slot 1+i = light i location
    Compiled &out;
    SceneHdr &h;
    std::vector<double> &t;
    std::vector<int> &it;
    Build(const rt_elem *in, uint32_t n, Compiled &o)
        : e(in, in + n), compact(n, -1), out(o), h(o.hdr), t(o.tab), it(o.itab) {}
    const decltype(rt_elem::u.sphere) &sphere(int k) const { return e[sph[k]].u.sphere; } // by table index
    const rt_vec3 &light(int i) const { return e[lights[i]].u.point_light.location; }
};

// A sphere's cone of directions as seen from an origin, with margins on the safe side: v = c - o,
// r = |radius|.  vl = |v|; sr >= sin(rho) and cr <= cos(rho) for the cone's half-angle rho; near:
// the origin is inside the sphere or so close that the cone is everything (sr = 1 or above, cr = 0);
// dlow <= |v| - r, the distance before which no ray from o reaches the sphere.  One function for
// the binary64 and binary32 cull rows and for the occluder masks' targets and candidates, which
// once spelled it four ways: `near ? 1 : ..` against `sr >= 1 ? 0 : ..` (near, once sr >= 1 is
// folded into it, says both), and `!(vl > x)` against `vl <= x` (the same, as vl is never NaN: it
// is the square root of a sum of squares of differences of finite inputs, +inf at worst).
struct Cone {
    double vl, sr, cr, dlow;
    bool near;
};
static Cone cone_of(double vx, double vy, double vz, double r, double eps) {
    Cone c;
    c.vl = std::sqrt(vx * vx + vy * vy + vz * vz);
    c.near = c.vl <= r * (1 + eps) + eps;
    c.sr = c.near ? 1.0 : r / c.vl * (1 + eps) + eps;
    if (c.sr >= 1.0) c.near = true;
    c.cr = c.near ? 0.0 : std::sqrt(1 - c.sr * c.sr) - eps;
    c.dlow = (c.vl - r) - eps * (c.vl + r) - eps;
    return c;
}

// Compact ids (list order: [Camera|Rest], :180; non-objects are skipped, :357), the lights (:248),
// the objects by type, the header's counts and the origins.
static int classify(Build &b, uint32_t n) {
    for (uint32_t i = 1; i < n; i++) {
        int k = b.e[i].kind;
        if (k == RT_SPHERE || k == RT_TRIANGLE || k == RT_PLANE) {
            b.compact[i] = (int)b.objs.size();
            b.objs.push_back((int)i);
        } else if (k == RT_POINT_LIGHT) {
            b.lights.push_back((int)i);
        }
    }
    // The per-origin tables (camera and every light) hold ~16 doubles per (origin, sphere) pair: a
    // scene whose tables would not fit 32-bit offsets is refused before they are built.
    const double per_origin = 16.0 * (double)b.objs.size();
    if ((double)(1 + b.lights.size()) * per_origin + 32.0 * (double)b.objs.size() >= (double)INT32_MAX / 2)
        return RT_ENOMEM;
    for (int i : b.objs) {
        if (b.e[i].kind == RT_SPHERE) b.sph.push_back(i);
        else if (b.e[i].kind == RT_TRIANGLE) b.tri.push_back(i);
        else b.pl.push_back(i);
    }
    SceneHdr &h = b.h;
    std::memset(&h, 0, sizeof(h));
    h.n_sph = (int)b.sph.size();
    h.n_tri = (int)b.tri.size();
    h.n_pl = (int)b.pl.size();
    h.n_obj = (int)b.objs.size();
    h.n_light = (int)b.lights.size();
    h.n_org = 1 + h.n_light;
    b.out.elem_of = b.objs; // compact ids follow list order
    b.out.canon_of.assign(n, -1);
    for (int i : b.objs) b.out.canon_of[i] = root(b.e, i);
    b.org.push_back(b.e[0].u.camera.location);
    for (int li : b.lights) b.org.push_back(b.e[li].u.point_light.location);
    b.t.clear();
    b.it.clear();
    return RT_OK;
}

// The spheres' table order (their local index) decides only the order candidates and occluders
// are visited in — nearest hits are broken by list position (compact id), shadow answers are
// any-hit — so the spheres that cover most of the lights' view go first: a shadow ray's
// occluder walk meets the likelier blockers early and its lane leaves sooner (measured against
// list order: config 5 -4.5 % per frame, config 3 -1 %; ordering by radius alone: -3 %, and +1 %
// on config 3).
static void order_spheres(Build &b) {
    // the spheres' solid angle summed over the lights (their radius when there are none)
    std::vector<double> w(b.e.size(), 0.0);
    for (int i : b.sph) {
        const auto &sp = b.e[i].u.sphere;
        const double r2 = sp.radius * sp.radius;
        double a = b.lights.empty() ? r2 : 0.0;
        for (int li : b.lights) {
            const rt_vec3 &L = b.e[li].u.point_light.location;
            const double dx = sp.center.x - L.x, dy = sp.center.y - L.y, dz = sp.center.z - L.z;
            a += r2 / std::fmax(dx * dx + dy * dy + dz * dz, 1e-300);
        }
        w[i] = a;
    }
    std::stable_sort(b.sph.begin(), b.sph.end(), [&](int p, int q) { return w[p] > w[q]; });
}

// Spheres (ray_sphere_intersect/2, :364-397), triangles (ray_triangle_intersect/2, :402-455) and
// planes (ray_plane_intersect/2, :461-480), each with its rows per origin.
static void primitive_tables(Build &b) {
    SceneHdr &h = b.h;
    std::vector<double> &t = b.t;
    h.o_sph = (int)t.size();
    for (int i : b.sph) {
        const auto &s = b.e[i].u.sphere;
        double r = s.radius;
        t.insert(t.end(), {s.center.x, s.center.y, s.center.z, r * r});
    }
    h.o_sph_org = (int)t.size();
    for (const rt_vec3 &o : b.org) {
        for (int i : b.sph) {
            const auto &s = b.e[i].u.sphere;
            double X0 = o.x, Y0 = o.y, Z0 = o.z, Xc = s.center.x, Yc = s.center.y, Zc = s.center.z;
            double r = s.radius;
            double C = (X0 - Xc) * (X0 - Xc) + (Y0 - Yc) * (Y0 - Yc) + (Z0 - Zc) * (Z0 - Zc) - r * r;
            t.insert(t.end(), {X0 - Xc, Y0 - Yc, Z0 - Zc, C});
        }
    }
    h.o_tri = (int)t.size();
    std::vector<rt_vec3> edge1; // Edge1 (:406), once for the triangle's row and its rows per origin
    for (int i : b.tri) {
        const auto &tr = b.e[i].u.triangle;
        const rt_vec3 e1 = {tr.v2.x - tr.v1.x, tr.v2.y - tr.v1.y, tr.v2.z - tr.v1.z};
        double e2x = tr.v3.x - tr.v1.x, e2y = tr.v3.y - tr.v1.y, e2z = tr.v3.z - tr.v1.z;
        t.insert(t.end(), {tr.v1.x, tr.v1.y, tr.v1.z, e1.x, e1.y, e1.z, e2x, e2y, e2z, 0, 0, 0});
        edge1.push_back(e1);
    }
    h.o_tri_org = (int)t.size();
    for (const rt_vec3 &o : b.org) {
        for (size_t k = 0; k < b.tri.size(); k++) {
            const rt_vec3 &v1 = b.e[b.tri[k]].u.triangle.v1, &e1 = edge1[k];
            double Tx = o.x - v1.x, Ty = o.y - v1.y, Tz = o.z - v1.z;
            // Q = vector_cross_product(T, Edge1) (:431, :549-552)
            double Qx = Ty * e1.z - Tz * e1.y, Qy = Tz * e1.x - Tx * e1.z, Qz = Tx * e1.y - Ty * e1.x;
            t.insert(t.end(), {Tx, Ty, Tz, Qx, Qy, Qz, 0, 0});
        }
    }
    h.o_pl = (int)t.size();
    for (int i : b.pl) {
        const auto &p = b.e[i].u.plane;
        t.insert(t.end(), {p.normal.x, p.normal.y, p.normal.z, p.distance});
    }
    h.o_pl_org = (int)t.size();
    for (const rt_vec3 &o : b.org) {
        for (int i : b.pl) {
            const auto &p = b.e[i].u.plane;
            double V0 = -(p.normal.x * o.x + p.normal.y * o.y + p.normal.z * o.z + p.distance);
            t.push_back(V0);
        }
    }
}

// Per-object shading records by compact id (what lighting_function/6, :209-252, reads of the hit
// object: normal or centre, material), then the lights.  int_pow: every specular power is an
// integer in [0, 1024], so the kernels need no general pow (rt_math.inc, GENPOW).
static void shading_tables(Build &b) {
    SceneHdr &h = b.h;
    std::vector<double> &t = b.t;
    h.int_pow = 1;
    while (t.size() % 2) t.push_back(0); // every later section starts 16-byte aligned
    h.o_obj = (int)t.size();
    for (int i : b.objs) {
        const rt_elem &o = b.e[i];
        const rt_material *m;
        double a = 0, bb = 0, c = 0;
        if (o.kind == RT_SPHERE) {
            m = &o.u.sphere.material;
            a = o.u.sphere.center.x; bb = o.u.sphere.center.y; c = o.u.sphere.center.z;
        } else if (o.kind == RT_TRIANGLE) {
            m = &o.u.triangle.material;
            // Normal = vector_normalize(vector_cross_product(v1, v2)) (:448-451), a constant
            const rt_vec3 &v1 = o.u.triangle.v1, &v2 = o.u.triangle.v2;
            double nx = v1.y * v2.z - v1.z * v2.y, ny = v1.z * v2.x - v1.x * v2.z, nz = v1.x * v2.y - v1.y * v2.x;
            double mag = std::sqrt(nx * nx + ny * ny + nz * nz);
            if (mag == 0) {
                a = bb = c = 0;
            } else {
                double s = 1 / std::sqrt(nx * nx + ny * ny + nz * nz);
                a = nx * s; bb = ny * s; c = nz * s;
            }
        } else {
            m = &o.u.plane.material;
            a = o.u.plane.normal.x; bb = o.u.plane.normal.y; c = o.u.plane.normal.z;
        }
        const double sp = m->specular_power;
        if (!(sp >= 0.0 && sp <= 1024.0 && sp == std::floor(sp))) h.int_pow = 0;
        t.insert(t.end(), {a, bb, c, m->colour.x, m->colour.y, m->colour.z, m->specular_power, m->shininess,
                           m->reflectivity, 0, 0, 0});
    }
    h.o_light = (int)t.size();
    for (int li : b.lights) {
        const auto &L = b.e[li].u.point_light;
        t.insert(t.end(), {L.diffuse_colour.x, L.diffuse_colour.y, L.diffuse_colour.z, L.location.x, L.location.y,
                           L.location.z, L.specular_colour.x, L.specular_colour.y, L.specular_colour.z, 0, 0, 0});
    }
}

// The cone rows per (origin, sphere), SPH_OB_W doubles each, then the same rows in binary32 for
// the binary32 beams: sin(rho) rounded up and widened, cos(rho) rounded down and narrowed by
// BEAM32_EPS, |v| - r rounded down.
static void cone_rows(Build &b) {
    SceneHdr &h = b.h;
    std::vector<double> &t = b.t;
    h.o_sph_ob = (int)t.size();
    for (const rt_vec3 &o : b.org) {
        for (int i : b.sph) {
            const auto &s = b.e[i].u.sphere;
            double vx = s.center.x - o.x, vy = s.center.y - o.y, vz = s.center.z - o.z;
            const Cone c = cone_of(vx, vy, vz, std::fabs(s.radius), CULL_EPS);
            t.insert(t.end(), {vx, vy, vz, c.vl, c.sr, c.cr, c.near ? 1.0 : 0.0, c.dlow});
        }
    }
    h.o_sph_ob32 = (int)t.size();
    for (const rt_vec3 &o : b.org) {
        for (int i : b.sph) {
            const auto &s = b.e[i].u.sphere;
            double vx = s.center.x - o.x, vy = s.center.y - o.y, vz = s.center.z - o.z;
            const Cone c = cone_of(vx, vy, vz, std::fabs(s.radius), (double)BEAM32_EPS);
            float f[SPH_OB32_W] = {(float)vx, (float)vy, (float)vz, (float)c.vl, f32_up(c.sr), f32_down(c.cr),
                                   c.near ? 1.0f : 0.0f, f32_down(c.dlow)};
            double d[SPH_OB32_W / 2];
            std::memcpy(d, f, sizeof(d));
            t.insert(t.end(), d, d + SPH_OB32_W / 2);
        }
    }
}

// Beam-culling tables (only consulted by the kernel when h.cull_ok; 16-byte aligned records) and
// the flags that depend on the scene's extent.
static void cull_tables(Build &b) {
    SceneHdr &h = b.h;
    while (b.t.size() % 2) b.t.push_back(0);
    h.o_sph_b = (int)b.t.size();
    for (int i : b.sph) {
        const auto &s = b.e[i].u.sphere;
        b.t.insert(b.t.end(), {s.center.x, s.center.y, s.center.z, std::fabs(s.radius)});
    }
    cone_rows(b);
    // hdr.ext: the largest |coordinate| or |radius| of the origins and spheres.  cull_ok, the
    // binary32 beams' margins (rt_cull.inc, make_beam32), norm_ok's tolerance below and the ray
    // queries' BVH domain (rt_query.hip) depend on it.
    double ext = 0;
    auto grow = [&](double v) { ext = std::fmax(ext, std::fabs(v)); };
    for (const rt_vec3 &o : b.org) { grow(o.x); grow(o.y); grow(o.z); }
    for (int i : b.sph) {
        const auto &s = b.e[i].u.sphere;
        grow(s.center.x); grow(s.center.y); grow(s.center.z); grow(s.radius);
    }
    h.cull_ok = ext <= CULL_EXTENT ? 1 : 0;
    h.ext = ext;
    // normalize3's range checks that cannot fail (SceneHdr::norm_ok / prim_ok)
    bool ok = h.cull_ok && h.n_tri == 0 && h.n_pl == 0;
    const double tol = 1.0e-9 * (h.ext + 1.0);
    for (int i : b.sph) {
        if (!ok) break;
        const auto &s = b.e[i].u.sphere;
        const double r = std::fabs(s.radius);
        if (!(r >= 1.0e-50)) ok = false;
        for (int li : b.lights) {
            const rt_vec3 &L = b.e[li].u.point_light.location;
            const double dx = L.x - s.center.x, dy = L.y - s.center.y, dz = L.z - s.center.z;
            if (!(std::fabs(std::sqrt(dx * dx + dy * dy + dz * dz) - r) > tol)) ok = false;
        }
    }
    h.norm_ok = ok ? 1 : 0;
    // Wave beams (a cone over the wave's rays, a candidate mask per 64 spheres) cost a few wave
    // reductions per scan; with a handful of spheres testing every one is cheaper.
    h.beam_ok = h.cull_ok && h.n_sph >= knobs().beam_min ? 1 : 0;
}

// Sphere BVH for the reflection scans (rt_layout.h).  Binary, one sphere per leaf; splits by the
// surface area heuristic within a depth cap (or median splits along the longest axis of the
// centroids' bounds), so the depth is bounded and the per-lane stack never overflows.
// Each sphere's box is its centre +- |r| widened by m = BVH_BOX_REL * (extent + 1), far more than
// the binary32 rounding of the kernel's slab test (origins and directions rounded to binary32,
// relative error ~2^-22 in the slab distances) for scenes within CULL_EXTENT; the box test is only
// a filter, every sphere it lets through is tested by the reference's binary64 expressions.
struct Box {
    double lo[3], hi[3];
};
static const Box EMPTY_BOX = {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
static Box join(const Box &a, const Box &b) {
    Box u;
    for (int c = 0; c < 3; ++c) {
        u.lo[c] = std::fmin(a.lo[c], b.lo[c]);
        u.hi[c] = std::fmax(a.hi[c], b.hi[c]);
    }
    return u;
}
static double area(const Box &x) {
    const double dx = x.hi[0] - x.lo[0], dy = x.hi[1] - x.lo[1], dz = x.hi[2] - x.lo[2];
    return dx * dy + dy * dz + dz * dx;
}
struct Node {
    Box b[2];
    int ch[2]; // >= 0: node, < 0: ~sphere (table index)
};
struct Tree {
    const Build &b;
    std::vector<Box> box;   // per sphere (table index)
    std::vector<int> items; // the spheres, permuted as the splits sort them
    std::vector<Node> nodes;
    int cap = 0, max_depth = 0; // SAH depth cap (0: median splits); deepest leaf
    double centre(int k, int a) const {
        const rt_vec3 &c = b.sphere(k).center;
        return a == 0 ? c.x : a == 1 ? c.y : c.z;
    }
    // the one order of the splits: centre along axis a, ties by index (a total order, so every
    // sort's result is unique)
    void sort_by(std::vector<int>::iterator first, std::vector<int>::iterator last, int a) const {
        std::sort(first, last, [this, a](int p, int q) {
            const double kp = centre(p, a), kq = centre(q, a);
            return kp < kq || (kp == kq && p < q);
        });
    }
};

// The surface-area-heuristic split of items[b, en) at level lvl: the axis and how many items go
// left, over all three axes among the positions that leave each side at most lim leaves (what
// fits below it within the cap); (ax, half) — the median split — when there is none.
struct Split {
    int axis, left;
};
static Split sah_split(const Tree &T, int b, int en, int lvl, int ax) {
    const int cnt = en - b, lim = 1 << (T.cap - lvl - 1); // each side's leaves within the cap
    double best = INFINITY;
    Split s = {ax, cnt / 2};
    std::vector<int> tmp(T.items.begin() + b, T.items.begin() + en);
    std::vector<Box> suf(cnt + 1);
    for (int a = 0; a < 3; ++a) {
        T.sort_by(tmp.begin(), tmp.end(), a);
        suf[cnt] = EMPTY_BOX;
        for (int i = cnt - 1; i >= 0; --i) suf[i] = join(suf[i + 1], T.box[tmp[i]]);
        Box pre = EMPTY_BOX;
        for (int i = 1; i < cnt; ++i) {
            pre = join(pre, T.box[tmp[i - 1]]);
            if (i > lim || cnt - i > lim) continue;
            const double cost = area(pre) * i + area(suf[i]) * (cnt - i);
            if (cost < best) {
                best = cost;
                s = {a, i};
            }
        }
    }
    return s;
}

// returns the link of the subtree over items[b, en) and its box
static int build_subtree(Tree &T, int b, int en, int lvl, Box &box) {
    if (en - b == 1) {
        box = T.box[T.items[b]];
        T.max_depth = std::max(T.max_depth, lvl);
        return ~T.items[b];
    }
    Box cb = EMPTY_BOX; // the centroids' bounds
    for (int i = b; i < en; ++i) {
        for (int a = 0; a < 3; ++a) {
            cb.lo[a] = std::fmin(cb.lo[a], T.centre(T.items[i], a));
            cb.hi[a] = std::fmax(cb.hi[a], T.centre(T.items[i], a));
        }
    }
    int ax = 0;
    for (int a = 1; a < 3; ++a)
        if (cb.hi[a] - cb.lo[a] > cb.hi[ax] - cb.lo[ax]) ax = a;
    T.sort_by(T.items.begin() + b, T.items.begin() + en, ax);
    int mid = b + (en - b) / 2;
    if (T.cap > 0) {
        const Split s = sah_split(T, b, en, lvl, ax);
        T.sort_by(T.items.begin() + b, T.items.begin() + en, s.axis);
        mid = b + s.left;
    }
    const int self_i = (int)T.nodes.size();
    T.nodes.push_back(Node{});
    Box bl, br;
    const int l = build_subtree(T, b, mid, lvl + 1, bl);
    const int r = build_subtree(T, mid, en, lvl + 1, br);
    T.nodes[self_i] = Node{{bl, br}, {l, r}};
    box = join(bl, br);
    return self_i;
}

// One 64-byte node: (lx0 lx1 ly0 ly1) (lz0 lz1 ux0 ux1) (uy0 uy1 uz0 uz1): the two children's
// bounds side by side, so the kernel's slab distances of both are packed binary32 pairs; then the
// two links and, for a sphere child, its compact object id.
static void pack_node(const Build &b, const Node &nd, std::vector<double> &t) {
    float f[16];
    const Box &b0 = nd.b[0], &b1 = nd.b[1];
    for (int a = 0; a < 3; ++a) {
        f[2 * a] = f32_down(b0.lo[a]);
        f[2 * a + 1] = f32_down(b1.lo[a]);
        f[6 + 2 * a] = f32_up(b0.hi[a]);
        f[6 + 2 * a + 1] = f32_up(b1.hi[a]);
    }
    std::memcpy(&f[12], &nd.ch[0], 4);
    std::memcpy(&f[13], &nd.ch[1], 4);
    const int id0 = nd.ch[0] < 0 ? b.compact[b.sph[~nd.ch[0]]] : -1, id1 = nd.ch[1] < 0 ? b.compact[b.sph[~nd.ch[1]]] : -1;
    std::memcpy(&f[14], &id0, 4);
    std::memcpy(&f[15], &id1, 4);
    double d[BVH_NODE_DOUBLES];
    std::memcpy(d, f, sizeof(d));
    t.insert(t.end(), d, d + BVH_NODE_DOUBLES);
}

// The extent the boxes' inflation m is relative to (the ext' of rt_query.hip's domain proof):
// origins by coordinate, spheres by |coordinate| + |radius|, so it is at least hdr.ext.
static double box_extent(const Build &b) {
    double ext = 0;
    for (const rt_vec3 &o : b.org) ext = std::fmax(ext, std::fmax(std::fabs(o.x), std::fmax(std::fabs(o.y), std::fabs(o.z))));
    for (int i : b.sph) {
        const auto &s = b.e[i].u.sphere;
        ext = std::fmax(ext, std::fmax(std::fabs(s.center.x), std::fmax(std::fabs(s.center.y), std::fabs(s.center.z))) +
                                 std::fabs(s.radius));
    }
    return ext;
}

static void build_bvh(Build &b) {
    SceneHdr &h = b.h;
    h.bvh_ok = 0;
    h.o_bvh = 0;
    h.n_bvh = 0;
    h.bvh_level = 1 << 30;
    h.bvh_depth = 0;
    h.l_bvh = h.l_bsph = -1;
    h.l_stack = 0;
    const int n = h.n_sph;
    if (!h.cull_ok || n < 2 || n < knobs().bvh_min || n > BVH_MAX_SPHERES) return;
    int depth = 0;
    while ((1 << depth) < n) ++depth;
    if (depth > BVH_STACK) return; // a node at depth i holds at most i stack entries, pushes one more
    Tree T{b};
    // Surface-area-heuristic splits among those that keep every leaf within ceil(log2 n) + slack
    // levels (the traversal stack's size; BVH_SAH_SLACK; 0: median splits).
    // Measured, config 5: slack 2 -2.2 % per frame against median splits; 1 or 3 neutral.
    constexpr int slack = BVH_SAH_SLACK;
    T.cap = slack > 0 && depth + 1 <= BVH_STACK ? std::min(depth + slack, BVH_STACK) : 0;
    const double m = BVH_BOX_REL * (box_extent(b) + 1.0);
    for (int k = 0; k < n; ++k) {
        const auto &s = b.sphere(k);
        const double c[3] = {s.center.x, s.center.y, s.center.z}, r = std::fabs(s.radius);
        Box bx;
        for (int a = 0; a < 3; ++a) {
            bx.lo[a] = c[a] - r - m;
            bx.hi[a] = c[a] + r + m;
        }
        T.box.push_back(bx);
        T.items.push_back(k);
    }
    T.nodes.reserve(n);
    Box all;
    build_subtree(T, 0, n, 0, all);
    while (b.t.size() % 2) b.t.push_back(0); // 16-byte aligned nodes
    h.o_bvh = (int)b.t.size();
    for (const Node &nd : T.nodes) pack_node(b, nd, b.t);
    h.n_bvh = (int)T.nodes.size();
    h.bvh_depth = T.max_depth;
    h.bvh_ok = 1;
    h.bvh_level = knobs().bvh_level < 1 ? 1 : knobs().bvh_level;
}

// The int table's ids by type and the meta row of every object.
static void id_tables(Build &b) {
    SceneHdr &h = b.h;
    std::vector<int> &it = b.it;
    h.i_sph_id = (int)it.size();
    for (int i : b.sph) it.push_back(b.compact[i]);
    h.i_tri_id = (int)it.size();
    for (int i : b.tri) it.push_back(b.compact[i]);
    h.i_pl_id = (int)it.size();
    for (int i : b.pl) it.push_back(b.compact[i]);
    while (it.size() % 4) it.push_back(0); // 16-byte rows
    h.i_obj_meta = (int)it.size();
    // each element's index within its type's table
    std::vector<int> local_of(b.e.size(), 0);
    for (const std::vector<int> *grp : {&b.sph, &b.tri, &b.pl})
        for (size_t q = 0; q < grp->size(); q++) local_of[(*grp)[q]] = (int)q;
    for (int i : b.objs) {
        int kind = b.e[i].kind == RT_SPHERE ? K_SPHERE : (b.e[i].kind == RT_TRIANGLE ? K_TRIANGLE : K_PLANE);
        // the canonical (first exactly equal) element is a record of the same type: its index
        // within the type is stored here too, so a shadow target resolves in one load
        const int r = root(b.e, i);
        it.insert(it.end(), {kind, local_of[i], b.compact[r], local_of[r]});
    }
}

// the scenes whose tables may be staged in LDS: spheres only, with culling and a light
static bool stage_kind(const SceneHdr &h) {
    return h.cull_ok && h.n_tri == 0 && h.n_pl == 0 && h.n_sph > 0 && h.n_light > 0;
}

// Whether the occluder masks exist and how many direction cells they have.
static void occluder_policy(SceneHdr &h) {
    h.n_chunk = (h.n_sph + 63) / 64;
    // Small scenes and scenes whose tables are staged in LDS (stage_layout) keep one cell: their walks
    // are short (S64: 1.37 steps per test) and the cells' extra LDS and binary32 work cost more
    // than they save (measured: config 3 -5 %); large scenes get OCC_CELLS (config 5: +4 %).
    const bool fits = stage_kind(h) && stage_lds_place(h, 1) <= LDS_STAGE_MAX;
    h.occ_cells = (h.n_sph < OCC_CELLS_MIN_SPHERES || fits) ? 1 : OCC_CELLS;
    // The masks cost the host one (light, target, sphere) test per triple and the device
    // n_light * n_sph^2 * cells bits: beyond OCC_MAX_TESTS tests there are none (occ_ok = 0) and
    // the shadow rays take the shadow cones over the sphere chunks instead (lit_by); beyond
    // OCC_MAX_BYTES the masks keep one cell.
    const double occ_tests = (double)h.n_light * h.n_sph * h.n_sph;
    h.occ_ok = h.cull_ok && h.n_sph > 0 && occ_tests <= OCC_MAX_TESTS ? 1 : 0;
    if (h.occ_ok && (double)h.n_light * h.n_sph * h.occ_cells * h.n_chunk * 8 > OCC_MAX_BYTES) h.occ_cells = 1;
}

// Occluder masks, per (light, target sphere, direction cell).  Shadow rays to a target
// sphere t start at the light L and point into the cone from L around ball(c_t, r_t); the
// target's own t* (its entry point) is at most |c_t - L|.  Sphere j can block such a ray only
// if (a) it meets that cone (angular test as in the kernel's beam culling, with CULL_EPS
// margins in the safe direction) and (b) some point of it is within |c_t - L| of L.  The
// target itself never blocks (its t equals t* and its list position is not earlier).
// Cells (the kernel's occ_cell): the cone is split by the signs of dir - a along two world
// axes i, j (a = (c_t - L)/|c_t - L|; the axes on which a is shortest, chosen from the
// binary32 components of L - c_t exactly as the kernel chooses them).  Sphere j stays in cell
// (b_i, b_j) only if its cone of directions (axis w, sin of its half-angle sr) reaches the
// half-spaces s*(dir_k - a_k) >= -OCC_CELL_EPS, s = +1 for b_k = 1 and -1 for b_k = 0: the
// largest s*dir_k over the cone is cos(max(0, angle(w, s*e_k) - rho)).
struct CellFrame {
    double a3[3]; // a, the target's direction from the light
    int axi, axj; // the kernel's cell axes
    double tau;   // the kernel's |sd - a| split: half the target cone's sine
};
// Does the cone of directions (unit axis w3, half-angle rho) reach cell c of the frame?
static bool in_cell(const CellFrame &f, const double w3[3], double rho, int c) {
    const double eps = OCC_CELL_EPS;
    // the cone reaches s*(dir_k - a_k) in [t_lo, t_hi] (widened by eps): its largest s*dir_k is
    // cos(max(0, psi - rho)), its smallest cos(min(pi, psi + rho))
    auto reach = [&](int k, double s, double t_lo, double t_hi) {
        const double psi = std::acos(std::max(-1.0, std::min(1.0, s * w3[k])));
        const double top = psi <= rho ? 1.0 : std::cos(psi - rho);
        const double bot = psi + rho >= M_PI ? -1.0 : std::cos(psi + rho);
        if (top + 1e-7 < s * f.a3[k] + t_lo - eps) return false;
        if (bot - 1e-7 > s * f.a3[k] + t_hi + eps) return false;
        return true;
    };
    // the kernel's bins along one axis (occ_cell): the sign of dir_k - a_k and |dir_k - a_k|
    // below / above tau
    auto reach_bin = [&](int k, int bin) {
        const double inf = 1e300;
        return reach(k, (bin & 1) ? 1.0 : -1.0, (bin & 2) ? f.tau : 0.0, (bin & 2) ? inf : f.tau);
    };
    // cell -> the bins of axes i and j (occ_cell's numbering)
    const int bi = (c & 1) | ((c >> 1) & 2), bj = ((c >> 1) & 1) | ((c >> 2) & 2);
    return reach_bin(f.axi, bi) && reach_bin(f.axj, bj);
}

// One sphere as a light sees it: v = c - L and its cone.  The same row serves the sphere as a
// target (st, ct, wide = sr, cr, near) and as a candidate occluder.
struct Seen {
    double v[3];
    Cone c;
};

// The masks m (ncell rows of n_chunk words) of light L and target sphere ti.
static void target_masks(const Build &b, const rt_vec3 &L, const std::vector<Seen> &seen, size_t ti, int ncell,
                         std::vector<uint64_t> &m) {
    const Seen &T = seen[ti];
    const rt_vec3 &ct3 = b.sphere((int)ti).center;
    const double D = T.c.vl, st = T.c.sr, ct = T.c.cr;
    const double tmax = D * (1 + CULL_EPS) + CULL_EPS;
    // the kernel's cell axes, from the binary32 components of its row (L - c_t)
    const float qx = (float)(L.x - ct3.x), qy = (float)(L.y - ct3.y), qz = (float)(L.z - ct3.z);
    const float fx = std::fabs(qx), fy = std::fabs(qy), fz = std::fabs(qz);
    const int drop = (fx >= fy && fx >= fz) ? 0 : (fy >= fz ? 1 : 2);
    const CellFrame f = {{T.v[0] / D, T.v[1] / D, T.v[2] / D}, drop == 0 ? 1 : 0, drop == 2 ? 1 : 2,
                         std::fabs(b.sphere((int)ti).radius) / D * 0.5};
    const bool wide = T.c.near || !(ct > 0.0); // the light inside the target, or nearly: no angular test
    for (size_t j = 0; j < seen.size(); j++) {
        if (j == ti) continue;
        const Seen &S = seen[j];
        const double vl = S.c.vl;
        bool keep = true, cells = false;
        if (!wide && !S.c.near) {
            const double thr = ct * S.c.cr - st * S.c.sr;
            const double av = (T.v[0] * S.v[0] + T.v[1] * S.v[1] + T.v[2] * S.v[2]) / D;
            keep = !(av + CULL_EPS * vl < thr * vl);
            cells = true;
        }
        if (!keep || S.c.dlow > tmax) continue;
        const bool split = cells && ncell > 1; // otherwise the sphere stays in every cell
        const double w3[3] = {S.v[0] / vl, S.v[1] / vl, S.v[2] / vl};
        const double rho = split ? std::asin(S.c.sr) + CULL_EPS : 0.0;
        for (int c = 0; c < ncell; c++) // (ncell is OCC_CELLS or 1)
            if (!split || in_cell(f, w3, rho, c)) m[(size_t)c * b.h.n_chunk + j / 64] |= 1ull << (j % 64);
    }
}

static void occluder_masks(Build &b) {
    SceneHdr &h = b.h;
    while (b.it.size() % 2) b.it.push_back(0);
    h.i_occ = (int)b.it.size();
    if (!h.occ_ok) return;
    std::vector<Seen> seen(h.n_sph);
    std::vector<uint64_t> m;
    for (int i = 0; i < h.n_light; i++) {
        const rt_vec3 &L = b.light(i);
        for (int k = 0; k < h.n_sph; k++) {
            const auto &S = b.sphere(k);
            const double vx = S.center.x - L.x, vy = S.center.y - L.y, vz = S.center.z - L.z;
            seen[k] = Seen{{vx, vy, vz}, cone_of(vx, vy, vz, std::fabs(S.radius), CULL_EPS)};
        }
        for (size_t ti = 0; ti < seen.size(); ti++) {
            m.assign((size_t)h.occ_cells * h.n_chunk, 0);
            target_masks(b, L, seen, ti, h.occ_cells, m);
            for (uint64_t w : m) {
                b.it.push_back((int)(uint32_t)(w & 0xffffffffu));
                b.it.push_back((int)(uint32_t)(w >> 32));
            }
        }
    }
}

// camera: point_on_screen/3 (:486-503) with focal_length/2 (:483-484).
// Sum = foldl(fun(V, S) -> vector_add(V, S) end, Location, [ {0*F,0*F,1*F}, {(X-0.5)*SW,0,0},
// {0,(Y-0.5)*SH,0} ]); the pixel-invariant parts are folded here in the same order.
static int camera(Build &b) {
    SceneHdr &h = b.h;
    const auto &cam = b.e[0].u.camera;
    double SW = cam.screen_width, SH = cam.screen_height;
    double F = SW / (2 * std::tan(cam.fov * (M_PI / 180) / 2));
    const rt_vec3 &L = cam.location;
    h.cam_x = L.x; h.cam_y = L.y; h.cam_z = L.z;
    h.sx = 0 * F + L.x;                       // x after step 1; step 2 adds (X-0.5)*SW, step 3 adds 0
    h.sy = 0.0 + (0 * F + L.y);               // y after steps 1-2; step 3 adds (Y-0.5)*SH
    double pz = 0.0 + (0.0 + (1 * F + L.z));  // z after steps 1-3
    h.dz = pz - L.z;                          // vector_sub(Through, From).z (:507)
    if (!std::isfinite(F) || !std::isfinite(h.sx) || !std::isfinite(h.sy) || !std::isfinite(h.dz))
        return RT_EBADARG; // Erlang raises badarith where binary64 would overflow
    h.screen_w = SW;
    h.screen_h = SH;
    h.n_light_d = (double)h.n_light;
    // primary rays: Through - From = (px - cx, py - cy, dz) with X, Y in [0, 1]: squared length
    // at least dz^2, at most (|sx| + |w| + |cx|)^2 + (|sy| + |h| + |cy|)^2 + dz^2 (prim_ok)
    const double bx = std::fabs(h.sx) + std::fabs(h.screen_w) + std::fabs(h.cam_x);
    const double by = std::fabs(h.sy) + std::fabs(h.screen_h) + std::fabs(h.cam_y);
    const double lo = h.dz * h.dz, hi = bx * bx + by * by + h.dz * h.dz;
    h.prim_ok = (lo >= 1.0e-100 && hi <= 1.0e100) ? 1 : 0;
    return RT_OK;
}

// LDS staging layout: the scenes of stage_kind whose masks exist with one cell, if they fit
static void stage_layout(SceneHdr &h) { stage_lds_place(h, stage_kind(h) && h.occ_ok ? h.occ_cells : 0); }

int compile_scene(const rt_elem *in, uint32_t n, Compiled &out) {
    int rc = check_scene(in, n);
    if (rc != RT_OK) return rc;
    Build b(in, n, out);
    fill_canon(b.e.data(), n);
    if ((rc = classify(b, n)) != RT_OK) return rc;
    order_spheres(b);
    // the double table, in this order
    primitive_tables(b);
    shading_tables(b);
    cull_tables(b);
    build_bvh(b);
    if (b.t.empty()) b.t.push_back(0);
    // the int table
    id_tables(b);
    occluder_policy(b.h);
    occluder_masks(b);
    if (b.it.empty()) b.it.push_back(0);
    // the kernels index both tables with 32-bit ints
    if (b.t.size() >= (size_t)INT32_MAX / 2 || b.it.size() >= (size_t)INT32_MAX / 2) return RT_ENOMEM;
    if ((rc = camera(b)) != RT_OK) return rc;
    stage_layout(b.h);
    return RT_OK;
}

} // namespace rtl
