"""Deterministic hostile scenes: the inputs ``scenes.synthetic_scene`` rejects.

The culling filters (wave beams, primary candidate masks, occluder masks and their direction
cells, shadow cones, the sphere BVH) and the camera set-up have branches that exist only for
scenes the benchmark generator never makes: an origin inside or on a sphere (``near`` / ``wide``
rows, ``sr >= 1``), degenerate radii and lights on a surface (``norm_ok = 0``), coordinates near
``CULL_EXTENT``, axis-parallel rays (``bvh_inv``'s clamp), exact distance ties, and cameras
whose location and focal length are not (0, 0, -2) and 2.  The builders here make such scenes,
without a GPU and with no randomness beyond ``SplitMix64``.

Every coordinate is a multiple of 2**-10 (exact in binary64 and in its Erlang text) except the
few decimal literals the cases are defined by (radii 0.015 and 0.016, the camera locations
(0.3, -1.7, -2.1) and (1/3, 0.1, -12.7), the 4e-60 screens), whose shortest decimal text
round-trips.  Colours are in [0, 1].  Every specular power is 0 or 1: ``pow(x, 0)`` and
``pow(x, 1)`` are exact in glibc and in the kernels' ``pow_libm``, so a frame of these scenes
must equal the oracle's bit for bit.

``SCENES`` maps a name to ``(builder, depth)``; ``build(name)`` returns the scene list.
"""
from __future__ import annotations

from eraytracer_amd import _native as N
from eraytracer_amd import scenes
from eraytracer_amd.records import camera, colour, material, point_light, screen, sphere, vector

BASES = ("s7", "s8", "s16", "s160", "mixed_int", "s300l190")
FAR_SHIFTS = {"far4900": (4900, 0, 0), "far5100": (5100, 0, 0), "far9970": (9970, -9000, 5000),
              "far10100": (10100, 0, 0)}


def _is_obj(t):
    return t[0] in ("sphere", "triangle", "plane")


def unit_powers(scene):
    """The scene with every object's specular power rewritten to 0 or 1 (alternating in list order)."""
    out, i = [], 0
    for t in scene:
        if _is_obj(t):
            m = t[-1]
            t = t[:-1] + (material(m[1], i % 2, m[3], m[4]),)
            i += 1
        out.append(t)
    return out


def base(name):
    return unit_powers(scenes.named(name))


def _mats(seed):
    """An endless supply of materials: colour in [0,1]^3, power in {0,1}, shininess in [0,1],
    reflectivity in [0.125, 0.75]."""
    rng = scenes.SplitMix64(seed)
    while True:
        col = (rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1))
        yield material(colour(*col), rng.next_u64() % 2, rng.uniform(0, 1), rng.uniform(0.125, 0.75))


def _lights(scene):
    return [t for t in scene if t[0] == "point_light"]


def _loc(light):
    return light[2][1:]


def geometry_set(lights, swap_pair=False):
    """G: a mirrored pair, twins (and a 2 / 2.0 copy), concentric, tangent, enclosing, light-enclosing
    and negative-radius spheres.  Keeps norm_ok = 1 (no light on a surface, no tiny radius)."""
    m = _mats(0x5EED600D)
    a, b = next(m), next(m)
    pair = [sphere(1.5, vector(-1, 0, 10), a), sphere(1.5, vector(1, 0, 10), b)]
    if swap_pair:
        pair.reverse()
    t1, t2 = next(m), next(m)
    lx, ly, lz = _loc(lights[0])
    return pair + [
        # twins: same centre and radius, other material; and the first one again with radius 2.0
        # (2 =/= 2.0: not the same term, so the first twin shadows it and is never lit through it)
        sphere(2, vector(-5, -3, 14), t1), sphere(2, vector(-5, -3, 14), t2), sphere(2.0, vector(-5, -3, 14), t1),
        # concentric
        sphere(1, vector(5, 2, 12), next(m)), sphere(2, vector(5, 2, 12), next(m)),
        # tangent: centres 2 apart, radius 1
        sphere(1, vector(-4, 3, 9), next(m)), sphere(1, vector(-2, 3, 9), next(m)),
        # encloses the camera, every light and every object of the S scenes (never hit from inside)
        sphere(30, vector(0, -2, 18), next(m)),
        # round light 0 (the light is inside, half a unit off the centre)
        sphere(1.5, vector(lx + 0.5, ly, lz), next(m)),
        # negative radius (r*r is what the reference uses)
        sphere(-1.5, vector(3, -3, 8), next(m)),
    ]


def degenerate_set(lights):
    """D minus G: radius 0, 0.015 (4 r^2 < 0.001: never hit), 0.016 (hit only near its axis; on the
    axis of the ray through X = 0.625, Y = 0.5), a light exactly on a surface and one at a centre."""
    m = _mats(0x5EEDDE6E)
    x1, y1, z1 = _loc(lights[1])
    x2, y2, z2 = _loc(lights[2])
    return [
        sphere(0, vector(0, 0.75, 2), next(m)),
        sphere(0.015, vector(-1, 0, 2), next(m)),
        sphere(0.016, vector(1, 0, 2), next(m)),
        sphere(3, vector(x1, y1, z1 + 3), next(m)),
        sphere(1, vector(x2, y2, z2), next(m)),
    ]


def with_set(base_name, which, swap_pair=False):
    """The base with G (which = 'g') or D (= 'd') inserted before its first object, so that a
    distance tie favours the hostile element."""
    sc = base(base_name)
    lights = _lights(sc)
    extra = geometry_set(lights, swap_pair)
    if which == "d":
        extra = extra + degenerate_set(lights)
    k = next(i for i, t in enumerate(sc) if _is_obj(t))
    return sc[:k] + extra + sc[k:]


def small_ties():
    """S2 with G's pair and twins only: 7 spheres, below BEAM_MIN_SPHERES, so the ties are scanned
    without wave beams (G itself lifts every base over that threshold)."""
    sc = base("s2")
    k = next(i for i, t in enumerate(sc) if _is_obj(t))
    return sc[:k] + geometry_set(_lights(sc))[:5] + sc[k:]


def lattice():
    """5x5x6 unit spheres at (3i-6, 3j-6, 8+3k) and a 5x5 wall at z = -8 behind the camera: 175
    spheres.  At even W and H the centre pixel's ray is (0, 0, 1) exactly and ping-pongs between
    (0, 0, 8) and (0, 0, -8), so every level traces an axis-parallel ray."""
    m = _mats(0x5EED1A77)
    sc = [camera(vector(0, 0, -2), vector(0, 0, 0), 90, screen(4, 3)),
          point_light(colour(1, 0.75, 0.5), vector(-7.5, -7.5, 0.5), colour(1, 1, 1)),
          point_light(colour(0.5, 0.75, 1), vector(4.5, 7.5, 3.5), colour(0.5, 1, 0.75))]
    for k in range(6):
        for j in range(5):
            for i in range(5):
                sc.append(sphere(1, vector(3 * i - 6, 3 * j - 6, 8 + 3 * k), next(m)))
    for j in range(5):
        for i in range(5):
            sc.append(sphere(1, vector(3 * i - 6, 3 * j - 6, -8), next(m)))
    return sc


def shifted(scene, d):
    """Camera, lights and spheres moved by d."""
    def mv(v):
        return vector(v[1] + d[0], v[2] + d[1], v[3] + d[2])
    out = []
    for t in scene:
        if t[0] == "camera":
            t = camera(mv(t[1]), t[2], t[3], t[4])
        elif t[0] == "point_light":
            t = point_light(t[1], mv(t[2]), t[3])
        elif t[0] == "sphere":
            t = sphere(t[1], mv(t[2]), t[3])
        else:
            raise ValueError("shifted: spheres-only scenes")
        out.append(t)
    return out


def far(name):
    return shifted(base("s64"), FAR_SHIFTS[name])


def _first_sphere(scene):
    return next(t for t in scene if t[0] == "sphere")


CAMERAS = {
    "fov20": lambda sc: camera(vector(0, 0, -2), vector(0, 0, 0), 20, screen(4, 3)),
    "fov150": lambda sc: camera(vector(0, 0, -2), vector(0, 0, 0), 150, screen(4, 3)),
    "tall": lambda sc: camera(vector(0.3, -1.7, -2.1), vector(0, 0, 0), 90, screen(3, 4)),
    # F = -2: the screen is behind the location, the camera looks towards -z
    "negscreen": lambda sc: camera(vector(0, 0, 50), vector(0, 0, 0), 90, screen(-4, 3)),
    "vga": lambda sc: camera(vector(1 / 3, 0.1, -12.7), vector(0, 0, 0), 60, screen(640, 480)),
    "inside_cloud": lambda sc: camera(vector(0, -1, 20), vector(0, 0, 0), 90, screen(4, 3)),
    # prim_ok = 0 (dz^2 ~ 4e-120); the same view as screen 4x3 at the origin
    "tiny_origin": lambda sc: camera(vector(0, 0, 0), vector(0, 0, 0), 90, screen(4e-60, 3e-60)),
    # F + Lz absorbs F: dz = 0, every ray lies in the plane z = -2, the centre pixel's is (0, 0, 0)
    "dz0": lambda sc: camera(vector(0, 0, -2), vector(0, 0, 0), 90, screen(4e-60, 3e-60)),
    "inside_sphere": lambda sc: (lambda c: camera(vector(c[1] + 0.25, c[2] + 0.125, c[3]), vector(0, 0, 0), 90,
                                                  screen(4, 3)))(_first_sphere(sc)[2]),
}
CAMERA_BASES = ("s64", "mixed_int")


def with_camera(base_name, cam):
    sc = base(base_name)
    return [CAMERAS[cam](sc)] + sc[1:]


def _scenes():
    t = {}
    for b in BASES:
        d = 3 if b == "s300l190" else 5
        t[f"{b}+g"] = ((lambda b=b: with_set(b, "g")), d)
        t[f"{b}+d"] = ((lambda b=b: with_set(b, "d")), d)
    t["s7+g_swapped"] = ((lambda: with_set("s7", "g", swap_pair=True)), 5)
    t["s2+ties"] = (small_ties, 5)
    t["lattice"] = (lattice, 8)
    for f in FAR_SHIFTS:
        t[f] = ((lambda f=f: far(f)), 5)
    for b in CAMERA_BASES:
        for c in CAMERAS:
            t[f"{b}@{c}"] = ((lambda b=b, c=c: with_camera(b, c)), 5)
    return t


SCENES = _scenes()
NAMES = tuple(SCENES)


def build(name):
    return SCENES[name][0]()


def depth(name):
    return SCENES[name][1]


_REFS = {}


def oracle_ref(O, name, w, h, spp=1, seed=0, scenes=None):
    """The C oracle's (frame, levels) of a hostile scene at its depth, computed once per process
    and shared read-only among the tests.  scenes: another table of name -> (builder, depth), whose
    names are not this module's (tests/hostile_flat.py)."""
    builder, d = (SCENES if scenes is None else scenes)[name]
    key = (name, w, h, spp, seed)
    if key not in _REFS:
        img, lv = O.render(N.marshal(builder()), w, h, d, mode=O.MEMO, levels=True, spp=spp, seed=seed)
        img.setflags(write=False)
        lv.setflags(write=False)
        _REFS[key] = (img, lv)
    return _REFS[key]
