"""Deterministic hostile scenes of triangles and planes: the flat counterpart of tests/hostile.py.

The sphere paths are reached by tests/hostile.py.  The triangle and plane paths have branches of
their own that no other scene reaches: plane normals that are not unit vectors (reflected
directions with |d|^2 far from 1: the beams' ``bad`` lanes, the BVH walked by non-unit
directions), hit points far beyond ``CULL_EXTENT`` (``SceneHdr::ext`` bounds origins and spheres,
not triangle vertices or plane hit points), triangle and plane shadow targets (negative and huge
``t*``), the reference's triangle normal ``normalize(v1 x v2)`` of the *position* vectors (zero
when v1 || v2, never the geometric normal unless the triangle's plane holds the origin), scenes
without a sphere, and exact distance ties across the three kinds.

Conventions are tests/hostile.py's: no randomness beyond ``SplitMix64``, every coordinate dyadic
(exact in binary64 and in its Erlang text), colours in [0, 1], every specular power 0 or 1
(alternating in list order), so a frame must equal the oracle's bit for bit.  Plane normals have
magnitude in [0.5, 2], so reflection chains stay finite.

``SCENES`` maps a name to ``(builder, depth)``; ``build(name)`` returns the scene list.
"""
from __future__ import annotations

from eraytracer_amd.records import camera, colour, material, plane, point_light, screen, sphere, triangle, vector
from tests import hostile as H


def _camera(fov=90):
    return camera(vector(0, 0, -2), vector(0, 0, 0), fov, screen(4, 3))


def _lights():
    return [point_light(colour(1, 0.75, 0.5), vector(-3, -2, 1), colour(1, 1, 1)),
            point_light(colour(0.5, 0.75, 1), vector(3, 2, 12), colour(0.5, 1, 0.75))]


def _refl(m, reflectivity):
    return material(m[1], m[2], m[3], reflectivity)


def sph9(seed=0x5EED0009):
    """Nine unit spheres at (3i-3, 3j-3, 12+2i)."""
    m = H._mats(seed)
    return [sphere(1, vector(3 * i - 3, 3 * j - 3, 12 + 2 * i), next(m)) for i in range(3) for j in range(3)]


def _scene(objects, cam=None, lights=None):
    return H.unit_powers([cam or _camera()] + (lights if lights is not None else _lights()) + objects)


# ---- planes ---------------------------------------------------------------------------------------
def corridor_planes(floor=(vector(0, -1, 0), 5), ceiling=(vector(0, 1, 0), 5)):
    """A floor, a ceiling and a back wall facing each other, reflectivity .75 / .75 / .5."""
    m = H._mats(0x5EEDC0DD)
    return [plane(floor[0], floor[1], _refl(next(m), 0.75)), plane(ceiling[0], ceiling[1], _refl(next(m), 0.75)),
            plane(vector(0, 0, -1), 40, _refl(next(m), 0.5))]


def corridor():
    return _scene(corridor_planes() + sph9())


def corridor_nonunit():
    """The same three planes, the floor written with a normal of magnitude 2 and the ceiling 0.5:
    every reflection off them has a direction that is not a unit vector."""
    return _scene(corridor_planes((vector(0, -2, 0), 10), (vector(0, 0.5, 0), 2.5)) + sph9())


def mirror_nonunit():
    """sph9 in front of a back wall at z = 20 written with a normal of magnitude 1.5 and over a floor
    of magnitude 1.25: the reflections (dz -> -3.5 dz, dy -> -2.125 dy, |d| up to 3.5 a bounce) come
    back onto the spheres, so most rays that are not unit vectors end on a sphere."""
    m = H._mats(0x5EED3122)
    return _scene([plane(vector(0, 0, -1.5), 30, _refl(next(m), 0.75)), plane(vector(0, -1.25, 0), 6.25, _refl(next(m), 0.5))]
                  + sph9())


def planes_only():
    return _scene(corridor_planes())


def graze(k):
    """A floor tilted by 2^-k towards the camera's axis and a ceiling: rays that graze the floor hit
    it tens of thousands of units away."""
    m = H._mats(0x5EED6A2E)
    return _scene([plane(vector(0, -1, -2.0 ** -k), 5, _refl(next(m), 0.6)),
                   plane(vector(0, 1, 0), 5, _refl(next(m), 0.6))] + sph9())


# ---- triangles ------------------------------------------------------------------------------------
def mesh_triangles(nx=8, ny=6, side=1.5, z=10, seed=0x5EED3E54):
    """nx x ny cells of the given side centred on the axis in the plane z, two triangles a cell,
    (p00, p01, p10) and (p10, p01, p11) with pij = (x_i, y_j): all face the camera, and neighbours
    share edges (and corners), which rays through pixel centres hit at exactly equal t."""
    m = H._mats(seed)
    out = []
    for j in range(ny):
        for i in range(nx):
            x0, y0 = (i - nx / 2) * side, (j - ny / 2) * side
            p = {(a, b): vector(x0 + a * side, y0 + b * side, z) for a in (0, 1) for b in (0, 1)}
            out.append(triangle(p[0, 0], p[0, 1], p[1, 0], next(m)))
            out.append(triangle(p[1, 0], p[0, 1], p[1, 1], next(m)))
    return out


def mesh():
    return _scene(mesh_triangles() + sph9())


def mesh_small():
    return _scene(mesh_triangles(2, 2) + sph9())


def tris_only():
    return _scene(mesh_triangles())


def tie3(order):
    """A triangle, a plane and a sphere that the centre ray (0, 0, 1) hits at exactly 12.0, in the
    list order `order` (a string of t, p, s), before sph9."""
    m = H._mats(0x5EED071E)
    objs = {"t": triangle(vector(-4, -4, 10), vector(0, 4, 10), vector(4, -4, 10), next(m)),
            "p": plane(vector(0, 0, -1), 10, next(m)),
            "s": sphere(2, vector(0, 0, 12), next(m))}
    return _scene([objs[k] for k in order] + sph9())


def behind(facing):
    """A floor, sph9 and, last in the list, a large triangle in the plane z = -6 behind the camera.
    Facing the camera, every primary ray hits it at negative t, which wins every comparison;
    with two vertices swapped it is back-face culled for the primary rays, and shadow and
    reflection rays still see it."""
    m = H._mats(0x5EEDBE41)
    a, b, c = vector(-30, -30, -6), vector(0, 40, -6), vector(30, -30, -6)
    floor = plane(vector(0, -1, 0), 5, _refl(next(m), 0.3))
    tri = triangle(a, b, c, next(m)) if facing else triangle(a, c, b, next(m))
    return _scene([floor] + sph9() + [tri])


def behind_without():
    """behind_away without its triangle (not in SCENES: what behind_away is compared with)."""
    return behind(False)[:-1]


def zero_normal():
    """v2 = 4 v1: the reference's normal normalize(v1 x v2) is (0, 0, 0), so the triangle is never
    lit and the reflected ray leaves its hit point in the incoming direction."""
    m = H._mats(0x5EED0000)
    return _scene([triangle(vector(-1, -1, 4), vector(-4, -4, 16), vector(-6, 6, 9), next(m))] + sph9())


# ---- far hit points ---------------------------------------------------------------------------------
PENCIL_SPHERES = ((3, 0, 10), (-3, 0, 14), (0, 3, 18), (0, -3, 22), (5, 5, 12), (-5, 4, 16), (6, -2, 20), (-6, -3, 24),
                  (2.5, 2.5, 26), (-2.5, -2.5, 28))


def pencil(far_object):
    """A camera with a field of view of 2^-10 degrees: a pencil of almost parallel rays along the
    axis, past ten unit spheres, onto one object 2^19 away."""
    m = H._mats(0x5EED9E2C)
    lights = [point_light(colour(1, 0.75, 0.5), vector(-1, -1, 1), colour(1, 1, 1)),
              point_light(colour(0.5, 0.75, 1), vector(1.5, 0.5, 4), colour(0.5, 1, 0.75))]
    if far_object == "wall":
        far = plane(vector(0, 0, -1), 2 ** 19, _refl(next(m), 0.75))
    else:
        far = triangle(vector(2 ** 20, -2 ** 22, 2 ** 19), vector(-2 ** 20, -2 ** 22, 2 ** 19), vector(0, 2 ** 22, 2 ** 19),
                       next(m))
    return _scene([far] + [sphere(1, vector(*c), next(m)) for c in PENCIL_SPHERES], _camera(2.0 ** -10), lights)


# ---- many spheres and flat objects -------------------------------------------------------------------
def big_flat():
    """S160 with the corridor's planes and the small mesh before its first sphere: the sphere BVH
    and the 16-cell occluder masks with flat objects present."""
    sc = H.base("s160")
    k = next(i for i, t in enumerate(sc) if H._is_obj(t))
    return H.unit_powers(sc[:k] + corridor_planes() + mesh_triangles(2, 2) + sc[k:])


def empty():
    return _scene([])


SCENES = {
    "corridor": (corridor, 8),
    "corridor_nonunit": (corridor_nonunit, 6),
    "mirror_nonunit": (mirror_nonunit, 5),
    "planes_only": (planes_only, 8),
    "tris_only": (tris_only, 5),
    "empty": (empty, 3),
    "tie3_tps": (lambda: tie3("tps"), 5),
    "tie3_pst": (lambda: tie3("pst"), 5),
    "tie3_stp": (lambda: tie3("stp"), 5),
    "mesh": (mesh, 5),
    "mesh_small": (mesh_small, 5),
    "behind_facing": (lambda: behind(True), 3),
    "behind_away": (lambda: behind(False), 3),
    "zero_normal": (zero_normal, 5),
    "graze12": (lambda: graze(12), 5),
    "graze16": (lambda: graze(16), 5),
    "pencil_wall": (lambda: pencil("wall"), 4),
    "pencil_fartri": (lambda: pencil("tri"), 4),
    "big_flat": (big_flat, 4),
}
NAMES = tuple(SCENES)
assert not set(SCENES) & set(H.SCENES)  # one cache of oracle frames, keyed by name


def build(name):
    return SCENES[name][0]()


def depth(name):
    return SCENES[name][1]


def oracle_ref(O, name, w, h, spp=1, seed=0):
    """hostile.oracle_ref's shared, read-only (frame, levels), for the scenes of this module."""
    return H.oracle_ref(O, name, w, h, spp=spp, seed=seed, scenes=SCENES)
