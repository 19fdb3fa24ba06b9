"""The reference for rt_launch_attrs (RT_ATTRIBUTES in include/rt_mi355x.h), composed of the C
oracle's own exports: for pixel (x, y)

    d = shoot_ray(Camera.location, point_on_screen(Camera, X, Y))     raytracer.erl:486-511
    nearest(Scene, Camera.location, d)                                :300-346

over the whole marshalled array (elements that are not objects never intersect, so the index the
oracle returns is the index in the scene list), the albedo read from that element's material.
With spp > 1, X and Y are the jittered sample position of RT_SUPERSAMPLING, restated here in Python
integers and binary64.  A frame is computed once per (scene, size, spp, seed, sample) and is
read-only.
"""
import functools

import numpy as np

from eraytracer_amd import _native as N
from eraytracer_amd import records, scenes

M64 = (1 << 64) - 1
PLANES = ("elem", "t", "point", "normal", "albedo")


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_xy(x, y, width, height, spp=1, seed=0, sample=0):
    """(X, Y) of sample `sample` of pixel (x, y) of the width x height image (RT_SUPERSAMPLING);
    spp = 1 is the reference's (x / width, y / height)."""
    if spp == 1:
        return x / width, y / height
    r = splitmix64(seed ^ (((y * width + x) * spp + sample) & M64))
    u, v = (r >> 40) * 2.0 ** -24, ((r >> 16) & 0xFFFFFF) * 2.0 ** -24
    return (x + u) / width, (y + v) / height


def scene_of(name):
    """"default" (records.scene()), a name of scenes.named, or a name of tests/hostile.py or
    tests/hostile_flat.py."""
    from tests import hostile, hostile_flat
    if name == "default":
        return records.scene()
    if name in hostile_flat.NAMES:
        return hostile_flat.build(name)
    return hostile.build(name) if name in hostile.NAMES else scenes.named(name)


def material_colour(elem):
    u = {N.RT_SPHERE: elem.u.sphere, N.RT_TRIANGLE: elem.u.triangle, N.RT_PLANE: elem.u.plane}[elem.kind]
    c = u.material.colour
    return c.x, c.y, c.z


def attrs_of(elems, width, height, spp=1, seed=0, sample=0, ties=False):
    """The five planes of the whole width x height frame as a dict of arrays (and, with ties, under
    "ties" a bool plane: a second object is hit at exactly the nearest one's distance)."""
    from oracle import oracle as O
    O.build()
    cam = elems[0]
    loc = (cam.u.camera.location.x, cam.u.camera.location.y, cam.u.camera.location.z)
    out = {"elem": np.full((height, width), -1, dtype=np.int32), "t": np.full((height, width), np.inf),
           "point": np.zeros((height, width, 3)), "normal": np.zeros((height, width, 3)),
           "albedo": np.zeros((height, width, 3))}
    objs = [i for i in range(len(elems)) if elems[i].kind in (N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE)]
    tie = np.zeros((height, width), dtype=bool)
    for y in range(height):
        for x in range(width):
            X, Y = sample_xy(x, y, width, height, spp, seed, sample)
            d = O.shoot_ray(loc, O.point_on_screen(cam, X, Y))
            hit = O.nearest(elems, loc, d)
            if hit is None:
                continue
            i, t, point, normal = hit
            out["elem"][y, x] = i
            out["t"][y, x] = t
            out["point"][y, x] = point
            out["normal"][y, x] = normal
            out["albedo"][y, x] = material_colour(elems[i])
            if ties:
                for j in objs:
                    if j != i:
                        other = O.intersect(elems[j], loc, d)
                        if other is not None and other[0] == t:
                            tie[y, x] = True
                            break
    if ties:
        out["ties"] = tie
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame(name, width, height, spp=1, seed=0, sample=0, ties=False):
    return attrs_of(N.marshal(scene_of(name)), width, height, spp, seed, sample, ties)


def kinds(name, ref):
    """(misses, sphere hits, triangle hits, plane hits, distinct objects hit) of a reference frame."""
    el = N.marshal(scene_of(name))
    kind = np.array([e.kind for e in el], dtype=np.int32)
    e = ref["elem"]
    k = kind[np.where(e >= 0, e, 0)]
    hit = e >= 0
    return (int((~hit).sum()), int((hit & (k == N.RT_SPHERE)).sum()), int((hit & (k == N.RT_TRIANGLE)).sum()),
            int((hit & (k == N.RT_PLANE)).sum()), len(set(e[hit].tolist())))
