"""The reference for rt_query_rays and rt_query_shadow (RT_QUERY in include/rt_mi355x.h), composed of
the C oracle's own exports, and the seeded batches the GPU tests send.

    rays     nearest(Scene, Origin, Direction)                               raytracer.erl:300-346
             over the whole marshalled array, the albedo read from the element hit (as tests/attr_ref.py)
    shadow   d = vec_op("normalize", vec_op("sub", Hit, Light))              :256-267
             nearest(Scene, Light, d), then `canon` of the element hit against `canon` of element e

Every batch is computed once per process and is read-only; tests/test_query.py checks on the CPU that
each holds what it is built for (hits and misses, every kind of object, ties, lit and unlit entries),
so that the GPU comparisons cannot pass on empty ground.
"""
import ctypes
import functools

import numpy as np

from eraytracer_amd import _native as N
from eraytracer_amd.records import camera, colour, material, point_light, screen, sphere, vector
from tests import attr_ref as A

PLANES = A.PLANES
OBJECTS = (N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE)
N_INCOHERENT = 4133  # not a multiple of 64 or 256
INCOHERENT_SCENES = ("default", "mixed", "s64", "s2+ties", "s256", "far10100")
CAMERA_FRAMES = (("mixed", 64, 48), ("s64", 96, 96))


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def _freeze(d):
    for a in (d.values() if isinstance(d, dict) else d):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def elems_of(name):
    return N.marshal(scene_of(name))


def scene_of(name):
    return duplicate_scene() if name == "twins" else A.scene_of(name)


def nearest_ref(elems, origins, dirs, ties=False):
    """The five planes of n rays as flat arrays (origins (n, 3) or (3,)); with ties also "ties": a second
    object is hit at exactly the nearest one's distance."""
    O = _oracle()
    n = len(dirs)
    out = {"elem": np.full(n, -1, dtype=np.int32), "t": np.full(n, np.inf), "point": np.zeros((n, 3)),
           "normal": np.zeros((n, 3)), "albedo": np.zeros((n, 3))}
    objs = [i for i in range(len(elems)) if elems[i].kind in OBJECTS]
    tie = np.zeros(n, dtype=bool)
    for k in range(n):
        o = tuple(origins) if np.ndim(origins) == 1 else tuple(origins[k])
        d = tuple(dirs[k])
        hit = O.nearest(elems, o, d)
        if hit is None:
            continue
        i, t, point, normal = hit
        out["elem"][k] = i
        out["t"][k] = t
        out["point"][k] = point
        out["normal"][k] = normal
        out["albedo"][k] = A.material_colour(elems[i])
        if ties:
            for j in objs:
                if j != i:
                    other = O.intersect(elems[j], o, d)
                    if other is not None and other[0] == t:
                        tie[k] = True
                        break
    if ties:
        out["ties"] = tie
    return _freeze(out)


def canon_roots(elems):
    """canon of every element after rt_scene_canon, chains resolved."""
    n = len(elems)
    copy = (N.RtElem * n)()
    ctypes.memmove(copy, elems, ctypes.sizeof(copy))
    N.check(N.lib().rt_scene_canon(copy, n), "rt_scene_canon")
    roots = []
    for i in range(n):
        j = i
        while copy[j].canon >= 0 and copy[j].canon != j:
            j = copy[j].canon
        roots.append(j)
    return roots


def shadow_ref(elems, lights, hits, elem_idx):
    """shadow_factor/4 for n triples (lights (n, 3) or (3,)): a uint8 array."""
    O = _oracle()
    roots = canon_roots(elems)
    n = len(hits)
    lit = np.zeros(n, dtype=np.uint8)
    for k in range(n):
        light = tuple(lights) if np.ndim(lights) == 1 else tuple(lights[k])
        d = O.vec_op("normalize", O.vec_op("sub", tuple(hits[k]), light))
        hit = O.nearest(elems, light, d)
        e = int(elem_idx[k])
        if hit is None or not 0 <= e < len(elems) or elems[e].kind not in OBJECTS:
            continue
        lit[k] = 1 if roots[hit[0]] == roots[e] else 0
    lit.setflags(write=False)
    return lit


# ---- test 1: camera rays -------------------------------------------------------------------------
def cam_location(elems):
    c = elems[0].u.camera.location
    return np.array([c.x, c.y, c.z])


@functools.lru_cache(maxsize=None)
def camera_rays(name, w, h):
    """(origin (3,), directions (w*h, 3)), row-major: the rays rt_launch_attrs traces at spp = 1."""
    O = _oracle()
    el = elems_of(name)
    loc = cam_location(el)
    d = np.empty((h * w, 3))
    for y in range(h):
        for x in range(w):
            d[y * w + x] = O.shoot_ray(tuple(loc), O.point_on_screen(el[0], x / w, y / h))
    return _freeze((loc, d))


def flat(frame):
    """A frame of tests/attr_ref.py as flat planes."""
    return {n: np.ascontiguousarray(frame[n].reshape((-1,) + frame[n].shape[2:])) for n in PLANES}


def surface_frame(name):
    """The frame whose hit points serve as on-surface origins for scene `name`."""
    return (name, 96, 96) if name == "s64" else (name, 64, 48)


# ---- test 2: incoherent rays ---------------------------------------------------------------------
def scene_box(elems):
    """(lo, hi) of the spheres' boxes and the triangles' vertices."""
    pts = []
    for e in elems:
        if e.kind == N.RT_SPHERE:
            c, r = e.u.sphere.center, abs(e.u.sphere.radius)
            pts += [(c.x - r, c.y - r, c.z - r), (c.x + r, c.y + r, c.z + r)]
        elif e.kind == N.RT_TRIANGLE:
            pts += [(v.x, v.y, v.z) for v in (e.u.triangle.v1, e.u.triangle.v2, e.u.triangle.v3)]
    p = np.array(pts)
    return p.min(axis=0), p.max(axis=0)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


SEEDS = {"default": 11, "mixed": 12, "s64": 13, "s2+ties": 14, "s256": 15, "far10100": 16}


def mixed_origins(name, rng, n):
    """A seeded mix of origins: inside the scene's box, on object surfaces (hit points of the scene's
    camera frame), inside spheres, and outside the box."""
    el = elems_of(name)
    lo, hi = scene_box(el)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    kind = rng.randint(0, 4, size=n)
    o = lo + (hi - lo) * rng.uniform(size=(n, 3))  # 0: inside the box
    fr = A.frame(*surface_frame(name))
    pts = fr["point"][fr["elem"] >= 0]
    on = kind == 1
    o[on] = pts[rng.randint(0, len(pts), size=int(on.sum()))]
    sph = [e.u.sphere for e in el if e.kind == N.RT_SPHERE]
    inside = np.flatnonzero(kind == 2)
    for k in inside:
        s = sph[rng.randint(0, len(sph))]
        o[k] = np.array([s.center.x, s.center.y, s.center.z]) + 0.9 * abs(s.radius) * rng.uniform(0, 1) * unit_vectors(rng, 1)[0]
    out = kind == 3
    o[out] = mid + unit_vectors(rng, int(out.sum())) * np.linalg.norm(half) * rng.uniform(1.5, 4.0, size=(int(out.sum()), 1))
    return o, kind


@functools.lru_cache(maxsize=None)
def incoherent(name):
    """(origins, directions, reference planes with "ties", origin kinds) of test 2's batch on `name`:
    N_INCOHERENT rays, the directions random and not normalised, lengths in [2^-3, 2^3].  Half of the rays
    from outside the box aim at a point inside it (the others mostly miss)."""
    rng = np.random.RandomState(SEEDS[name])
    n = N_INCOHERENT
    o, kind = mixed_origins(name, rng, n)
    d = unit_vectors(rng, n)
    lo, hi = scene_box(elems_of(name))
    aim = (kind == 3) & (rng.uniform(size=n) < 0.5)
    target = lo + (hi - lo) * rng.uniform(size=(n, 3))
    v = target - o
    d[aim] = (v / np.linalg.norm(v, axis=1, keepdims=True))[aim]
    if name == "s2+ties":  # a share of the rays aimed at the twins and at the mirrored pair's plane of symmetry
        k = np.flatnonzero(rng.uniform(size=n) < 0.25)
        tw = np.array([-5.0, -3.0, 14.0]) + 1.5 * rng.uniform(size=(len(k), 1)) * unit_vectors(rng, len(k))
        v = tw - o[k]
        d[k] = v / np.linalg.norm(v, axis=1, keepdims=True)
    d = d * np.exp2(rng.uniform(-3, 3, size=(n, 1)))
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    ref = nearest_ref(elems_of(name), o, d, ties=True)
    return _freeze((o, d, ref, kind))


# ---- test 3: reflection-like rays ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reflections(name, w, h):
    """(origins, directions, reference): from every primary hit point of the frame, the primary ray
    bounced off the hit's normal (vector_bounce_off_plane/2)."""
    O = _oracle()
    fr = flat(A.frame(name, w, h))
    _, prim = camera_rays(name, w, h)
    idx = np.flatnonzero(fr["elem"] >= 0)
    o = np.ascontiguousarray(fr["point"][idx])
    d = np.array([O.vec_op("bounce", tuple(prim[k]), tuple(fr["normal"][k])) for k in idx])
    return _freeze((o, d, nearest_ref(elems_of(name), o, d)))


# ---- test 4: the filters' domain -----------------------------------------------------------------
N_DOMAIN = 64 * 13 + 5
# (slot, what): the hostile rays, spread through the first waves; waves 9 and later hold ordinary rays only
HOSTILE = ((3, "far1e6"), (64 + 17, "far1e12"), (2 * 64 + 40, "tiny"), (3 * 64 + 63, "huge"), (4 * 64, "axis_x"),
           (5 * 64 + 31, "axis_y"), (6 * 64 + 5, "axis_z"), (7 * 64 + 50, "zero"), (8 * 64 + 9, "far1e6_out"))
NONFINITE = ((64 + 1, "nan_dir"), (3 * 64 + 2, "inf_origin"), (9 * 64 + 33, "nan_origin"), (10 * 64 + 7, "inf_dir"))


@functools.lru_cache(maxsize=None)
def domain(name, nonfinite=False):
    """(origins, directions, reference, checked): ordinary rays — unit directions from origins on
    surfaces and inside the scene's box, the BVH's domain — with a handful of rays outside the filters'
    domains spread through the first waves: origins 1e6 and 1e12 from the scene, directions scaled by
    2^-30 and 2^30, axis-parallel directions, a zero direction.  nonfinite: a NaN and an infinity among
    the directions and origins as well; `checked` is False for those rays (their values are unspecified)."""
    rng = np.random.RandomState(SEEDS[name] + 100)
    n = N_DOMAIN
    el = elems_of(name)
    lo, hi = scene_box(el)
    mid = (lo + hi) / 2
    fr = A.frame(*surface_frame(name))
    pts = fr["point"][fr["elem"] >= 0]
    o = lo + (hi - lo) * rng.uniform(size=(n, 3))
    on = rng.uniform(size=n) < 0.5
    o[on] = pts[rng.randint(0, len(pts), size=int(on.sum()))]
    d = unit_vectors(rng, n)
    for slot, what in HOSTILE:
        u = unit_vectors(rng, 1)[0]
        if what in ("far1e6", "far1e12"):  # towards the scene from afar
            o[slot] = mid - u * float(what[3:])
            d[slot] = u
        elif what == "far1e6_out":  # away from it
            o[slot] = mid - u * 1e6
            d[slot] = -u
        elif what == "tiny":
            d[slot] = d[slot] * 2.0 ** -30
        elif what == "huge":
            d[slot] = d[slot] * 2.0 ** 30
        elif what.startswith("axis"):
            a = "xyz".index(what[-1])
            o[slot] = pts[rng.randint(0, len(pts))]
            d[slot] = 0.0
            d[slot, a] = -1.0 if a == 2 else 1.0
        elif what == "zero":
            d[slot] = 0.0
    checked = np.ones(n, dtype=bool)
    od, dd = o.copy(), d.copy()  # what the oracle sees: the non-finite rays replaced
    if nonfinite:
        for slot, what in NONFINITE:
            checked[slot] = False
            if what == "nan_dir":
                d[slot, 1] = np.nan
            elif what == "inf_dir":
                d[slot, 0] = np.inf
            elif what == "nan_origin":
                o[slot, 2] = np.nan
            else:
                o[slot, 0] = np.inf
    ref = nearest_ref(el, od, dd)
    return _freeze((np.ascontiguousarray(o), np.ascontiguousarray(d), ref, checked))


# ---- test 8: shadow queries ----------------------------------------------------------------------
def light_locations(elems):
    return [(i, np.array([e.u.point_light.location.x, e.u.point_light.location.y, e.u.point_light.location.z]))
            for i, e in enumerate(elems) if e.kind == N.RT_POINT_LIGHT]


@functools.lru_cache(maxsize=None)
def shadows(name, w, h, stride=1):
    """Every light of the scene against (every stride-th of) the frame's primary hit points and their
    elements: (lights (m, 3), hits (m, 3), elems (m,), reference (m,), per-light slices)."""
    el = elems_of(name)
    fr = flat(A.frame(name, w, h))
    idx = np.flatnonzero(fr["elem"] >= 0)[::stride]
    hits, elem = fr["point"][idx], fr["elem"][idx]
    L, Hh, E, parts = [], [], [], []
    for _, loc in light_locations(el):
        parts.append(slice(len(L) * len(idx), (len(L) + 1) * len(idx)))
        L.append(np.tile(loc, (len(idx), 1)))
        Hh.append(hits)
        E.append(elem)
    L, Hh, E = np.concatenate(L), np.ascontiguousarray(np.concatenate(Hh)), np.concatenate(E).astype(np.int32)
    return _freeze((L, Hh, E, shadow_ref(el, L, Hh, E))) + (tuple(parts),)


def duplicate_scene():
    """Two bit-identical spheres (elements 2 and 4) around another one, a light that sees them and a
    sphere that shadows part of them: a hit point on the sphere labelled with element 4 is lit only
    because elements 2 and 4 are the same term."""
    m = material(colour(0.5, 0.25, 1), 1, 0.5, 0.25)
    return [camera(vector(0, 0, -2), vector(0, 0, 0), 90, screen(4, 3)),
            point_light(colour(1, 1, 1), vector(-3, -4, 2), colour(1, 1, 1)),
            sphere(1.5, vector(0, 0, 10), m),
            sphere(1, vector(3, 1, 9), material(colour(1, 0.5, 0), 1, 0.5, 0.25)),
            sphere(1.5, vector(0, 0, 10), m),
            sphere(0.75, vector(-0.5, -2, 6), material(colour(0, 0.5, 0), 0, 0.5, 0.25))]


@functools.lru_cache(maxsize=None)
def duplicate_shadows():
    """(lights, hits, elems, reference, by_index): the twins scene's primary hit points, each once with
    the element the camera ray hit and once with its twin's index (2 <-> 4); by_index: what comparing
    list indices instead of terms would answer."""
    el = elems_of("twins")
    fr = flat(A.attrs_of(el, 48, 36))
    idx = np.flatnonzero(fr["elem"] >= 0)
    hits = np.concatenate([fr["point"][idx], fr["point"][idx]])
    e0 = fr["elem"][idx]
    swap = np.where(e0 == 2, 4, np.where(e0 == 4, 2, e0))
    elem = np.concatenate([e0, swap]).astype(np.int32)
    light = light_locations(el)[0][1]
    O = _oracle()
    by_index = np.zeros(len(elem), dtype=np.uint8)
    for k in range(len(elem)):
        d = O.vec_op("normalize", O.vec_op("sub", tuple(hits[k]), tuple(light)))
        hit = O.nearest(el, tuple(light), d)
        by_index[k] = 1 if hit is not None and hit[0] == elem[k] else 0
    return _freeze((light, np.ascontiguousarray(hits), elem, shadow_ref(el, light, hits, elem), by_index))
