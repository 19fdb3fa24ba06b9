"""The reference for rt_query_colours (RT_QUERY in include/rt_mi355x.h) and the batches its tests send.

    arbitrary rays   oracle/erl_restatement.pixel_colour_from_ray(Ray, Scene without its camera, Depth,
                     memo=True) on the Erlang terms (raytracer.erl:186-252), and beside it the number of
                     objects the ray's reflection chain hit, restated here (chain_levels)
    camera rays      the C oracle's render(..., levels=True): fast enough for whole small frames

The batches are tests/query_ref.py's (camera_rays, incoherent, reflections, domain), scenes are named as
in tests/attr_ref.py, with three kinds of variant spelled in the name: "s64~u" is s64 with every specular
power rewritten to 0 or 1 (tests/hostile.unit_powers: compared bit for bit), "default~1" the default
scene with its first light only, "s64~dark" s64 without lights.  The pure-Python restatement is slow, so
it runs on a seeded subset of a batch (N_SUBSET rays, not a multiple of 64); every result is computed
once per process and is read-only.  tests/test_trace.py checks on the CPU that the subsets hold what
they are chosen for.
"""
import functools

import numpy as np

from eraytracer_amd import _native as N
from oracle import erl_restatement as E
from tests import attr_ref as A
from tests import query_ref as Q

N_SUBSET = 550  # not a multiple of 64 (nor is SUBSET_SIZE's 1100)
INCOHERENT = ("default", "mixed", "s64~u", "s2+ties")  # test 2's scenes
INCOHERENT_DEPTH = 4
CAMERA_FRAMES = (("mixed", 64, 48, 5), ("s64", 96, 96, 5), ("default", 64, 48, 8))


def base_of(name):
    return name.split("~")[0]


def scene_of(name):
    """The scene list (Erlang terms) of a name, variants included."""
    from tests import hostile
    base, _, var = name.partition("~")
    sc = Q.scene_of(base)
    if var == "u":
        return hostile.unit_powers(sc)
    if var == "dark":
        return [t for t in sc if t[0] != "point_light"]
    if var == "1":
        first = [i for i, t in enumerate(sc) if t[0] == "point_light"][0]
        return [t for i, t in enumerate(sc) if t[0] != "point_light" or i == first]
    assert not var, name
    return sc


def unit_powers(name):
    """Every specular power of the scene is 0 or 1: no pow rounding, the comparison is bit for bit."""
    return all(t[-1][2] in (0, 1) for t in scene_of(name) if t[0] in ("sphere", "triangle", "plane"))


def n_lights(name):
    return sum(1 for t in scene_of(name) if t[0] == "point_light")


@functools.lru_cache(maxsize=None)
def elems_of(name):
    return N.marshal(scene_of(name))


def _ray(o, d):
    return ("ray", ("vector",) + tuple(float(v) for v in o), ("vector",) + tuple(float(v) for v in d))


def chain_levels(ray, scene, depth):
    """The number of objects the reflection chain of `ray` hits: rt_launch's levels.  The reflection is
    asked for inside the fold over the lights (:232), so a scene without lights stops after one."""
    lights = any(isinstance(t, tuple) and t and t[0] == "point_light" for t in scene)
    n = 0
    while n < depth:
        r = E.nearest_object_intersecting_ray(ray, scene)
        if r is None:
            break
        n += 1
        if not lights:
            break
        ray = ("ray", r[2], E.vector_bounce_off_plane(ray[2], r[3]))
    return min(n, 255)


def restate(scene, origins, dirs, depth, idx, levels=True):
    """(colours (len(idx), 3), levels (len(idx),)) of rays idx of a batch (origins (n, 3) or (3,))."""
    rest = scene[1:]  # trace_ray_through_pixel/3 hands the scene's tail on (:180-184)
    rgb = np.zeros((len(idx), 3))
    lv = np.zeros(len(idx), dtype=np.uint8)
    for m, k in enumerate(idx):
        ray = _ray(origins if np.ndim(origins) == 1 else origins[k], dirs[k])
        c = E.pixel_colour_from_ray(ray, rest, depth, True)
        rgb[m] = [float(c[1]), float(c[2]), float(c[3])]
        if levels:
            lv[m] = chain_levels(ray, rest, depth)
    rgb.setflags(write=False)
    lv.setflags(write=False)
    return rgb, lv


# (seeds chosen on the reference alone so that each subset holds what tests/test_trace.py asks of it:
# chains of length 3 are rare among incoherent rays, 25 of the 4133 in s2+ties)
SUBSET_SEED = {"default": 21, "mixed": 22, "s64": 52, "s2+ties": 155}
# s64 gets twice the rays: a reflection changes the colour of only 93 of its 4133 (most chains of its
# incoherent rays run inside a sphere, in the dark)
SUBSET_SIZE = {"s64": 1100}


@functools.lru_cache(maxsize=None)
def subset(name):
    """The sorted indices of the restatement subset of Q.incoherent(base of name)."""
    rng = np.random.RandomState(SUBSET_SEED[base_of(name)])
    n = SUBSET_SIZE.get(base_of(name), N_SUBSET)
    idx = np.sort(rng.permutation(Q.N_INCOHERENT)[:n])
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def incoherent_ref(name, depth=INCOHERENT_DEPTH):
    """(indices, colours, levels) of the restatement subset of the scene's incoherent batch."""
    o, d, _, _ = Q.incoherent(base_of(name))
    idx = subset(name)
    return (idx,) + restate(scene_of(name), o, d, depth, idx)


@functools.lru_cache(maxsize=None)
def incoherent_unshadowed(name, depth=INCOHERENT_DEPTH):
    """The subset's colours with every shadow factor forced to 1 (non-vacuity: shadows matter)."""
    o, d, _, _ = Q.incoherent(base_of(name))
    keep = E.shadow_factor
    E.shadow_factor = lambda *a: 1
    try:
        return restate(scene_of(name), o, d, depth, subset(name), levels=False)[0]
    finally:
        E.shadow_factor = keep


@functools.lru_cache(maxsize=None)
def incoherent_depth1(name):
    o, d, _, _ = Q.incoherent(base_of(name))
    return restate(scene_of(name), o, d, 1, subset(name), levels=False)[0]


@functools.lru_cache(maxsize=None)
def batch_ref(name, kind, depth, count, seed=0):
    """(indices, colours, levels): `count` seeded rays of another batch of tests/query_ref.py —
    kind "reflections" (of the 48x36 frame), "domain", "unit" (tests/bvh_batches.unit_rays) or "camera" (of
    the 64x48 frame)."""
    o, d = batch(name, kind)
    rng = np.random.RandomState(1000 + seed)
    idx = np.sort(rng.permutation(len(d))[:count])
    idx.setflags(write=False)
    return (idx,) + restate(scene_of(name), o, d, depth, idx)


def batch(name, kind):
    base = base_of(name)
    if kind == "reflections":
        o, d, _ = Q.reflections(base, 48, 36)
    elif kind == "domain":
        o, d, _, _ = Q.domain(base)
    elif kind == "camera":
        o, d = Q.camera_rays(base, 64, 48)
    elif kind == "unit":  # unit rays from inside 4E, whole waves in the BVH walk's domain and a partial one
        from tests import bvh_batches as BB
        o, d = BB.unit_rays(base)
    else:
        o, d, _, _ = Q.incoherent(base)
    return o, d


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, depth):
    """The C oracle's (frame (h, w, 3), levels (h, w)) of the scene's own camera."""
    from oracle import oracle as O
    O.build()
    img, lv = O.render(elems_of(name), w, h, depth, mode=O.MEMO, levels=True)
    img.setflags(write=False)
    lv.setflags(write=False)
    return img, lv


def compare(gpu, ref, name, depth, what=""):
    """The two comparison rules of the GPU tests: unit powers bit for bit; general powers within the
    project's relative bound (tests/dispatch_matrix.colour_bound) and 1e-5."""
    from tests import dispatch_matrix as M
    gpu, ref = np.ascontiguousarray(gpu, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    if unit_powers(name):
        bad = np.flatnonzero((gpu.view(np.int64) != ref.view(np.int64)).reshape(len(gpu), -1).any(axis=1))
        assert not len(bad), f"{what} {name}: {len(bad)} of {len(gpu)} rays differ, first {bad[0]}: {gpu[bad[0]]!r} against {ref[bad[0]]!r}"
        return
    worst, bad = M.colour_excess(gpu, ref, n_lights(name), depth)
    delta = float(np.abs(gpu - ref).max()) if gpu.size else 0.0
    print(f"{what} {name}: worst {worst:.2f} x 2^-52 (bound {M.colour_bound(n_lights(name), depth) * 2.0 ** 52:.0f}), max |d| {delta:.3g}",
          flush=True)
    assert bad == 0, f"{what} {name}: {bad} channels outside the bound, worst {worst:.2f} x 2^-52"
    assert delta <= 1e-5, (what, name, delta)
