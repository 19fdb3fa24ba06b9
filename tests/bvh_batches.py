"""The seeded batches of tests/test_query_bvh.py (CPU) and tests/test_gpu_query_bvh.py (GPU): rays that
put whole waves of k_query<.., SCAN_BVH> on the per-lane BVH walk, up to and just across the limits of
the walk's domain (rt_query.hip, "The BVH's domain"), with the oracle's answer for each.

Every batch is computed once per process and is read-only; tests/test_query_bvh.py checks that each
holds what it is built for.
"""
import functools
import zlib

import numpy as np

from eraytracer_amd import _native as N
from tests import attr_ref as A
from tests import bvh_ref as B
from tests import query_ref as Q

N_RAYS = 64 * 40 + 37
LAYOUT_SCENES = ("s256", "s427", "s428", "s2000")          # staged (<= 427 spheres) and HBM layouts, depths 10 to 13
HOSTILE_SCENES = ("s160+g", "s160+d", "big_flat", "s300l190+g", "lattice")
SPHERE_SCENES = tuple(s for s in LAYOUT_SCENES + HOSTILE_SCENES if s != "big_flat")
TINY_SCENES = ("twins", "s2+ties", "mixed", "default", "s7+g")   # trees only with RT_BVH_MIN=2
TIE_SCENES = ("s2+ties", "s7+g")                           # G's mirrored pair, x = -1 and x = +1
IN_BOX, ON_SURFACE, IN_SPHERE, IN_CUBE = range(4)
# edge(): what was done to a ray
PLAIN, O_IN, O_OUT, D_IN, D_OUT = range(5)
EDITS = {O_IN: "origin on 4E", O_OUT: "origin just past 4E", D_IN: "d.d - 1 just inside 2^-20",
         D_OUT: "d.d - 1 just past 2^-20"}


def seed_of(name, salt=0):
    return (zlib.crc32(name.encode()) + salt) & 0x7fffffff


def spheres_of(name):
    """(centres (m, 3), |radii| (m,)) of the scene's spheres, in list order."""
    sph = [e.u.sphere for e in Q.elems_of(name) if e.kind == N.RT_SPHERE]
    return np.array([[s.center.x, s.center.y, s.center.z] for s in sph]), np.array([abs(s.radius) for s in sph])


def box_of(name):
    """The scene's box (Q.scene_box), cut to the walk's domain."""
    lim = 4.0 * B.domain_E(name)
    lo, hi = Q.scene_box(Q.elems_of(name))
    return np.maximum(lo, -lim), np.minimum(hi, lim)


def aimed(rng, name, o):
    """Unit directions from o towards seeded points of the scene's box."""
    lo, hi = box_of(name)
    v = lo + (hi - lo) * rng.uniform(size=o.shape) - o
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(name, rng, n):
    E = B.domain_E(name)
    lo, hi = box_of(name)
    c, r = spheres_of(name)
    kind = rng.randint(0, 4, size=n)
    o = lo + (hi - lo) * rng.uniform(size=(n, 3))
    k = rng.randint(0, len(c), size=n)
    u = Q.unit_vectors(rng, n)
    on, ins, cube = kind == ON_SURFACE, kind == IN_SPHERE, kind == IN_CUBE
    o[on] = (c[k] + r[k, None] * u)[on]
    o[ins] = (c[k] + 0.9 * r[k, None] * rng.uniform(size=(n, 1)) * u)[ins]
    o[cube] = rng.uniform(-4.0 * E, 4.0 * E, size=(n, 3))[cube]
    d = Q.unit_vectors(rng, n)
    aim = cube | (rng.uniform(size=n) < 0.3)
    d[aim] = aimed(rng, name, o)[aim]
    tri = [e.u.triangle for e in Q.elems_of(name) if e.kind == N.RT_TRIANGLE]
    if tri:  # a quarter of the rays towards a point of a triangle (small meshes are rarely hit by chance)
        v = np.array([[[p.x, p.y, p.z] for p in (t.v1, t.v2, t.v3)] for t in tri])
        at = np.flatnonzero(rng.uniform(size=n) < 0.25)
        w = rng.dirichlet((1.0, 1.0, 1.0), size=len(at))
        to = (v[rng.randint(0, len(v), size=len(at))] * w[:, :, None]).sum(axis=1) - o[at]
        d[at] = to / np.linalg.norm(to, axis=1, keepdims=True)
    return o, d, kind


# ---- batch 1 -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inside4E(name):
    """(origins, directions, reference, origin kinds): N_RAYS unit rays from inside the scene's box, from
    sphere surfaces, from inside spheres and from anywhere in the cube [-4E, 4E]^3 — the last, and 30 % of
    the others, aimed at a point of the box.  Every ray is in the walk's domain."""
    rng = np.random.RandomState(seed_of(name))
    o, d, kind = _rays(name, rng, N_RAYS)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    return Q._freeze((o, d, Q.nearest_ref(Q.elems_of(name), o, d), kind))


def unit_rays(name, n=N_RAYS):
    """Batch-1-style rays without a reference (tiny scenes: E from the scene, as for any other)."""
    rng = np.random.RandomState(seed_of(name, 7))
    o, d, _ = _rays(name, rng, n)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


N_TIES = 640


@functools.lru_cache(maxsize=None)
def tie_rays(name):
    """(origins, directions, reference with "ties"): N_TIES unit rays in the plane x = 0 (o.x = d.x = 0
    exactly) towards G's mirrored pair, spheres of radius 1.5 at (-1, 0, 10) and (1, 0, 10): both are hit
    at the same distance, bit for bit, and list order decides."""
    rng = np.random.RandomState(seed_of(name, 9))
    n = N_TIES
    o = np.stack([np.zeros(n), rng.uniform(-3, 3, n), rng.uniform(-2, 4, n)], axis=1)
    to = np.stack([np.zeros(n), rng.uniform(-1.2, 1.2, n), 10 + rng.uniform(-1.2, 1.2, n)], axis=1) - o
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(to / np.linalg.norm(to, axis=1, keepdims=True))
    return Q._freeze((o, d, Q.nearest_ref(Q.elems_of(name), o, d, ties=True)))


# ---- batch 2 -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge(name):
    """(origins, directions, reference, edits): batch 1 with waves rewritten, by wave index mod 8:
        0  the whole wave: one coordinate of each origin exactly +-4E (in the domain), re-aimed at the box
        1  one ray of the wave: that coordinate nextafter(+-4E) outwards (out), re-aimed
        2  the whole wave: directions scaled by sqrt(1 +- 2^-20 (1 - 2^-10)) (in), signs alternating
        3  one ray of the wave: scaled by sqrt(1 +- 2^-20 (1 + 2^-10)) (out)
    edits: PLAIN or what was done to the ray.  Whether a ray is in the domain is B.in_domain's to say."""
    rng = np.random.RandomState(seed_of(name, 1))
    o, d, _, _ = inside4E(name)
    o, d = o.copy(), d.copy()
    lim = 4.0 * B.domain_E(name)
    edits = np.zeros(len(d), dtype=np.int64)
    for w in range(len(d) // 64):
        lanes = np.arange(w * 64, w * 64 + 64)
        what = w % 8
        if what in (1, 3):
            lanes = lanes[rng.randint(0, 64):][:1]
        if what in (0, 1):
            a = rng.randint(0, 3, size=len(lanes))
            s = np.where(rng.uniform(size=len(lanes)) < 0.5, -1.0, 1.0)
            o[lanes, a] = s * lim if what == 0 else np.nextafter(s * lim, s * np.inf)
            d[lanes] = aimed(rng, name, o[lanes])
            edits[lanes] = O_IN if what == 0 else O_OUT
        elif what in (2, 3):
            s = np.where(np.arange(len(lanes)) % 2 == (w // 8) % 2, -1.0, 1.0)
            eps = 2.0 ** -20 * ((1 - 2.0 ** -10) if what == 2 else (1 + 2.0 ** -10))
            d[lanes] = d[lanes] * np.sqrt(1.0 + s * eps)[:, None]
            edits[lanes] = D_IN if what == 2 else D_OUT
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    return Q._freeze((o, d, Q.nearest_ref(Q.elems_of(name), o, d), edits))


# ---- batch 3 -------------------------------------------------------------------------------------
AXIS_OTHER = (0.0, -0.0, 1e-31, -1e-40)   # below bvh_inv's 1e-30 clamp; d.d == 1 exactly
CENTRE, INSIDE, TANGENT, OUTSIDE = range(4)


@functools.lru_cache(maxsize=None)
def axis():
    """(origins, directions, reference, axes, signs, aims) on the lattice: N_RAYS rays along +-e_a from
    -+4E, past a seeded sphere of the scene: through its centre, r - 2^-10 off it, exactly tangent (disc
    = 0 < 0.001: a miss) and 1.5 r off, the offset along the next axis.  The other two components of the
    direction cycle through AXIS_OTHER."""
    name = "lattice"
    rng = np.random.RandomState(seed_of(name, 2))
    n = N_RAYS
    lim = 4.0 * B.domain_E(name)
    c, r = spheres_of(name)
    k = rng.randint(0, len(c), size=n)
    ax = np.arange(n) % 3
    sg = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    aim = rng.randint(0, 4, size=n)
    off = np.choose(aim, [0.0 * r[k], r[k] - 2.0 ** -10, r[k], 1.5 * r[k]]) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    o = c[k].copy()
    rows = np.arange(n)
    o[rows, (ax + 1) % 3] += off
    o[rows, ax] = -sg * lim
    d = np.empty((n, 3))
    d[rows, (ax + 1) % 3] = np.array(AXIS_OTHER)[(rows // 6) % 4]
    d[rows, (ax + 2) % 3] = np.array(AXIS_OTHER)[(rows // 6 + 1 + rows // 24) % 4]
    d[rows, ax] = sg
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    return Q._freeze((o, d, Q.nearest_ref(Q.elems_of(name), o, d), ax, sg, aim))


# ---- shadow batches ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shadows_s2000():
    """Every light of s2000 against the primary hit points of a 64x48 frame, strided to <= 3000 triples:
    (lights, hits, elems, reference)."""
    fr = Q.flat(A.frame("s2000", 64, 48))
    hits = int((fr["elem"] >= 0).sum())
    lights = len(Q.light_locations(Q.elems_of("s2000")))
    stride = -(-hits * lights // 3000)
    return Q.shadows("s2000", 64, 48, stride)[:4]


@functools.lru_cache(maxsize=None)
def shadows_l190():
    """All 190 lights of s300l190+g against 16 seeded primary hit points each: (lights (3040, 3), hits,
    elems, reference, per-light slices)."""
    name = "s300l190+g"
    rng = np.random.RandomState(seed_of(name, 3))
    el = Q.elems_of(name)
    fr = Q.flat(A.frame(name, 64, 48))
    idx = np.flatnonzero(fr["elem"] >= 0)
    L, H, E, parts = [], [], [], []
    for i, (_, loc) in enumerate(Q.light_locations(el)):
        pick = idx[rng.randint(0, len(idx), size=16)]
        parts.append(slice(16 * i, 16 * i + 16))
        L.append(np.tile(loc, (16, 1)))
        H.append(fr["point"][pick])
        E.append(fr["elem"][pick])
    L, H, E = np.concatenate(L), np.ascontiguousarray(np.concatenate(H)), np.concatenate(E).astype(np.int32)
    return Q._freeze((L, H, E, Q.shadow_ref(el, L, H, E))) + (tuple(parts),)


def twin_elements(name="s160+g"):
    """The list indices of G's spheres of radius 2 at (-5, -3, 14): the first twin, the second (another
    material) and the first one's 2 / 2.0 copy."""
    el = Q.elems_of(name)
    out = [i for i, e in enumerate(el) if e.kind == N.RT_SPHERE and e.u.sphere.radius == 2.0 and
           (e.u.sphere.center.x, e.u.sphere.center.y, e.u.sphere.center.z) == (-5.0, -3.0, 14.0)]
    assert len(out) == 3
    return out


@functools.lru_cache(maxsize=None)
def shadows_twins160():
    """s160+g: every light against hit points on the three coincident spheres (where rays from the lights
    towards seeded points of their surface end on one of them: the first twin, by list order), each
    labelled once with its own element and once with the second twin's or the copy's, as
    Q.duplicate_shadows does: (lights, hits, elems, reference, by_index) — by_index: what comparing list
    indices would answer.  No two of the three are the same term (another material; 2 =/= 2.0), so here
    the two agree: a point on the first twin is not lit through its bit-identical 2.0 copy."""
    name = "s160+g"
    rng = np.random.RandomState(seed_of(name, 4))
    el = Q.elems_of(name)
    tw = twin_elements(name)
    O = Q._oracle()
    c, r = np.array([-5.0, -3.0, 14.0]), 2.0
    pts, own = [], []
    for _, loc in Q.light_locations(el):
        for u in Q.unit_vectors(rng, 96):
            v = c + r * u - loc
            hit = O.nearest(el, tuple(loc), tuple(v / np.linalg.norm(v)))
            if hit is not None and hit[0] in tw:
                pts.append(hit[2])
                own.append(hit[0])
    pts, own = np.array(pts), np.array(own, dtype=np.int32)
    other = np.where(np.arange(len(own)) % 2 == 0, tw[1], tw[2]).astype(np.int32)
    L, H, E = [], [], []
    for _, loc in Q.light_locations(el):
        for lab in (own, other):
            L.append(np.tile(loc, (len(pts), 1)))
            H.append(pts)
            E.append(lab)
    L, H, E = np.concatenate(L), np.ascontiguousarray(np.concatenate(H)), np.concatenate(E)
    by_index = np.zeros(len(E), dtype=np.uint8)
    for j in range(len(E)):
        dj = O.vec_op("normalize", O.vec_op("sub", tuple(H[j]), tuple(L[j])))
        hit = O.nearest(el, tuple(L[j]), dj)
        by_index[j] = 1 if hit is not None and hit[0] == E[j] else 0
    return Q._freeze((L, H, E, Q.shadow_ref(el, L, H, E), by_index))
