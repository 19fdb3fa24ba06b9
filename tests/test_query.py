"""Ray queries (RT_QUERY in include/rt_mi355x.h) on the CPU: the header's declarations and the export
list, the argument checks of rt_query_rays and rt_query_shadow (all made before any HIP call and
before the context is read, so no device is needed), the checks of raytracer.nearest_hits and
raytracer.shadow_factors (made before the library is loaded), and the population of every batch
tests/test_gpu_query.py sends, on the reference alone: the GPU comparisons cannot pass on empty ground."""
import ctypes
import os
import re

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer, records
from tests import query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_mi355x.h")
A8 = 0x10000  # a pointer never dereferenced, aligned for everything


def test_header_declares_the_queries():
    src = open(HEADER).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert re.search(r"#define\s+RT_QUERY_ONE_ORIGIN\s+1\b", src) and N.RT_QUERY_ONE_ORIGIN == 1
    assert re.search(r"#define\s+RT_MAX_QUERY_RAYS\s+\(1u << 30\)", src) and N.RT_MAX_QUERY_RAYS == 1 << 30
    assert "RT_QUERY" in re.sub(r"RT_QUERY_ONE_ORIGIN", "", src)
    want = {"rt_query_rays": ["p", "d_origin", "d_dir", "n", "flags", "out", "stream"],
            "rt_query_shadow": ["p", "d_light", "d_hit", "d_elem", "n", "flags", "d_lit", "stream"]}
    for name, names in want.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src)
        assert m, f"the header does not declare {name}"
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
        assert name in N.EXPORTS and not any(ch.isdigit() for ch in name)


def planes(precision=N.RT_OUT_F64, elem=A8, t=A8, point=A8, normal=A8, albedo=A8, struct_size=None):
    size = ctypes.sizeof(N.RtAttrPlanes) if struct_size is None else struct_size
    return N.RtAttrPlanes(size, precision, elem, t, point, normal, albedo)


def rays(L, pl, *, p=A8, o=A8, d=A8, n=100, flags=0):
    return L.rt_query_rays(p, o, d, n, flags, ctypes.byref(pl) if pl is not None else None, None)


def shadow(L, *, p=A8, light=A8, hit=A8, elem=A8, n=100, flags=0, lit=A8):
    return L.rt_query_shadow(p, light, hit, elem, n, flags, lit, None)


def test_argument_checks_need_no_device_and_never_read_the_context(native):
    """Every documented argument error, with a context pointer that is null or would fault if read."""
    L = native.lib()
    bad, big = N.RT_EBADARG, N.RT_ETOOBIG
    assert rays(L, planes(), p=None) == bad
    assert rays(L, planes(), o=None) == bad and rays(L, planes(), d=None) == bad
    assert rays(L, None) == bad
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert rays(L, planes(), flags=flags) == bad, flags
        assert shadow(L, flags=flags) == bad, flags
    for off in (1, 2, 4):
        assert rays(L, planes(), o=A8 + off) == bad and rays(L, planes(), d=A8 + off) == bad
        assert shadow(L, light=A8 + off) == bad and shadow(L, hit=A8 + off) == bad
    assert shadow(L, elem=A8 + 1) == bad and shadow(L, elem=A8 + 2) == bad
    # rt_launch_attrs' plane checks
    last = N.RtAttrPlanes.d_albedo.offset
    for size in (0, 8, last, last + 7):
        assert rays(L, planes(struct_size=size)) == bad, size
    assert rays(L, planes(elem=None, t=None, point=None, normal=None, albedo=None)) == bad
    for prec in (N.RT_OUT_U8, N.RT_OUT_U16, -1, 4):
        assert rays(L, planes(precision=prec)) == bad, prec
    assert rays(L, planes(elem=A8 + 2)) == bad
    for name in ("t", "point", "normal", "albedo"):
        assert rays(L, planes(**{name: A8 + 4})) == bad, name
        assert rays(L, planes(N.RT_OUT_F32, **{name: A8 + 2})) == bad, name
    assert shadow(L, p=None) == bad
    for name in ("light", "hit", "elem", "lit"):
        assert shadow(L, **{name: None}) == bad, name
    for n in (N.RT_MAX_QUERY_RAYS + 1, 1 << 40, (1 << 64) - 1):
        assert rays(L, planes(), n=n) == big, n
        assert shadow(L, n=n) == big, n


def test_an_empty_batch_launches_nothing(native):
    """n = 0 is RT_OK with a context that would fault if read — and still an error with bad arguments."""
    L = native.lib()
    assert rays(L, planes(), n=0) == N.RT_OK
    assert rays(L, planes(N.RT_OUT_F32, t=A8 + 4, elem=None), n=0, flags=N.RT_QUERY_ONE_ORIGIN) == N.RT_OK
    assert shadow(L, n=0) == N.RT_OK and shadow(L, n=0, flags=1, elem=A8 + 4, lit=A8 + 1) == N.RT_OK
    assert rays(L, planes(), n=0, p=None) == N.RT_EBADARG and shadow(L, n=0, lit=None) == N.RT_EBADARG
    assert rays(L, planes(), n=0, flags=2) == N.RT_EBADARG


def boom():
    raise AssertionError("the library was loaded")


O3, D3 = np.zeros(3), np.ones((5, 3))
ROW = np.zeros(3)  # the one row every row of `Huge` below is


@pytest.mark.parametrize("args,kw", [
    ((O3, np.ones(3)), {}), ((O3, np.ones((5, 2))), {}), ((O3, np.ones((5, 3, 1))), {}), ((np.zeros((4, 3)), D3), {}),
    ((np.zeros(2), D3), {}), ((np.zeros((5, 3), dtype=complex), D3), {}), ((O3, np.ones((5, 3), dtype=bool)), {}),
    ((O3, np.array([["a", "b", "c"]])), {}), ((O3, [[1, 2, None]]), {}), ((O3, 3.0), {}),
    ((O3, D3), dict(planes=())), ((O3, D3), dict(planes=("elem", "depth"))), ((O3, D3), dict(planes="elem")),
    ((O3, D3), dict(planes=("t", "t"))), ((O3, D3), dict(planes=(1,))), ((O3, D3), dict(precision="u8")),
    ((O3, D3), dict(precision="f16")), ((O3, D3), dict(device=-1)), ((O3, D3), dict(device=True)),
    ((O3, D3), dict(device=0.0))])
def test_nearest_hits_refuses_bad_arguments_without_the_library(monkeypatch, args, kw):
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):
        raytracer.nearest_hits(*args, records.scene(), **kw)


@pytest.mark.parametrize("args,kw", [
    ((O3, np.ones(3), [1]), {}), ((O3, np.ones((5, 2)), np.zeros(5, int)), {}), ((np.zeros((4, 3)), D3, np.zeros(5, int)), {}),
    ((O3, D3, np.zeros(4, int)), {}), ((O3, D3, np.zeros((5, 1), int)), {}), ((O3, D3, np.zeros(5)), {}),
    ((O3, D3, np.zeros(5, bool)), {}), ((O3, D3, np.full(5, 1 << 31)), {}), ((O3, D3, np.full(5, -(1 << 31) - 1)), {}),
    ((np.zeros(3, dtype=complex), D3, np.zeros(5, int)), {}), ((O3, D3, np.zeros(5, int)), dict(device=-1))])
def test_shadow_factors_refuses_bad_arguments_without_the_library(monkeypatch, args, kw):
    monkeypatch.setattr(N, "lib", boom)
    with pytest.raises(ValueError):
        raytracer.shadow_factors(*args, records.scene(), **kw)


def test_wrappers_check_sizes_and_scenes_without_the_library(monkeypatch):
    monkeypatch.setattr(N, "lib", boom)

    class Huge:  # an (n, 3) array of more rows than the limit, without its memory
        __array_interface__ = {"shape": (N.RT_MAX_QUERY_RAYS + 1, 3), "typestr": "<f8", "version": 3,
                               "data": ROW.__array_interface__["data"], "strides": (0, 8)}
    with pytest.raises(ValueError, match="RT_MAX_QUERY_RAYS"):
        raytracer.nearest_hits(O3, Huge(), records.scene())
    with pytest.raises(ValueError, match="RT_MAX_QUERY_RAYS"):
        raytracer.shadow_factors(O3, Huge(), np.zeros(5, int), records.scene())
    with pytest.raises(ValueError):  # a scene marshal refuses
        raytracer.nearest_hits(O3, D3, records.scene()[1:])
    with pytest.raises(ValueError):
        raytracer.shadow_factors(O3, D3, np.zeros(5, int), records.scene()[1:])
    # an empty batch needs no library either
    got = raytracer.nearest_hits(O3, np.zeros((0, 3)), records.scene(), precision="f32", planes=("elem", "point"))
    assert got["elem"].shape == (0,) and got["elem"].dtype == np.int32
    assert got["point"].shape == (0, 3) and got["point"].dtype == np.float32
    assert raytracer.shadow_factors(O3, np.zeros((0, 3)), np.zeros(0, int), records.scene()).shape == (0,)
    # good arguments pass the checks and reach the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.nearest_hits([0, 0, -2], [[0, 0, 1], [1, 0, 0]], records.scene(), planes=("t", "normal"), precision="f32")
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.nearest_hits(np.zeros((5, 3), dtype=np.float32), np.ones((5, 3), dtype=np.int64), records.scene())
    with pytest.raises(AssertionError, match="the library was loaded"):
        raytracer.shadow_factors(np.zeros((5, 3)), D3, np.arange(5, dtype=np.int16), records.scene())


# ---- the population of the GPU tests' batches, on the reference alone ----------------------------
def finite_but_miss_t(ref):
    hit = ref["elem"] >= 0
    assert all(np.isfinite(ref[n]).all() for n in ("point", "normal", "albedo"))
    assert np.isfinite(ref["t"][hit]).all() and np.isposinf(ref["t"][~hit]).all()
    return hit


def kinds_hit(name, ref):
    kind = np.array([e.kind for e in Q.elems_of(name)])
    hit = ref["elem"] >= 0
    return set(kind[ref["elem"][hit]].tolist())


@pytest.mark.parametrize("name", Q.INCOHERENT_SCENES)
def test_incoherent_batches_hold_what_they_are_chosen_for(name):
    o, d, ref, kind = Q.incoherent(name)
    assert len(d) == Q.N_INCOHERENT and Q.N_INCOHERENT % 64 and o.shape == d.shape == (Q.N_INCOHERENT, 3)
    hit = finite_but_miss_t(ref)
    assert 0.1 <= hit.mean() <= 0.9, hit.mean()
    assert set(kind.tolist()) == {0, 1, 2, 3} and min(np.bincount(kind)) >= Q.N_INCOHERENT // 8
    length = np.linalg.norm(d, axis=1)
    assert 2.0 ** -3 * (1 - 1e-12) <= length.min() < 0.25 and 4 < length.max() <= 2.0 ** 3 * (1 + 1e-12)
    assert np.abs(length * length - 1).min() > 2.0 ** -20, "a direction is a unit vector: it would be in the BVH's domain"
    if name in ("default", "mixed"):
        assert kinds_hit(name, ref) == {N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE}
        assert (ref["t"] < 0).sum() >= 8, "no negative distance (triangles and planes)"
    if name == "s2+ties":
        assert ref["ties"].sum() >= 8
        # ... and the later twin is what a scan that breaks ties the other way would report
        assert len(set(ref["elem"][ref["ties"]].tolist())) >= 2


@pytest.mark.parametrize("name,w,h", Q.CAMERA_FRAMES)
def test_reflection_batches_hold_what_they_are_chosen_for(name, w, h):
    o, d, ref = Q.reflections(name, w, h)
    hit = finite_but_miss_t(ref)
    assert len(d) >= 1000 and 0.1 <= hit.mean() <= 0.9
    if name == "mixed":
        assert kinds_hit(name, ref) == {N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE}


@pytest.mark.parametrize("name", ["s256", "mixed"])
def test_domain_batches_hold_what_they_are_chosen_for(name):
    o, d, ref, checked = Q.domain(name)
    hit = finite_but_miss_t(ref)
    assert checked.all() and len(d) == Q.N_DOMAIN and 0.1 <= hit.mean() <= 0.9
    slots = dict((w, s) for s, w in Q.HOSTILE)
    assert len({s // 64 for s in slots.values()}) == len(slots) and max(slots.values()) < 9 * 64
    mid = sum(Q.scene_box(Q.elems_of(name))) / 2
    assert 0.9e6 < np.linalg.norm(o[slots["far1e6"]] - mid) < 1.1e6 and 0.9e12 < np.linalg.norm(o[slots["far1e12"]] - mid) < 1.1e12
    assert np.isclose(np.linalg.norm(d[slots["tiny"]]), 2.0 ** -30) and np.isclose(np.linalg.norm(d[slots["huge"]]), 2.0 ** 30)
    for a, w in enumerate(("axis_x", "axis_y", "axis_z")):
        assert np.count_nonzero(d[slots[w]]) == 1 and d[slots[w]][a] != 0
    assert not d[slots["zero"]].any() and ref["elem"][slots["zero"]] == -1
    assert ref["elem"][slots["far1e6"]] >= 0 or ref["elem"][slots["far1e12"]] >= 0, "no ray from afar hits"
    # the ordinary rays are unit vectors from inside 4 (ext + 1): whole waves lie in the BVH's domain
    ordinary = np.ones(len(d), dtype=bool)
    ordinary[list(slots.values())] = False
    dd = (d * d).sum(axis=1)
    assert (np.abs(dd[ordinary] - 1) <= 2.0 ** -21).all()
    ext = max(max(abs(c) for c in (e.u.sphere.center.x, e.u.sphere.center.y, e.u.sphere.center.z, e.u.sphere.radius))
              for e in Q.elems_of(name) if e.kind == N.RT_SPHERE)
    if name == "s256":  # (the scene with a BVH; mixed's planes are hit far away)
        assert np.abs(o[ordinary]).max() <= 2 * (ext + 1)
    o2, d2, ref2, checked2 = Q.domain(name, True)
    bad = ~checked2
    assert bad.sum() == len(Q.NONFINITE) and (~np.isfinite(o2[bad]) | ~np.isfinite(d2[bad])).any(axis=1).all()
    assert np.isfinite(o2[checked2]).all() and np.isfinite(d2[checked2]).all()
    assert all(ref2[n][checked2].tobytes() == ref[n][checked2].tobytes() for n in Q.PLANES)
    assert {s // 64 for s, _ in Q.NONFINITE} & set(range(9, 13)), "no non-finite ray in a wave of ordinary rays"


@pytest.mark.parametrize("name,w,h", Q.CAMERA_FRAMES + (("s256", 64, 48),))
def test_shadow_batches_hold_what_they_are_chosen_for(name, w, h):
    L, H, E, lit, parts = Q.shadows(name, w, h, 4 if name == "s256" else 1)
    assert len(parts) == 4 and len(lit) == len(E) == len(H) >= 1000
    assert 0.1 <= lit.mean() <= 0.9, lit.mean()
    for p in parts:
        assert 0 < lit[p].sum() < p.stop - p.start, "a light that sees everything or nothing"


def test_duplicate_batch_has_entries_lit_only_by_the_canon_rule():
    light, H, E, lit, by_index = Q.duplicate_shadows()
    el = Q.elems_of("twins")
    assert el[2].canon == el[4].canon == 2 and bytes(el[2].u) == bytes(el[4].u)
    assert ((lit == 1) & (by_index == 0)).sum() >= 1
    assert not ((lit == 0) & (by_index == 1)).any()
    assert 0.1 <= lit.mean() <= 0.9 and (E == 4).sum() >= 8
