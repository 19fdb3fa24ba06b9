"""rt_query_rays and rt_query_shadow (RT_QUERY in include/rt_mi355x.h) on the GPU, against
tests/query_ref.py — the C oracle's nearest and vec_op composed per ray — in every byte, misses
included, for binary64 planes and, as astype(float32) of the reference, binary32 ones.

Every buffer is pre-filled with a sentinel and has GUARD entries after the n the call is given: they
must keep the sentinel, and a plane that is not asked for is handed over as a null pointer while its
buffer must stay untouched.  tests/test_query.py checks on the CPU that the batches hold what they are
built for.

Which test reaches which instantiation of k_query<PREC, MODE, SCAN> (PREC 0 = binary64, 1 = binary32;
MODE 0 = rays, 1 = shadow, which has PREC 0 only; SCAN 0 = brute force, the header's cull_ok = 0;
1 = wave beams, a scene without a sphere BVH; 2 = a scene with one, each wave walking it or taking the
beam by its rays):
  k_query<0, 0, 1>, k_query<1, 0, 1>  test_camera_rays_equal_the_attribute_pass, test_reflection_rays, and
                                      test_incoherent_rays, test_filters_domain on every scene but s256, far10100
  k_query<0, 0, 2>, k_query<1, 0, 2>  test_incoherent_rays on s256 (no unit direction: every wave takes the
                                      beam) and test_filters_domain on s256 (whole waves of unit directions
                                      from inside the scene walk the BVH; the waves holding a hostile ray
                                      take the beam)
  k_query<0, 0, 0>, k_query<1, 0, 0>  test_incoherent_rays on far10100 (beyond CULL_EXTENT: cull_ok = 0) and
                                      test_brute_force on every scene
  k_query<0, 1, 1>                    test_shadow_queries on mixed and s64, test_duplicate_objects,
                                      test_shadow_edge_cases
  k_query<0, 1, 2>                    test_shadow_queries on s256 (shadow rays are unit vectors)
  k_query<0, 1, 0>                    test_shadow_brute_force
  the walk itself, k_query<.., 2>     tests/test_gpu_query_bvh.py: both BVH memory layouts (nodes and rows staged in
                                      LDS, or read from HBM), trees of depth 10 to 13 and of a few nodes, whole
                                      waves from anywhere in the walk's domain and on its limits, partial and
                                      one-origin waves, the loop iteration after staging, rt_update_scene across
                                      layouts (the CPU restatement of the walk: tests/test_query_bvh.py)
"""
import ctypes
import functools

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer
from tests import attr_ref as A
from tests import query_ref as Q
from tests.test_gpu_primary_tiles import PREC, SENTINEL, TORCH_DT, Ctx

pytestmark = pytest.mark.gpu
GUARD = 64
ELEM_SENTINEL = -7777
LIT_SENTINEL = 0x5A
PLANES = Q.PLANES
NP_DT = {"f32": np.float32, "f64": np.float64}


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_device(a, dtype=None):
    """A C-contiguous copy of a host array (the reference's are read-only) on the device."""
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def query_device(c, d_o, d_d, n, *, one, prec="f64", want=PLANES, skew=0, expect=N.RT_OK):
    """One rt_query_rays of device tensors into sentinel-filled device buffers of n + GUARD entries: the
    dict of all five buffers, and the allocations of the 3-channel ones (skew elements in front)."""
    import torch
    fdt = getattr(torch, TORCH_DT[prec])
    m = n + GUARD
    buf = {"elem": torch.full((m,), ELEM_SENTINEL, dtype=torch.int32, device="cuda"),
           "t": torch.full((m,), SENTINEL, dtype=fdt, device="cuda")}
    keep = []
    for name in ("point", "normal", "albedo"):
        alloc = torch.full((m * 3 + skew,), SENTINEL, dtype=fdt, device="cuda")
        assert alloc.data_ptr() % 16 == 0
        keep.append(alloc)
        buf[name] = alloc[skew:].view(m, 3)
    pl = N.RtAttrPlanes(ctypes.sizeof(N.RtAttrPlanes), PREC[prec], *[buf[k].data_ptr() if k in want else None for k in PLANES])
    rc = c.L.rt_query_rays(c.p, d_o.data_ptr(), d_d.data_ptr(), n, N.RT_QUERY_ONE_ORIGIN if one else 0, ctypes.byref(pl),
                           stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    return buf, keep


def query(c, o, d, *, prec="f64", want=PLANES, skew=0, n=None):
    """rt_query_rays of host arrays (o (n, 3), or (3,) for RT_QUERY_ONE_ORIGIN): the planes asked for,
    n entries each, after checking the guard entries, the planes not asked for and the skew."""
    n = len(d) if n is None else n
    buf, keep = query_device(c, to_device(o), to_device(d), n, one=np.ndim(o) == 1, prec=prec, want=want, skew=skew)
    out = {k: b.cpu().numpy() for k, b in buf.items()}
    assert all(bool((a[:skew] == SENTINEL).all()) for a in keep), "wrote in front of a skewed plane"
    for k in PLANES:
        sent = ELEM_SENTINEL if k == "elem" else SENTINEL
        if k in want:
            assert np.all(out[k][n:] == sent), (k, "entries past n written")
        else:
            assert np.all(out[k] == sent), (k, "a plane not asked for was written")
    return {k: out[k][:n] for k in want}


def expected(ref, prec, k):
    return ref[k] if k == "elem" else np.ascontiguousarray(ref[k].astype(NP_DT[prec]))


def check(got, ref, prec, want=PLANES, what="", sel=None):
    for k in want:
        e, g = expected(ref, prec, k), np.ascontiguousarray(got[k])
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k, g.dtype, g.shape)
        if sel is not None:
            e, g = np.ascontiguousarray(e[sel]), np.ascontiguousarray(g[sel])
        if g.tobytes() != e.tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != e.view(np.uint8).reshape(len(e), -1)).any(axis=1))
            at = (np.arange(len(ref[k])) if sel is None else np.arange(len(ref[k]))[sel])[bad]  # indices in the call
            waves = sorted(set((at // 64).tolist()))  # (a wave: 64 consecutive rays of the call)
            raise AssertionError(f"{what} {k} {prec}: {len(bad)} rays differ, first {at[0]}: {g[bad[0]]!r} against {e[bad[0]]!r}; "
                                 f"in waves {waves}")


def same(a, b, want=PLANES, what=""):
    for k in want:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def gpu_incoherent(name, prec="f64", cull=True):
    """Test 2's batch on a fresh context (computed once, read-only)."""
    o, d, _, _ = Q.incoherent(name)
    with Ctx(Q.scene_of(name), cull=cull) as c:
        got = query(c, o, d, prec=prec)
    for a in got.values():
        a.setflags(write=False)
    return got


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,w,h", Q.CAMERA_FRAMES)
def test_camera_rays_equal_the_attribute_pass(name, w, h, prec):
    """The camera's own rays, built by the oracle: with RT_QUERY_ONE_ORIGIN and with the origin repeated,
    the five planes of rt_launch_attrs and of tests/attr_ref.py."""
    from tests.test_gpu_attrs import image, launch
    loc, d = Q.camera_rays(name, w, h)
    ref = Q.flat(A.frame(name, w, h))
    with Ctx(Q.scene_of(name)) as c:
        one = query(c, loc, d, prec=prec)
        rep = query(c, np.tile(loc, (len(d), 1)), d, prec=prec)
        attrs = Q.flat(image(launch(c, w, h, prec=prec), h))
    check(one, ref, prec, what=f"{name} one origin")
    same(one, rep, what="one origin against a repeated one")
    same(one, attrs, what="against rt_launch_attrs")


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", Q.INCOHERENT_SCENES)
def test_incoherent_rays(name, prec):
    """4133 rays from everywhere to everywhere, directions not normalised."""
    ref = Q.incoherent(name)[2]
    print(name, prec, "hits", int((ref["elem"] >= 0).sum()), "ties", int(ref["ties"].sum()), flush=True)
    check(gpu_incoherent(name, prec), ref, prec, what=name)


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,w,h", Q.CAMERA_FRAMES)
def test_reflection_rays(name, w, h, prec):
    """From every primary hit point along the bounced primary ray: the thresholds at t ~ 0."""
    o, d, ref = Q.reflections(name, w, h)
    with Ctx(Q.scene_of(name)) as c:
        check(query(c, o, d, prec=prec), ref, prec, what=f"{name} reflections")


# ---- 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["s256", "mixed"])
def test_filters_domain(name, prec):
    """Rays outside the filters' domains among ordinary ones: all equal the oracle; with a NaN and an
    infinity in the batch as well, every other ray still does, and the call returns RT_OK."""
    o, d, ref, _ = Q.domain(name)
    o2, d2, ref2, checked = Q.domain(name, True)
    with Ctx(Q.scene_of(name)) as c:
        check(query(c, o, d, prec=prec), ref, prec, what=f"{name} domain")
        check(query(c, o2, d2, prec=prec), ref2, prec, what=f"{name} domain, non-finite rays", sel=checked)


# ---- 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s256", "mixed"])
def test_independence(name):
    """A ray's bytes depend on nothing but the ray: a permutation, two calls on halves split at an odd
    index, and n = 1, 63, 64, 65 give the one call's bytes."""
    o, d, _, _ = Q.incoherent(name)
    whole = gpu_incoherent(name)
    n = len(d)
    perm = np.random.RandomState(5).permutation(n)
    cut = 2067
    with Ctx(Q.scene_of(name)) as c:
        got = query(c, o[perm], d[perm])
        same(got, {k: whole[k][perm] for k in PLANES}, what="permutation")
        a, b = query(c, o[:cut], d[:cut]), query(c, o[cut:], d[cut:])
        same({k: np.concatenate([a[k], b[k]]) for k in PLANES}, whole, what="halves")
        for m in (1, 63, 64, 65):
            same(query(c, o, d, n=m), {k: whole[k][:m] for k in PLANES}, what=f"prefix {m}")
            same(query(c, o[:m], d[:m]), {k: whole[k][:m] for k in PLANES}, what=f"batch of {m}")


# ---- 6 ------------------------------------------------------------------------------------------
def test_grid_stride_loop():
    """3 * 2^20 + 37 rays — more than 8192 blocks of 256 — tiling test 2's batch: the tiling of its
    planes (GPU against GPU), and nothing past n."""
    import torch
    name = "mixed"
    o, d, _, _ = Q.incoherent(name)
    small = gpu_incoherent(name)
    n = 3 * (1 << 20) + 37
    assert n > 8192 * 256
    idx = torch.arange(n, device="cuda") % len(d)
    d_o, d_d = to_device(o)[idx].contiguous(), to_device(d)[idx].contiguous()
    with Ctx(Q.scene_of(name)) as c:
        buf, _ = query_device(c, d_o, d_d, n, one=False)
    for k in PLANES:
        want = to_device(small[k])[idx]
        ibits = torch.int32 if k == "elem" else torch.int64
        assert torch.equal(buf[k][:n].contiguous().view(ibits), want.contiguous().view(ibits)), k
        assert bool((buf[k][n:] == (ELEM_SENTINEL if k == "elem" else SENTINEL)).all()), (k, "entries past n written")


# ---- 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", Q.INCOHERENT_SCENES)
def test_brute_force(name, prec):
    """RT_CFG_CULL = 0 (every object tested) gives the bytes of test 2 ..."""
    same(gpu_incoherent(name, prec), gpu_incoherent(name, prec, cull=False), what=name)


@pytest.mark.parametrize("name", ["s256", "mixed"])
def test_brute_force_reflections_and_domain(name):
    """... and of tests 3 and 4."""
    o, d, ref, _ = Q.domain(name)
    o2, d2, ref2, checked = Q.domain(name, True)
    with Ctx(Q.scene_of(name), cull=False) as c:
        check(query(c, o, d), ref, "f64", what=f"{name} domain, brute force")
        check(query(c, o2, d2), ref2, "f64", what=f"{name} domain, non-finite rays, brute force", sel=checked)
        if name == "mixed":
            for fr in Q.CAMERA_FRAMES[:1]:
                ro, rd, rref = Q.reflections(*fr)
                check(query(c, ro, rd), rref, "f64", what="reflections, brute force")
    if name == "s256":
        ro, rd, rref = Q.reflections(*Q.CAMERA_FRAMES[1])
        with Ctx(Q.scene_of("s64"), cull=False) as c:
            check(query(c, ro, rd), rref, "f64", what="s64 reflections, brute force")


# ---- 8 ------------------------------------------------------------------------------------------
def shadow(c, lights, hits, elems, *, n=None, expect=N.RT_OK):
    """rt_query_shadow of host arrays (lights (n, 3), or (3,) for RT_QUERY_ONE_ORIGIN): n bytes, after
    checking the guard bytes."""
    import torch
    n = len(hits) if n is None else n
    d_l, d_h, d_e = to_device(lights), to_device(hits), to_device(elems, np.int32)
    lit = torch.full((n + GUARD,), LIT_SENTINEL, dtype=torch.uint8, device="cuda")
    rc = c.L.rt_query_shadow(c.p, d_l.data_ptr(), d_h.data_ptr(), d_e.data_ptr(), n,
                             N.RT_QUERY_ONE_ORIGIN if np.ndim(lights) == 1 else 0, lit.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = lit.cpu().numpy()
    assert np.all(out[n:] == LIT_SENTINEL), "bytes past n written"
    return out[:n]


def lit_equal(got, ref, what):
    bad = np.flatnonzero(got != ref)
    assert not len(bad), f"{what}: {len(bad)} of {len(ref)} differ, first {bad[0]}: {got[bad[0]]} against {ref[bad[0]]}"


SHADOW_FRAMES = Q.CAMERA_FRAMES + (("s256", 64, 48),)


def shadow_stride(name):
    return 4 if name == "s256" else 1


@pytest.mark.parametrize("name,w,h", SHADOW_FRAMES)
def test_shadow_queries(name, w, h):
    """Every light against the frame's primary hit points and their elements, in one batch and, with
    RT_QUERY_ONE_ORIGIN, light by light."""
    L, H, E, ref, parts = Q.shadows(name, w, h, shadow_stride(name))
    print(name, len(ref), "lit", int(ref.sum()), flush=True)
    with Ctx(Q.scene_of(name)) as c:
        lit_equal(shadow(c, L, H, E), ref, name)
        for i, p in enumerate(parts):
            lit_equal(shadow(c, L[p.start], H[p], E[p]), ref[p], f"{name} light {i}, one origin")


@pytest.mark.parametrize("name,w,h", SHADOW_FRAMES)
def test_shadow_brute_force(name, w, h):
    L, H, E, ref, _ = Q.shadows(name, w, h, shadow_stride(name))
    with Ctx(Q.scene_of(name), cull=False) as c:
        lit_equal(shadow(c, L, H, E), ref, f"{name} brute force")


def test_duplicate_objects():
    """Two bit-identical spheres: a hit labelled with either element is lit through the other."""
    light, H, E, ref, by_index = Q.duplicate_shadows()
    assert ((ref == 1) & (by_index == 0)).any()
    with Ctx(Q.scene_of("twins")) as c:
        lit_equal(shadow(c, light, H, E), ref, "twins")
        lit_equal(shadow(c, np.tile(light, (len(H), 1)), H, E), ref, "twins, the light repeated")


def test_shadow_edge_cases():
    """d_elem of -1, n_elems, the camera's and a light's index give 0 where the object's own index gives
    1; hit == light (the zero vector) equals the reference."""
    name, w, h = Q.CAMERA_FRAMES[0]
    el = Q.elems_of(name)
    L, H, E, ref, parts = Q.shadows(name, w, h)
    p = parts[0]
    lit = np.flatnonzero(ref[p] == 1)[:200]
    assert len(lit) == 200
    light, hits, elem = L[p.start], H[p][lit], E[p][lit]
    first_light = Q.light_locations(el)[0][0]
    with Ctx(Q.scene_of(name)) as c:
        assert shadow(c, light, hits, elem).all()
        for e in (-1, len(el), len(el) + 1000, 0, first_light, -(1 << 31), (1 << 31) - 1):
            assert not shadow(c, light, hits, np.full(len(hits), e)).any(), e
        # the hit point is the light: vector_normalize/1 gives the zero vector, which hits nothing
        zero = np.tile(light, (len(hits), 1))
        zref = Q.shadow_ref(el, light, zero, elem)
        assert not zref.any()
        lit_equal(shadow(c, light, zero, elem), zref, "hit == light")
        mix_h, mix_e = hits.copy(), elem.copy()
        mix_h[::3] = light
        mix_e[1::3] = -1
        lit_equal(shadow(c, light, mix_h, mix_e), Q.shadow_ref(el, light, mix_h, mix_e), "mixed with ordinary triples")


# ---- 9 ------------------------------------------------------------------------------------------
def test_scene_update():
    """rt_update_scene, then a query, sees the new scene (and its element table)."""
    new = Q.elems_of("default")
    o1, d1, ref1, _ = Q.incoherent("s64")
    o2, d2, ref2, _ = Q.incoherent("default")
    L, H, E, sref, _ = Q.shadows("mixed", 64, 48)
    mixed = Q.elems_of("mixed")
    with Ctx(Q.scene_of("s64")) as c:
        check(query(c, o1, d1), ref1, "f64", what="before the update")
        N.check(c.L.rt_update_scene(c.p, new, len(new)), "rt_update_scene")
        check(query(c, o2, d2), ref2, "f64", what="after the update")
        N.check(c.L.rt_update_scene(c.p, mixed, len(mixed)), "rt_update_scene")
        lit_equal(shadow(c, L[:2000], H[:2000], E[:2000]), sref[:2000], "shadow queries after two updates")
    assert ref1["elem"].max() > len(new) > ref2["elem"].max()


# ---- 10 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,skew", [("f32", 1), ("f32", 3), ("f64", 1)])
def test_unaligned_plane(prec, skew):
    """A 3-channel binary32 plane starting 4 (and 12) bytes into a 16-byte aligned allocation, a
    binary64 one 8 bytes in: the same bytes, and nothing written in front."""
    o, d, _, _ = Q.incoherent("mixed")
    with Ctx(Q.scene_of("mixed")) as c:
        same(query(c, o, d, prec=prec, skew=skew), gpu_incoherent("mixed", prec), what=(prec, skew))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("want", [("elem",), ("t", "normal"), ("point",), ("t", "point", "normal", "albedo")])
def test_plane_subsets(want, prec):
    o, d, _, _ = Q.incoherent("mixed")
    with Ctx(Q.scene_of("mixed")) as c:
        same(query(c, o, d, prec=prec, want=want), gpu_incoherent("mixed", prec), want, what=want)


def test_python_wrappers_are_the_c_path():
    o, d, ref, _ = Q.incoherent("mixed")
    for prec in ("f64", "f32"):
        got = raytracer.nearest_hits(o, d, Q.scene_of("mixed"), precision=prec)
        assert tuple(got) == PLANES
        same(got, gpu_incoherent("mixed", prec), what=prec)
    loc, cd = Q.camera_rays("mixed", 64, 48)
    part = raytracer.nearest_hits(loc.tolist(), cd.astype(np.float64), Q.scene_of("mixed"), planes=("normal", "elem"))
    assert tuple(part) == ("normal", "elem")
    check(part, Q.flat(A.frame("mixed", 64, 48)), "f64", ("normal", "elem"), what="nearest_hits, one origin")
    L, H, E, sref, parts = Q.shadows("mixed", 64, 48)
    got = raytracer.shadow_factors(L, H, E, Q.scene_of("mixed"))
    assert got.dtype == np.uint8 and got.shape == sref.shape
    lit_equal(got, sref, "shadow_factors")
    p = parts[1]
    lit_equal(raytracer.shadow_factors(L[p.start], H[p], E[p].astype(np.int64), Q.scene_of("mixed")), sref[p], "one light")
