"""rt_launch_attrs (RT_ATTRIBUTES in include/rt_mi355x.h) on the GPU: the five planes of the primary
hit against tests/attr_ref.py — the C oracle's point_on_screen, shoot_ray and nearest composed per
pixel — in every byte, misses included.

Every buffer is pre-filled with a sentinel and has 16 guard rows after the slab: rows past the
window and the guard rows must keep the sentinel, and a plane that is not asked for is handed to
the library as a null pointer while its buffer must stay untouched.

Which test reaches which instantiation of k_attrs<PREC, FAST> (PREC 0 = binary64, 1 = binary32; FAST
= the compiled header's cull_ok, which RT_CFG_CULL = 0 clears):
  k_attrs<0, true>, k_attrs<1, true>    test_planes_equal_the_reference on every frame but far10100
                                        (tests/test_hostile.py pins cull_ok = 1 for them), and every
                                        other test but the two below
  k_attrs<0, false>, k_attrs<1, false>  test_planes_equal_the_reference on far10100 (beyond
                                        CULL_EXTENT: cull_ok = 0), and test_brute_force on every frame
"""
import ctypes
import functools

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer
from tests import attr_ref as A
from tests.test_gpu_primary_tiles import PREC, SENTINEL, TORCH_DT, Ctx

pytestmark = pytest.mark.gpu
GUARD = 16
ELEM_SENTINEL = -7777
PLANES = A.PLANES
FRAMES = [("mixed", 128, 96), ("default", 64, 48), ("s2+ties", 64, 48), ("mixed_int@inside_cloud", 64, 48),
          ("s64", 96, 96), ("far10100", 64, 48)]
NP_DT = {"f32": np.float32, "f64": np.float64}


def launch(c, iw, ih, win=None, *, prec="f64", rb=16, shard=0, nshards=1, spp=1, seed=0, sample=0, want=PLANES,
           expect=N.RT_OK, skew=0):
    """One rt_launch_attrs into sentinel-filled buffers, GUARD rows after each slab: a dict of all
    five buffers (those not in `want` were not handed to the library and must still be sentinel).
    skew: the 3-channel planes start that many elements into their (16-byte aligned) allocations."""
    import torch
    x0, y0, w, h = win or (0, 0, iw, ih)
    rows = c.L.rt_shard_rows(h, rb, nshards) + GUARD
    fdt = getattr(torch, TORCH_DT[prec])
    buf = {"elem": torch.full((rows, w), ELEM_SENTINEL, dtype=torch.int32, device="cuda"),
           "t": torch.full((rows, w), SENTINEL, dtype=fdt, device="cuda")}
    keep = []
    for n in ("point", "normal", "albedo"):
        flat = torch.full((rows * w * 3 + skew,), SENTINEL, dtype=fdt, device="cuda")
        assert flat.data_ptr() % 16 == 0
        keep.append(flat)
        buf[n] = flat[skew:].view(rows, w, 3)
    pl = N.RtAttrPlanes(ctypes.sizeof(N.RtAttrPlanes), PREC[prec], *[buf[n].data_ptr() if n in want else None for n in PLANES])
    rc = c.L.rt_launch_attrs(c.p, iw, ih, x0, y0, w, h, rb, shard, nshards, spp, seed, sample, ctypes.byref(pl),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, win)
    out = {n: b.cpu().numpy() for n, b in buf.items()}
    assert all(bool((f[:skew] == SENTINEL).all()) for f in keep), "wrote in front of a skewed plane"
    for n in PLANES:
        if n not in want:
            assert np.all(out[n] == (ELEM_SENTINEL if n == "elem" else SENTINEL)), (n, "a plane not asked for was written")
    return out


def untouched(a, n):
    return np.all(a == (ELEM_SENTINEL if n == "elem" else SENTINEL))


def image(got, h, want=PLANES):
    """The planes' rows inside the image, after checking that every later row kept its sentinel."""
    for n in want:
        assert untouched(got[n][h:], n), (n, "rows past the window written")
    return {n: got[n][:h] for n in want}


def expected(ref, prec, n):
    return ref[n] if n == "elem" else np.ascontiguousarray(ref[n].astype(NP_DT[prec]))


def check(img, ref, prec, want=PLANES, what=""):
    for n in want:
        e = expected(ref, prec, n)
        g = np.ascontiguousarray(img[n])
        assert g.dtype == e.dtype and g.shape == e.shape, (what, n, g.dtype, g.shape)
        if g.tobytes() != e.tobytes():
            diff = g.view(np.uint8).reshape(g.shape[0], g.shape[1], -1) != e.view(np.uint8).reshape(g.shape[0], g.shape[1], -1)
            bad = np.argwhere(diff.any(axis=-1))
            y, x = bad[0]
            raise AssertionError(f"{what} {n} {prec}: {len(bad)} pixels differ, first at ({x}, {y}): "
                                 f"{g[y, x]!r} against {e[y, x]!r}")


@functools.lru_cache(maxsize=None)
def gpu_frame(name, w, h, prec="f64", cull=True):
    """The whole frame's five planes by one launch on a fresh context (rendered once, read-only)."""
    with Ctx(A.scene_of(name), cull=cull) as c:
        img = image(launch(c, w, h, prec=prec), h)
    for a in img.values():
        a.setflags(write=False)
    return img


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,w,h", FRAMES)
def test_planes_equal_the_reference(name, w, h, prec):
    """All five planes, every byte: elem as int32 with its -1 misses, the binary64 planes as the
    oracle's doubles, the binary32 planes as astype(float32) of them."""
    ref = A.frame(name, w, h)
    img = gpu_frame(name, w, h, prec)
    print(name, w, h, prec, "hits", int((ref["elem"] >= 0).sum()), flush=True)
    check(img, ref, prec, what=name)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,w,h", FRAMES)
def test_brute_force(name, w, h, prec):
    """RT_CFG_CULL = 0 (no beams, every object tested) gives the same bytes."""
    a, b = gpu_frame(name, w, h, prec), gpu_frame(name, w, h, prec, cull=False)
    for n in PLANES:
        assert a[n].tobytes() == b[n].tobytes(), (name, n, prec)


W, H = 200, 150
WINDOWS = [(37, 21, 83, 59), (1, 8, 1, 1), (0, 0, 1, 1), (100, 0, 1, 150)]


def crop(a, win):
    x0, y0, w, h = win
    return np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])


def test_whole_frame_200x150_equals_the_reference():
    check(gpu_frame("s64", W, H), A.frame("s64", W, H), "f64", what="s64 200x150")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("win", WINDOWS)
def test_window_is_the_crop(win, prec):
    full = gpu_frame("s64", W, H, prec)
    with Ctx(A.scene_of("s64")) as c:
        img = image(launch(c, W, H, win, prec=prec), win[3])
    for n in PLANES:
        assert img[n].tobytes() == crop(full[n], win).tobytes(), (win, n, prec)
    ref = A.frame("s64", W, H)
    if win == (1, 8, 1, 1):
        assert img["elem"][0, 0] == ref["elem"][8, 1] >= 1
    if win == (0, 0, 1, 1):
        assert img["elem"][0, 0] == -1 and np.isposinf(img["t"][0, 0]) and not img["albedo"].any()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_shards_reassemble(prec):
    """Three shards of row block 16: the 3-channel planes through rt_unshard, elem and t by the
    shard-row mapping, give the whole frame; slab rows past the image keep their sentinel."""
    import torch
    ns, rb = 3, 16
    full = gpu_frame("s64", W, H, prec)
    with Ctx(A.scene_of("s64")) as c:
        slabs = [launch(c, W, H, prec=prec, rb=rb, shard=s, nshards=ns) for s in range(ns)]
        rows = c.L.rt_shard_rows(H, rb, ns)
        st = torch.cuda.current_stream().cuda_stream
        for n in ("point", "normal", "albedo"):
            for s in range(ns):
                assert untouched(slabs[s][n][rows:], n)
            d_slabs = torch.from_numpy(np.stack([slabs[s][n][:rows] for s in range(ns)])).cuda()
            d_img = torch.full((H, W, 3), SENTINEL, dtype=getattr(torch, TORCH_DT[prec]), device="cuda")
            N.check(c.L.rt_unshard(d_slabs.data_ptr(), W, H, rb, ns, PREC[prec], d_img.data_ptr(), st), "rt_unshard")
            torch.cuda.synchronize()
            assert d_img.cpu().numpy().tobytes() == full[n].tobytes(), (n, prec)
    for n in ("elem", "t"):
        img = np.full((H, W), ELEM_SENTINEL if n == "elem" else SENTINEL, dtype=full[n].dtype)
        for s in range(ns):
            assert untouched(slabs[s][n][rows:], n)
            for r in range(rows):
                g = ((r // rb) * ns + s) * rb + r % rb
                if g < H:
                    img[g] = slabs[s][n][r]
                else:
                    assert untouched(slabs[s][n][r], n), (n, s, r, "a slab row past the image written")
        assert img.tobytes() == full[n].tobytes(), (n, prec)


@pytest.mark.parametrize("sample", [0, 2])
def test_jitter(sample):
    """Sample `sample` of a 3-sample frame: the jittered ray of RT_SUPERSAMPLING."""
    w, h, seed = 64, 48, 0x5EED0003
    ref = A.frame("mixed", w, h, 3, seed, sample)
    with Ctx(A.scene_of("mixed")) as c:
        img = image(launch(c, w, h, spp=3, seed=seed, sample=sample), h)
    check(img, ref, "f64", what=f"mixed spp 3 sample {sample}")
    assert ref["t"].tobytes() != A.frame("mixed", w, h)["t"].tobytes(), "the jittered frame is the unjittered one"


def test_elem_is_the_renderers_hit_mask():
    """mixed 128x96 at depth 1: elem >= 0 exactly where rt_launch_window's levels say the primary ray hit."""
    from tests.test_gpu_window import launch as launch_window
    w, h = 128, 96
    with Ctx(A.scene_of("mixed")) as c:
        lv = launch_window(c, w, h, (0, 0, w, h), 1)[1][:h]
    assert set(np.unique(lv).tolist()) == {0, 1}
    assert np.array_equal(gpu_frame("mixed", w, h)["elem"] >= 0, lv == 1)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("want", [("elem",), ("t", "normal"), ("t", "point", "normal", "albedo")])
def test_plane_subsets(want, prec):
    w, h = 128, 96
    full = gpu_frame("mixed", w, h, prec)
    with Ctx(A.scene_of("mixed")) as c:
        img = image(launch(c, w, h, prec=prec, want=want), h, want)
    for n in want:
        assert img[n].tobytes() == full[n].tobytes(), (want, n, prec)


@pytest.mark.parametrize("prec,skew", [("f64", 1), ("f64", 2), ("f32", 1), ("f32", 3)])
def test_plane_alignment(prec, skew):
    """The 3-channel planes at every alignment the contract allows — a binary64 plane 8 bytes off a
    16-byte boundary (no 16-byte stores) and on one, a binary32 plane 4 and 12 bytes off — and, at
    85 pixels a row, an odd width: the same bytes as the aligned 128x96 frame and its crop."""
    w, h = 128, 96
    full = gpu_frame("mixed", w, h, prec)
    with Ctx(A.scene_of("mixed")) as c:
        img = image(launch(c, w, h, prec=prec, skew=skew), h)
        odd = image(launch(c, w, h, (3, 5, 85, 64), prec=prec, skew=skew), 64)
    for n in PLANES:
        assert img[n].tobytes() == full[n].tobytes(), (n, prec, skew)
        assert odd[n].tobytes() == crop(full[n], (3, 5, 85, 64)).tobytes(), (n, prec, skew)


def test_scene_update():
    """rt_update_scene to a scene with another element count: elem and albedo follow the new list."""
    w, h = 64, 48
    new = N.marshal(A.scene_of("default"))
    assert len(new) != len(N.marshal(A.scene_of("s64")))
    with Ctx(A.scene_of("s64")) as c:
        before = image(launch(c, w, h), h)
        N.check(c.L.rt_update_scene(c.p, new, len(new)), "rt_update_scene")
        after = image(launch(c, w, h), h)
    check(before, A.frame("s64", w, h), "f64", what="before the update")
    check(after, A.frame("default", w, h), "f64", what="after the update")
    assert before["elem"].max() > len(new) > after["elem"].max()


def test_render_attributes_is_the_c_path():
    w, h, win = 128, 96, (5, 3, 100, 77)
    for prec in ("f64", "f32"):
        full = gpu_frame("mixed", w, h, prec)
        got = raytracer.render_attributes(w, h, A.scene_of("mixed"), precision=prec)
        assert tuple(got) == PLANES
        part = raytracer.render_attributes(w, h, A.scene_of("mixed"), precision=prec, window=win, planes=("normal", "elem"))
        assert tuple(part) == ("normal", "elem")
        for n in PLANES:
            assert got[n].dtype == full[n].dtype and got[n].tobytes() == full[n].tobytes(), (n, prec)
        for n in part:
            assert part[n].tobytes() == crop(full[n], win).tobytes(), (n, prec)
    seed = 0x5EED0003
    jit = raytracer.render_attributes(64, 48, A.scene_of("mixed"), spp=3, seed=seed, sample=2)
    check(jit, A.frame("mixed", 64, 48, 3, seed, 2), "f64", what="render_attributes spp 3")


def test_pick():
    """One pixel of each kind, located from the reference: a sphere, a triangle, a plane, a miss."""
    w, h = 64, 48
    scene = A.scene_of("default")
    el = N.marshal(scene)
    ref = A.frame("default", w, h)
    kind = np.array([e.kind for e in el])
    seen = set()
    for k in (N.RT_SPHERE, N.RT_TRIANGLE, N.RT_PLANE, None):
        where = np.argwhere(ref["elem"] < 0 if k is None else (ref["elem"] >= 0) & (kind[np.maximum(ref["elem"], 0)] == k))
        assert len(where), k
        y, x = (int(v) for v in where[len(where) // 2])
        got = raytracer.pick(w, h, x, y, scene)
        if k is None:
            assert got is None
            continue
        i = int(ref["elem"][y, x])
        assert got["elem"] == i and got["term"] is scene[i] and el[i].kind == k
        assert got["t"] == ref["t"][y, x]
        for n in ("point", "normal", "albedo"):
            assert np.array(got[n]).tobytes() == ref[n][y, x].tobytes(), (k, n)
        seen.add(k)
    assert len(seen) == 3
