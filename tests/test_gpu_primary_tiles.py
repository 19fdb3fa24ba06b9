"""k_primary traces no ray for an 8x16 half-tile whose candidate-sphere masks (k_pmask) are all zero,
and writes a 16x16 tile with two such halves with 16-byte stores when the pass writes the frame
itself and every row starts on a 16-byte boundary.  Neither may change a bit of any frame, write
outside the image's rows and columns, or disturb the per-tile counts the later kernels read.

The yardstick is the same launch with brute-force scans (rt_configure(RT_CFG_CULL, 0): no masks, so
no half-tile is ever taken for empty): output and levels, pre-filled with a sentinel, must agree
byte for byte over the whole buffer, padding and guard rows included.  On the sphere scenes the C
oracle's levels say which pixels are background: those must be +0.0, sign bit included, and the
frames used here must have both kinds of 16x16 tile (25-75 % without a hit pixel).
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import scenes
from eraytracer_amd.records import camera, colour, material, point_light, screen, sphere, vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, LV_SENTINEL = 12345.0, 77
DEPTH = 5
TORCH_DT = {"f32": "float32", "f64": "float64"}
PREC = {"f32": N.RT_OUT_F32, "f64": N.RT_OUT_F64}


class Ctx:
    """One prepared context; cull=False: brute-force scans."""

    def __init__(self, scene, cull=True, side=None):
        self.L = N.lib()
        el = N.marshal(scene)
        self.p = ctypes.c_void_p()
        N.check(self.L.rt_prepare(el, len(el), 0, ctypes.byref(self.p)), "rt_prepare")
        if side is not None:
            N.check(self.L.rt_configure(self.p, N.RT_CFG_SIDE_STREAMS, side), "rt_configure")
        if not cull:
            N.check(self.L.rt_configure(self.p, N.RT_CFG_CULL, 0), "rt_configure")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.rt_release(self.p)

    def launch(self, w, h, d=DEPTH, *, prec="f32", rb=16, shard=0, nshards=1, spp=1, seed=0, levels=True, guard=0,
               skew=0):
        """The slab of one rt_launch_spp as (values, levels), both pre-filled with a sentinel; `guard`
        more rows after the slab; skew: the output starts that many elements into its allocation
        (the returned values then include the elements before it and as many after)."""
        import torch
        rows = self.L.rt_shard_rows(h, rb, nshards) + guard
        dt = getattr(torch, TORCH_DT[prec])
        flat = torch.full((rows * w * 3 + 2 * skew,), SENTINEL, dtype=dt, device="cuda")
        assert flat.data_ptr() % 16 == 0
        lv = torch.full((rows, w), LV_SENTINEL, dtype=torch.uint8, device="cuda")
        N.check(self.L.rt_launch_spp(self.p, w, h, d, rb, shard, nshards, PREC[prec], N.RT_ORDER_EXACT, spp, seed,
                                     flat.data_ptr() + skew * flat.element_size(), lv.data_ptr() if levels else None,
                                     torch.cuda.current_stream().cuda_stream), "rt_launch_spp")
        torch.cuda.synchronize()
        out = flat.cpu().numpy()
        if skew:
            assert np.all(out[:skew] == SENTINEL) and np.all(out[-skew:] == SENTINEL), "wrote outside a skewed view"
            out = out[skew:-skew]
        return out.reshape(rows, w, 3), lv.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def pair(scene, w, h, d=DEPTH, side=None, **kw):
    """The launch with the filters on, checked against the same launch with brute-force scans: every
    byte of the output and of the levels."""
    with Ctx(scene, side=side) as c, Ctx(scene, cull=False, side=side) as b:
        img, lv = c.launch(w, h, d, **kw)
        ref, rlv = b.launch(w, h, d, **kw)
    assert same(img, ref), (w, h, kw, int((bits(img) != bits(ref)).any(axis=-1).sum()))
    assert np.array_equal(lv, rlv), (w, h, kw, int((lv != rlv).sum()))
    return img, lv


@functools.lru_cache(maxsize=None)
def oracle_levels(name, w, h, d=DEPTH):
    from oracle import oracle as O
    O.build()
    lv = O.render(N.marshal(scene_of(name)), w, h, d, mode=O.MEMO, levels=True)[1]
    lv.setflags(write=False)
    return lv


def empty_share(lv):
    """The share of the frame's 16x16 tiles without a hit pixel."""
    h, w = lv.shape
    tiles = [(lv[y:y + 16, x:x + 16] == 0).all() for y in range(0, h, 16) for x in range(0, w, 16)]
    return sum(tiles) / len(tiles)


def corner_scene(behind=False):
    """Twelve small spheres in the frame's top left corner (or, behind: all of them behind the
    camera, so that no primary ray can reach any), two lights."""
    out = [camera(vector(0, 0, -2), vector(0, 0, 0), 90, screen(4, 3)),
           point_light(colour(1, 1, 1), vector(-10, -8, 0), colour(1, 1, 1)),
           point_light(colour(0.5, 0.75, 1), vector(6, -9, 4), colour(0.25, 1, 0.5))]
    for i in range(12):
        cx, cy, cz = -9.0 + 0.9 * (i % 4), -6.5 + 0.8 * (i // 4), 12.0 + 0.5 * i
        if behind:
            cz = -14.0 - 0.5 * i
        out.append(sphere(0.45 + 0.02 * i, vector(cx, cy, cz),
                          material(colour(0.2 + 0.06 * i, 0.9 - 0.05 * i, 0.5), (1, 4, 20)[i % 3], 0.5, 0.4)))
    return out


def scene_of(name):
    return {"corner": corner_scene, "behind": lambda: corner_scene(True)}.get(name, lambda: scenes.named(name))()


def check_background(name, img, lv, w, h, lo=0.25, hi=0.75):
    """Against the oracle's levels: the frame has both kinds of tile, the launch's levels are the
    oracle's, no sentinel is left inside the image, and every background pixel is +0.0."""
    olv = oracle_levels(name, w, h)
    share = empty_share(olv)
    print(f"{name} {w}x{h}: {share:.3f} of the 16x16 tiles without a hit pixel", flush=True)
    assert lo <= share <= hi, f"{name} {w}x{h}: {share:.3f} of the tiles are empty; the scene generator changed?"
    assert np.array_equal(lv[:h], olv)
    assert not np.any(img[:h] == SENTINEL)
    assert np.all(bits(img[:h])[olv == 0] == 0), "a background pixel that is not +0.0"
    assert np.all(img[h:] == SENTINEL) and np.all(lv[h:] == LV_SENTINEL), "rows past the image written"


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("w,h", [(256, 192), (200, 150), (203, 150)])
def test_alignment_and_edges(w, h, prec):
    """Whole tiles (256x192), a partial last tile column and row (200x150), and rows that do not
    start on 16 bytes (203x150: no wide fill)."""
    img, lv = pair(scenes.s64(), w, h, prec=prec)
    check_background("s64", img, lv, w, h)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_output_view_off_a_16_byte_boundary(prec):
    """The output starts one element (4 or 8 bytes) past a 16-byte boundary: per-pixel stores."""
    img, lv = pair(scenes.s64(), 256, 192, prec=prec, skew=1)
    check_background("s64", img, lv, 256, 192)


@pytest.mark.parametrize("name", ["s256", "s16"])
def test_other_sphere_scenes(name):
    img, lv = pair(scenes.named(name), 256, 192)
    check_background(name, img, lv, 256, 192)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("rb", [16, 5])
def test_only_the_images_rows(rb, prec):
    """A single-shard launch into a buffer of the image's rows followed by guard rows: the slab's
    padding rows (rb 16: rows 150-159) and the guard rows keep their sentinel, no image pixel does."""
    w, h = 200, 150
    img, lv = pair(scenes.s64(), w, h, prec=prec, rb=rb, guard=16)
    assert img.shape[0] >= h + 16
    check_background("s64", img, lv, w, h)


@pytest.mark.parametrize("nshards,rb", [(2, 16), (3, 16), (2, 7), (3, 7)])
def test_shards(nshards, rb):
    """Every shard's slab equals its brute-force slab, and rt_unshard of the slabs is the
    one-shard frame."""
    import torch
    w, h = 200, 150
    sc = scenes.s64()
    L = N.lib()
    one, one_lv = pair(sc, w, h)
    check_background("s64", one, one_lv, w, h)
    slabs = [pair(sc, w, h, rb=rb, shard=s, nshards=nshards)[0] for s in range(nshards)]
    d_slabs = torch.from_numpy(np.stack(slabs)).cuda()
    d_img = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
    N.check(L.rt_unshard(d_slabs.data_ptr(), w, h, rb, nshards, N.RT_OUT_F32, d_img.data_ptr(),
                         torch.cuda.current_stream().cuda_stream), "rt_unshard")
    torch.cuda.synchronize()
    assert same(d_img.cpu().numpy(), one[:h])


def test_two_frame_geometries_on_one_context():
    """One context renders 200x150, 256x192, three shards and 200x150 again: the masks are rebuilt
    for each, and every frame is a fresh brute-force context's."""
    sc = scenes.s64()
    geoms = [dict(w=200, h=150), dict(w=256, h=192), dict(w=200, h=150, rb=7, shard=1, nshards=3), dict(w=200, h=150)]
    with Ctx(sc) as c:
        got = [c.launch(g["w"], g["h"], **{k: v for k, v in g.items() if k not in "wh"}) for g in geoms]
    with Ctx(sc, cull=False) as b:
        for g, (img, lv) in zip(geoms, got):
            ref, rlv = b.launch(g["w"], g["h"], **{k: v for k, v in g.items() if k not in "wh"})
            assert same(img, ref) and np.array_equal(lv, rlv), g
    check_background("s64", *got[3], 200, 150)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_supersampling_running_sum(prec):
    """Three samples on the path that writes every pixel once (no side streams, no levels): sample 0
    writes the running sum, sample 1 leaves a background pixel alone, sample 2 reads and divides."""
    img, _ = pair(scenes.s64(), 200, 150, side=0, prec=prec, spp=3, seed=0x5EED0003, levels=False)
    assert not np.any(img[:150] == SENTINEL) and np.all(img[150:] == SENTINEL)
    assert np.any(bits(img[:150]) == 0) and np.any(img[:150] > 0)


def test_supersampling_sample_slab():
    """Four samples of S256 with side streams (each pass writes a binary64 sample slab)."""
    img, lv = pair(scenes.s256(), 256, 192, spp=4, seed=0x5EED0004)
    assert not np.any(img == SENTINEL) and not np.any(lv == LV_SENTINEL)


def test_levels_and_hit_mask():
    """Per-pixel level counts (above: every case asks for them) and the primary-hit mask of
    RT_LEVELS_HIT: 0 on every background pixel, nothing left unwritten inside the image."""
    from eraytracer_amd.raytracer import render
    w, h = 200, 150
    sc = scenes.s64()
    olv = oracle_levels("s64", w, h)
    img, lv = pair(sc, w, h, prec="f64")
    out = np.full((h, w, 3), SENTINEL)
    got, hit = render(w, h, sc, DEPTH, levels="hit", out=out)
    assert np.array_equal(hit, (olv > 0).astype(np.uint8))
    assert same(got, img[:h])


_CHILD = r"""
import numpy as np
from eraytracer_amd import _native as N, scenes
from tests.test_gpu_primary_tiles import Ctx, pair, SENTINEL, LV_SENTINEL
w, h = 200, 150
for name in ('mixed', 'default'):
    sc = scenes.named(name)
    with Ctx(sc) as c:
        assert c.L.rt_engine(c.p, 1) == N.RT_ENGINE_WAVE
    for prec in ('f32', 'f64'):
        img, lv = pair(sc, w, h, prec=prec, guard=16)
        assert not np.any(img[:h] == SENTINEL) and np.all(img[h:] == SENTINEL)
        assert not np.any(lv[:h] == LV_SENTINEL) and np.all(lv[h:] == LV_SENTINEL)
        print(name, prec, 'pixels hit', int((lv[:h] > 0).sum()), flush=True)
        assert int((lv[:h] > 0).sum()) > w * h // 3  # the planes fill what no sphere reaches
print('ok')
"""


def test_scenes_with_planes_and_triangles_take_no_shortcut():
    """The mixed scene and the default scene on the wavefront engine (RT_ENGINE is read once per
    process: a child): a plane or a triangle fills tiles that no sphere's mask reaches."""
    e = dict(os.environ, PYTHONPATH=ROOT, RT_ENGINE="wave")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.split(), r.stdout + r.stderr


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_all_empty_and_none_empty(prec):
    """Spheres in one corner (nearly every tile empty), all behind the camera (every tile empty, the
    whole frame +0.0), depth 0 (no ray at all), and a 48x48 frame of S64 (nine tiles, one sphere or
    more in front of each; by the oracle one of them has no hit pixel, so no share is asked of it)."""
    w, h = 200, 150
    img, lv = pair(corner_scene(), w, h, prec=prec)
    check_background("corner", img, lv, w, h, lo=0.75, hi=0.99)
    assert np.any(lv[:h] > 0)
    img, lv = pair(corner_scene(True), w, h, prec=prec)
    check_background("behind", img, lv, w, h, lo=1.0, hi=1.0)
    assert np.all(bits(img[:h]) == 0) and np.all(lv[:h] == 0)
    img, lv = pair(scenes.s64(), w, h, 0, prec=prec)
    assert np.all(bits(img[:h]) == 0) and np.all(lv[:h] == 0) and np.all(img[h:] == SENTINEL)
    img, lv = pair(scenes.s64(), 48, 48, prec=prec)
    check_background("s64", img, lv, 48, 48, lo=0.0, hi=1.0)


def test_four_frames_in_flight():
    """Four FrameRenderer slots (bench.py's arrangement: no side streams, no levels) render the
    frame a single launch gives."""
    import torch

    from eraytracer_amd.dist import FrameRenderer
    w, h = 256, 192
    sc = scenes.s64()
    one, lv = pair(sc, w, h, side=0, levels=False)
    fr = FrameRenderer(sc, w, h, DEPTH, precision="f32", inflight=4)
    try:
        for s in fr.slabs:
            s.fill_(SENTINEL)
        fr.fork()
        for _ in range(8):
            fr.launch()
        fr.join()
        torch.cuda.synchronize()
        frames = [s.cpu().numpy() for s in fr.slabs]
    finally:
        fr.close()
    for f in frames:
        assert same(f, one)
    check_background("s64", one, oracle_levels("s64", w, h), w, h)
