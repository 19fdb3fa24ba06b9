"""k_primary in two phases: a background phase that streams black over the tiles both of whose halves
have all-zero candidate masks, and a ray phase that strides over the compact list of active tiles
k_pmask builds with the masks (per tile row an offset, then the row's active columns).  Neither may
change a bit of any frame, and the list must follow its masks: complete, free of duplicates, rebuilt
when the scene or the frame geometry changes.

The yardstick is the same launch with brute-force scans (rt_configure(RT_CFG_CULL, 0): no masks, so no
list), byte for byte over the whole sentinel-filled buffer; on S64 also the C oracle.  A tile whose
level-0 count were lost (a zero racing the tile's total) would lose its hits' shading, and a tile
missing from the list would keep its sentinel: both show in the frame.  levels=False takes the
instantiation the benchmark runs (the streamed fill where rows are 16-byte aligned), levels=True the
LEVELS instantiation (per-pixel levels equal to brute force, narrow fill).
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
from tests.test_gpu_primary_tiles import LV_SENTINEL, SENTINEL, Ctx, bits, corner_scene, pair, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (48, 50, 52)  # aligned whole tiles; f32 pitch 600 bytes (no wide fill); aligned, partial last tile
HEIGHTS = (32, 40)     # whole tile rows; a partial last tile row
DEPTHS = (0, 1, 3)


def lit(objs):
    return [camera(vector(0, 0, -2), vector(0, 0, 0), 90, screen(4, 3)),
            point_light(colour(1, 1, 1), vector(-10, -8, 0), colour(1, 1, 1)),
            point_light(colour(0.5, 0.75, 1), vector(6, -9, 4), colour(0.25, 1, 0.5))] + objs


def ball(r, x, y, z, i=0):
    return sphere(r, vector(x, y, z), material(colour(0.2 + 0.05 * i, 0.9 - 0.05 * i, 0.5), (1, 4, 20)[i % 3], 0.5, 0.4))


def filler(i=0):
    """Spheres far behind the camera: they bring the scene to the eight spheres from which beams (and
    with them masks and the list) exist, and no primary ray reaches them."""
    return [ball(0.5, -3.0 + k, 2.0, -30.0 - k, k + i) for k in range(8)]


def one_big():
    """One sphere that fills the view (every tile active), the fillers behind the camera."""
    return lit([ball(40.0, 0, 0, 45.0)] + filler(1))


def one_small(x=-12.0, y=-8.2):
    """One small sphere, by default inside the top left 16x16 tile of a 112 x 72 frame: one active tile."""
    return lit([ball(0.4, x, y, 12.0)] + filler(1))


@functools.lru_cache(maxsize=None)
def oracle_frame(w, h, d):
    from oracle import oracle as O
    O.build()
    img, lv = O.render(N.marshal(scenes.s64()), w, h, d, mode=O.MEMO, levels=True)
    img.setflags(write=False)
    lv.setflags(write=False)
    return img, lv


def both(c, b, w, h, d, **kw):
    """pair() on two resident contexts (c: filters on, b: brute force)."""
    img, lv = c.launch(w, h, d, **kw)
    ref, rlv = b.launch(w, h, d, **kw)
    assert same(img, ref), (w, h, d, kw, int((bits(img) != bits(ref)).any(axis=-1).sum()))
    assert np.array_equal(lv, rlv), (w, h, d, kw, int((lv != rlv).sum()))
    return img, lv


def hit_tiles(lv, h):
    """16x16 tiles of the image's rows with a hit pixel, and all tiles."""
    lv = lv[:h]  # (the slab's padding rows keep their sentinel)
    t = [(lv[y:y + 16, x:x + 16] > 0).any() for y in range(0, h, 16) for x in range(0, lv.shape[1], 16)]
    return sum(t), len(t)


# ---- scenes, widths, heights, precisions, depths ---------------------------------------------------
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["s64", "corner"])
def test_small_rasters(name, prec, levels):
    """S64 and twelve small spheres in a corner at 48/50/52 x 32/40, depths 0, 1 and 3."""
    sc = scenes.s64() if name == "s64" else corner_scene()
    with Ctx(sc) as c, Ctx(sc, cull=False) as b:
        _small_rasters(c, b, name, prec, levels)


def _small_rasters(c, b, name, prec, levels):
    for w in WIDTHS:
        for h in HEIGHTS:
            for d in DEPTHS:
                img, lv = both(c, b, w, h, d, prec=prec, levels=levels)
                assert not np.any(img[:h] == SENTINEL), (w, h, d, "a pixel was never written")
                assert np.all(img[h:] == SENTINEL), (w, h, d, "rows past the image written")
                if name == "s64" and d > 0:
                    ref, rlv = oracle_frame(w, h, d)
                    err = float(np.abs(img[:h].astype(np.float64) - ref).max())
                    assert err <= 1e-5, (w, h, d, err)
                    if levels:
                        assert np.array_equal(lv[:h], rlv), (w, h, d)


# ---- extreme list lengths ---------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_no_tile_every_tile_one_tile(prec, levels):
    """No active tile (every sphere behind the camera: the frame is +0.0), every tile active (one
    sphere fills the view: no pixel is background), and a single sphere in the corner; the last two
    lose pixels if a wholesale zero beats a tile's level-0 total."""
    w, h = 112, 72
    img, lv = pair(corner_scene(True), w, h, 3, prec=prec, levels=levels)
    assert np.all(bits(img[:h]) == 0) and np.all(img[h:] == SENTINEL)
    img, lv = pair(one_big(), w, h, 3, prec=prec, levels=levels)
    assert np.all(img[:h].max(axis=-1) > 0), "a pixel of the sphere that fills the view is black"
    assert np.all(img[h:] == SENTINEL)
    if levels:
        assert np.all(lv[:h] >= 1)
    _, lv = pair(one_small(), w, h, 3, prec=prec, levels=True)
    assert hit_tiles(lv, h) == (1, 35) and (lv[:16, :16] > 0).any()
    img, _ = pair(one_small(), w, h, 3, prec=prec, levels=levels)
    assert np.any(img[:16, :16] > 0) and np.all(img[h:] == SENTINEL)


# ---- grid and list sharing ---------------------------------------------------------------------------
def test_more_tiles_than_blocks():
    """2048 x 1040: 8,320 tiles for a grid of 8,192 blocks, so both phases stride; and twelve small
    spheres in a corner of it: far fewer active tiles than blocks."""
    for sc in (scenes.s64(), corner_scene()):
        img, _ = pair(sc, 2048, 1040, 1, levels=False)
        assert not np.any(img == SENTINEL) and np.any(img > 0)


# ---- geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("nshards,rb", [(2, 8), (2, 16), (3, 8), (3, 16)])
def test_shards(nshards, rb, levels):
    """Every shard's slab, the one with the image's tail row block included (52 x 40, 100 x 70)."""
    with Ctx(scenes.s64()) as c, Ctx(scenes.s64(), cull=False) as b:
        for w, h in ((52, 40), (100, 70)):
            for shard in range(nshards):
                for prec in ("f32", "f64"):
                    both(c, b, w, h, 3, prec=prec, rb=rb, shard=shard, nshards=nshards, levels=levels, guard=16)


@pytest.mark.parametrize("levels", [False, True])
def test_windows_at_odd_origins(levels):
    """Pixel windows of a 200 x 150 image at odd origins, whole and in two shards."""
    from tests.test_gpu_window import launch
    wins = [(37, 21, 52, 40), (1, 3, 48, 32), (139, 101, 60, 49)]
    with Ctx(scenes.s64()) as c, Ctx(scenes.s64(), cull=False) as b:
        for win in wins:
            for prec in ("f32", "f64"):
                for geom in (dict(), dict(rb=8, shard=1, nshards=2)):
                    img, lv = launch(c, 200, 150, win, 3, prec=prec, levels=levels, **geom)
                    ref, rlv = launch(b, 200, 150, win, 3, prec=prec, levels=levels, **geom)
                    assert same(img, ref) and np.array_equal(lv, rlv), (win, prec, geom)


_CHILD = r"""
import ctypes
import numpy as np
from eraytracer_amd import _native as N, scenes
from tests.test_gpu_primary_tiles import Ctx, pair, same, SENTINEL
"""


def _child(body, **env):
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, "-c", _CHILD + body], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout.split(), r.stdout + r.stderr


def test_row_passes():
    """RT_QUEUE_MB=64 (read once per process: a child) at 2048 x 208 depth 5: three row passes of 96,
    96 and 16 rows, each with its own range of the list."""
    _child(r"""
for levels in (False, True):
    img, _ = pair(scenes.s64(), 2048, 208, 5, levels=levels)
    assert not np.any(img == SENTINEL) and np.any(img > 0)
print('ok')
""", RT_QUEUE_MB="64")


# ---- instantiations and modes ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_supersampling_running_sum(prec):
    """Four samples folded into the running sum where each pixel is written (no side streams)."""
    for w, h in ((52, 40), (50, 32)):
        img, _ = pair(scenes.s64(), w, h, 3, side=0, prec=prec, spp=4, seed=0x5EED0004, levels=False)
        assert not np.any(img[:h] == SENTINEL) and np.all(img[h:] == SENTINEL)


@pytest.mark.parametrize("spp", [1, 4])
def test_progressive_first_pass(spp):
    """rt_launch_samples [0, 1): the pass only folds its sample into the binary64 sum (spp 1: one
    sample per pixel with a running sum, so the list with the narrow fill; spp 4: a jittered pass)."""
    from tests.test_gpu_progressive import Sum
    w, h = 52, 40
    for side in (None, 0):
        with Ctx(scenes.s64(), side=side) as c, Ctx(scenes.s64(), cull=False, side=side) as b:
            got = Sum(c, w, h, (0, 0, w, h), 3, spp=spp).add(0, 1).host()
            ref = Sum(b, w, h, (0, 0, w, h), 3, spp=spp).add(0, 1).host()
        assert same(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (spp, side)


# ---- staleness -------------------------------------------------------------------------------------------
def moved(step):
    """The corner sphere of one_small, `step` tiles to the right and down."""
    return one_small(-12.0 + 3.1 * step, -8.2 + 2.3 * step)


def launch_f32(c, w, h, d=3, **kw):
    return c.launch(w, h, d, levels=False, **kw)[0]


def check_list_follows(graph=False):
    """One context: a frame, the sphere moved across tiles by rt_update_scene, a second geometry and
    back; every frame (with graphs: the third of three identical launches, a replay) equals a fresh
    brute-force context's."""
    steps = [(0, 112, 72), (2, 112, 72), (2, 100, 40), (2, 112, 72), (1, 112, 72)]
    with Ctx(moved(0), side=0) as c:
        seen = 0
        for step, w, h in steps:
            if step != seen:
                el = N.marshal(moved(step))
                N.check(c.L.rt_update_scene(c.p, el, len(el)), "rt_update_scene")
                seen = step
            for _ in range(3 if graph else 1):
                img = launch_f32(c, w, h)
            with Ctx(moved(step), cull=False, side=0) as b:
                ref = launch_f32(b, w, h)
            assert same(img, ref), (step, w, h, int((bits(img) != bits(ref)).any(axis=-1).sum()))
            assert np.any(img[:h] > 0), (step, "the sphere is not in the frame")


def test_list_follows_scene_and_geometry():
    check_list_follows()


def test_list_follows_under_frame_graphs():
    """The same with RT_GRAPH=1 (read once per process: a child)."""
    _child(r"""
from tests.test_gpu_primary_list import check_list_follows
check_list_follows(graph=True)
print('ok')
""", RT_GRAPH="1")
