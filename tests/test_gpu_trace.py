"""rt_query_colours (RT_QUERY in include/rt_mi355x.h) on the GPU, against tests/trace_ref.py — the
pure-Python restatement of pixel_colour_from_ray/3 per ray, the C oracle per frame — against
rt_launch_window on the camera's own rays, and against itself on a context with RT_CFG_CULL = 0 (brute
force: the same device arithmetic, so every byte, with general powers too).

Everywhere: scenes whose specular powers are all 0 or 1 are compared with the reference bit for bit,
general powers are held to the project's bound |gpu - ref| <= 2^-52 (2 + 2 (L + 5) D) max(|gpu|, |ref|)
and to 1e-5 (trace_ref.compare), and levels are equal.  d_rgb and d_levels are pre-filled with a
sentinel and have GUARD entries after the n the call is given, which must keep it; the work space is
filled with NaN bytes before every call (its contents are unspecified).  tests/test_trace.py checks on
the CPU that the restatement subsets hold what they are chosen for.

Which test reaches which instantiation of k_trace<PREC, GENPOW, SCAN> (PREC 0 = binary64, 1 = binary32;
GENPOW: the scene has a specular power that is no integer in [0, 1024]; SCAN 0 = brute force, 1 = wave
beams, 2 = a scene with a sphere BVH):
  k_trace<0, 0, 0>  test_incoherent_rays on s64~u and s2+ties (the RT_CFG_CULL = 0 context), test_filters_domain
  k_trace<0, 0, 1>  test_camera_rays_are_the_frame on s64, test_incoherent_rays on s64~u and s2+ties
  k_trace<0, 0, 2>  test_bvh_layouts on s256 and s428
  k_trace<0, 1, 0>  test_incoherent_rays on default and mixed (the RT_CFG_CULL = 0 context)
  k_trace<0, 1, 1>  test_camera_rays_are_the_frame on mixed and default, test_incoherent_rays on them
  k_trace<0, 1, 2>  test_tiny_trees (mixed and default get a BVH under RT_BVH_MIN=2, in a child)
  k_trace<1, g, s>  test_binary32_is_the_rounded_binary64 on the same scenes and contexts, one case per
                    (g, s); <1, 1, 2> in test_tiny_trees' child
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import raytracer
from tests import query_ref as Q
from tests import trace_ref as T
from tests.test_gpu_primary_tiles import PREC, TORCH_DT, Ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL, LV_SENTINEL = 12345.0, 77


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_device(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def trace_device(c, d_o, d_d, n, depth, *, one, prec="f64", levels=True, work=None):
    """One rt_query_colours of device tensors into sentinel-filled buffers of n + GUARD entries:
    (rgb (n + GUARD, 3), levels (n + GUARD,)) as device tensors, after synchronising."""
    import torch
    rgb = torch.full((n + GUARD, 3), SENTINEL, dtype=getattr(torch, TORCH_DT[prec]), device="cuda")
    lv = torch.full((n + GUARD,), LV_SENTINEL, dtype=torch.uint8, device="cuda")
    need = c.L.rt_query_colours_work_bytes(n, depth)
    assert (need > 0) == (n > 0 and depth > 0)
    if work is None and need:
        work = torch.empty((need,), dtype=torch.uint8, device="cuda")
    if need:
        assert work.numel() >= need and work.data_ptr() % 16 == 0
        work[:need].fill_(0xFF)  # NaNs and ids of -1: nothing may be read before it is written
    rc = c.L.rt_query_colours(c.p, d_o.data_ptr(), d_d.data_ptr(), n, depth, N.RT_QUERY_ONE_ORIGIN if one else 0, PREC[prec],
                              rgb.data_ptr(), lv.data_ptr() if levels else None, work.data_ptr() if need else None, need,
                              stream())
    assert rc == N.RT_OK, rc
    torch.cuda.synchronize()
    return rgb, lv


def trace(c, o, d, depth, *, prec="f64", n=None, levels=True, work=None):
    """rt_query_colours of host arrays (o (n, 3), or (3,) for RT_QUERY_ONE_ORIGIN): (rgb (n, 3), levels
    (n,)), after checking the guard entries."""
    n = len(d) if n is None else n
    rgb, lv = trace_device(c, to_device(o), to_device(d), n, depth, one=np.ndim(o) == 1, prec=prec, levels=levels, work=work)
    rgb, lv = rgb.cpu().numpy(), lv.cpu().numpy()
    assert np.all(rgb[n:] == SENTINEL), "colours past n written"
    assert np.all(lv[n:] == LV_SENTINEL) and (levels or np.all(lv == LV_SENTINEL)), "levels past n (or not asked for) written"
    return rgb[:n], lv[:n]


def same(a, b, what=""):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1))
            raise AssertionError(f"{what}: {len(bad)} rays differ, first {bad[0]}: {x[bad[0]]!r} against {y[bad[0]]!r}; "
                                 f"in waves {sorted(set((bad // 64).tolist()))[:20]}")


@functools.lru_cache(maxsize=None)
def gpu_batch(name, kind, depth, prec="f64", cull=True):
    """A whole batch of tests/trace_ref.batch on a fresh context (computed once, read-only)."""
    o, d = T.batch(name, kind)
    with Ctx(T.scene_of(name), cull=cull) as c:
        got = trace(c, o, d, depth, prec=prec)
    for a in got:
        a.setflags(write=False)
    return got


def launch_window(c, w, h, depth):
    """rt_launch_window of the whole frame, binary64, RT_ORDER_EXACT, with levels: ((h*w, 3), (h*w,))."""
    import torch
    rows = c.L.rt_shard_rows(h, 16, 1)
    out = torch.full((rows, w, 3), SENTINEL, dtype=torch.float64, device="cuda")
    lv = torch.full((rows, w), LV_SENTINEL, dtype=torch.uint8, device="cuda")
    N.check(c.L.rt_launch_window(c.p, w, h, depth, 0, 0, w, h, 16, 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, 1, 0,
                                 out.data_ptr(), lv.data_ptr(), stream()), "rt_launch_window")
    torch.cuda.synchronize()
    return out[:h].reshape(h * w, 3).cpu().numpy(), lv[:h].reshape(h * w).cpu().numpy()


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,depth", T.CAMERA_FRAMES)
def test_camera_rays_are_the_frame(name, w, h, depth):
    """The camera's own rays, one origin: every byte of rt_launch_window's frame and levels on a fresh
    context (general powers too: both sides run the device pow), and the C oracle's frame."""
    loc, d = Q.camera_rays(name, w, h)
    with Ctx(T.scene_of(name)) as c:
        rgb, lv = trace(c, loc, d, depth)
    with Ctx(T.scene_of(name)) as c:
        frame, flv = launch_window(c, w, h, depth)
    same((rgb, lv), (frame, flv), f"{name} against rt_launch_window")
    img, olv = T.oracle_frame(name, w, h, depth)
    assert np.array_equal(lv, olv.reshape(-1)) and lv.max() >= min(depth, 3)
    T.compare(rgb, img.reshape(-1, 3), name, depth, "camera rays")


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.INCOHERENT)
def test_incoherent_rays(name):
    """4133 rays from everywhere to everywhere, directions not normalised, depth 4: the restatement on
    its subset, and every ray bit for bit on a context with RT_CFG_CULL = 0."""
    depth = T.INCOHERENT_DEPTH
    rgb, lv = gpu_batch(name, "incoherent", depth)
    idx, ref, rlv = T.incoherent_ref(name)
    assert np.array_equal(lv[idx], rlv), np.flatnonzero(lv[idx] != rlv)[:10]
    T.compare(rgb[idx], ref, name, depth, "incoherent")
    same((rgb, lv), gpu_batch(name, "incoherent", depth, cull=False), f"{name} against brute force")


# ---- 3 ------------------------------------------------------------------------------------------
BVH_DEPTH = 3


@pytest.mark.parametrize("name,kinds", [("s256", ("reflections", "domain")), ("s428", ("reflections", "unit"))])
def test_bvh_layouts(name, kinds):
    """The walk with the nodes staged in LDS (s256) and read from HBM (s428), depth 3, against brute force
    bit for bit: reflection rays, and s256's domain batch (whole waves of unit rays walk, the waves with a
    hostile ray take the beam) or s428's unit rays from inside 4E (every wave walks); both end in a
    partial wave.  128 rays of the second batch against the restatement."""
    for kind in kinds:
        got = gpu_batch(name, kind, BVH_DEPTH)
        same(got, gpu_batch(name, kind, BVH_DEPTH, cull=False), f"{name} {kind} against brute force")
    idx, ref, rlv = T.batch_ref(name, kinds[1], BVH_DEPTH, 128)
    assert np.array_equal(got[1][idx], rlv) and rlv.max() >= 2 and not rlv.all()
    T.compare(got[0][idx], ref, name, BVH_DEPTH, kinds[1])
    assert len(got[1]) % 64, "no partial wave"


_CHILD = r"""
import sys
import numpy as np
from eraytracer_amd import _native as N
from tests import trace_ref as T
from tests.test_gpu_primary_tiles import Ctx
from tests.test_gpu_trace import same, trace
z = np.load(sys.argv[1])
ran = 0
for name in sys.argv[2].split(","):
    o, d = z[name + "|o"], z[name + "|d"]
    with Ctx(T.scene_of(name)) as c:
        for prec in ("f64", "f32"):
            rgb, lv = trace(c, o, d, 3, prec=prec)
            same((rgb, lv), (z[name + "|rgb"].astype(rgb.dtype), z[name + "|lv"]), name + " tiny tree " + prec)
            ran += 1
print("tiny ok", ran)
"""
TINY = ("mixed", "default")


def test_tiny_trees(tmp_path):
    """RT_BVH_MIN=2 RT_BVH_LEVEL=1 (read once per process: a child): mixed and default, scenes with
    triangles, planes and general powers, get a BVH and their unit rays walk it — the brute-force bytes
    of this process, in binary64 and binary32."""
    arrs = {}
    for name in TINY:
        o, d = T.batch(name, "domain")
        rgb, lv = gpu_batch(name, "domain", 3, cull=False)
        assert lv.max() >= 2
        arrs.update({f"{name}|o": o, f"{name}|d": d, f"{name}|rgb": rgb, f"{name}|lv": lv})
    path = str(tmp_path / "refs.npz")
    np.savez(path, **arrs)
    env = dict(os.environ, PYTHONPATH=ROOT, RT_BVH_MIN="2", RT_BVH_LEVEL="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, path, ",".join(TINY)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "tiny ok 4" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


# ---- 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s64", "far10100"])
def test_filters_domain(name):
    """Rays outside the filters' domains among ordinary ones (far10100: beyond CULL_EXTENT, the
    brute-force scan): all equal brute force and the restatement; with a NaN and an infinity in the batch
    as well the call returns RT_OK, the stream synchronises, and every other ray keeps its bytes."""
    depth = 3
    o, d, _, _ = Q.domain(name)
    o2, d2, _, checked = Q.domain(name, True)
    assert not checked.all() and not (np.isfinite(o2).all() and np.isfinite(d2).all())
    rgb, lv = gpu_batch(name, "domain", depth)
    same((rgb, lv), gpu_batch(name, "domain", depth, cull=False), f"{name} domain against brute force")
    idx, ref, rlv = T.batch_ref(name, "domain", depth, Q.N_DOMAIN)
    assert len(idx) == Q.N_DOMAIN and np.array_equal(lv, rlv)
    T.compare(rgb, ref, name, depth, "domain")
    for cull in (True, False):
        with Ctx(T.scene_of(name), cull=cull) as c:
            rgb2, lv2 = trace(c, o2, d2, depth)
        same((rgb2[checked], lv2[checked]), (rgb[checked], lv[checked]), f"{name} beside non-finite rays, cull {cull}")


# ---- 5 ------------------------------------------------------------------------------------------
def test_independence():
    """A ray's bytes depend on nothing but the ray: a permutation, two calls, the prefixes n = 1, 63, 64,
    65, one origin against a repeated one; and 2^21 + 357 rays, once through the grid-stride loop."""
    import torch
    name, depth, n = "s64", 4, 64 * 5 + 7
    o, d = (a[:n] for a in T.batch(name, "incoherent"))
    whole = tuple(a[:n] for a in gpu_batch(name, "incoherent", depth))
    assert len(set(whole[1].tolist())) >= 4
    perm = np.random.RandomState(5).permutation(n)
    with Ctx(T.scene_of(name)) as c:
        same(trace(c, o, d, depth), whole, "the batch alone")
        same(trace(c, o[perm], d[perm], depth), (whole[0][perm], whole[1][perm]), "permutation")
        a, b = trace(c, o[:131], d[:131], depth), trace(c, o[131:], d[131:], depth)
        same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole, "two calls")
        for m in (1, 63, 64, 65):
            same(trace(c, o, d, depth, n=m), (whole[0][:m], whole[1][:m]), f"prefix {m}")
        one = trace(c, o[7], d, depth)
        same(one, trace(c, np.tile(o[7], (n, 1)), d, depth), "one origin against a repeated one")
        assert one[1].any()
        big = (1 << 21) + 357
        assert big > 8192 * 256
        idx = torch.arange(big, device="cuda") % n
        rgb, lv = trace_device(c, to_device(o)[idx].contiguous(), to_device(d)[idx].contiguous(), big, 3, one=False)
        small = trace(c, o, d, 3)
        assert torch.equal(rgb[:big].view(torch.int64), to_device(small[0])[idx].contiguous().view(torch.int64))
        assert torch.equal(lv[:big], to_device(small[1])[idx]) and len(set(small[1].tolist())) >= 3
        assert bool((rgb[big:] == SENTINEL).all()) and bool((lv[big:] == LV_SENTINEL).all()), "entries past n written"


# ---- 6 ------------------------------------------------------------------------------------------
def test_depth_zero_and_one():
    import torch
    name = "mixed"
    o, d, qref, _ = Q.incoherent(name)
    with Ctx(T.scene_of(name)) as c:
        rgb, lv = trace(c, o, d, 0)  # (a null d_work: the size is 0)
        assert rgb.view(np.int64).max() == 0 and rgb.view(np.int64).min() == 0 and not lv.any()
        rgb, lv = trace(c, o, d, 1)
    assert np.array_equal(lv, (qref["elem"] >= 0).astype(np.uint8)), "depth 1 levels are rt_query_rays' hit mask"
    idx = T.subset(name)
    T.compare(rgb[idx], T.incoherent_depth1(name), name, 1, "depth 1")
    assert not lv[idx].all() and lv[idx].any()


def test_chains_that_never_end():
    """The default scene with one light at depth 40."""
    name, w, h, depth = "default~1", 64, 48, 40
    loc, d = Q.camera_rays("default", w, h)
    with Ctx(T.scene_of(name)) as c:
        rgb, lv = trace(c, loc, d, depth)
    with Ctx(T.scene_of(name)) as c:
        same((rgb, lv), launch_window(c, w, h, depth), "against rt_launch_window")
    idx, ref, rlv = T.batch_ref(name, "camera", depth, 64)
    assert np.array_equal(lv[idx], rlv) and lv.max() == depth
    T.compare(rgb[idx], ref, name, depth, "depth 40")


def test_no_lights_and_many_lights():
    o, d = T.batch("s64", "incoherent")
    rgb, lv = gpu_batch("s64~dark", "incoherent", 4)
    assert not rgb.any() and lv.max() == 1 and np.array_equal(lv, (Q.incoherent("s64")[2]["elem"] >= 0).astype(np.uint8))
    name, depth = "s20l33", 3  # (the reflection rays of its 48x36 frame)
    rgb, lv = gpu_batch(name, "reflections", depth)
    same((rgb, lv), gpu_batch(name, "reflections", depth, cull=False), f"{name} against brute force")
    idx, ref, rlv = T.batch_ref(name, "reflections", depth, 200)
    assert np.array_equal(lv[idx], rlv) and rlv.max() == depth and not rlv.all()
    T.compare(rgb[idx], ref, name, depth, "more than 32 lights")


# ---- 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,depth,cull", [
    ("s64~u", "incoherent", 4, False), ("s64~u", "incoherent", 4, True), ("s256", "domain", 3, True),
    ("mixed", "incoherent", 4, False), ("mixed", "incoherent", 4, True)])
def test_binary32_is_the_rounded_binary64(name, kind, depth, cull):
    rgb, lv = gpu_batch(name, kind, depth, cull=cull)
    r32, l32 = gpu_batch(name, kind, depth, "f32", cull)
    assert r32.dtype == np.float32
    same((r32, l32), (rgb.astype(np.float32), lv), f"{name} f32")


# ---- 8 ------------------------------------------------------------------------------------------
def test_scene_update():
    """rt_update_scene between calls on one context, with one work buffer: each result a fresh context's."""
    import torch
    depth = 3
    names = ("s64", "mixed", "s256", "s64")
    o, d = T.batch("s64", "domain")
    with Ctx(T.scene_of(names[0])) as c:
        work = torch.empty((c.L.rt_query_colours_work_bytes(len(d), depth),), dtype=torch.uint8, device="cuda")
        for k, name in enumerate(names):
            if k:
                el = T.elems_of(name)
                N.check(c.L.rt_update_scene(c.p, el, len(el)), "rt_update_scene")
            got = trace(c, o, d, depth, work=work)
            with Ctx(T.scene_of(name)) as fresh:
                same(got, trace(fresh, o, d, depth), f"after the update to {name}")
            assert got[1].any()


# ---- 9 ------------------------------------------------------------------------------------------
def test_python_wrappers():
    name, w, h, depth = "mixed", 64, 48, 3
    o, d = T.batch(name, "incoherent")
    for prec in ("f64", "f32"):
        rgb, lv = raytracer.trace_rays(o, d, 4, T.scene_of(name), precision=prec, levels=True)
        same((rgb, lv), gpu_batch(name, "incoherent", 4, prec), f"trace_rays {prec}")
    only = raytracer.trace_rays(o[3].tolist(), d[:100], 4, T.scene_of(name))
    assert isinstance(only, np.ndarray) and only.shape == (100, 3) and only.dtype == np.float64
    zero = raytracer.trace_rays(o, d, 0, T.scene_of(name))
    assert zero.shape == (len(d), 3) and not zero.any()
    # a tilted pose: the restatement on the rays view_rays returned
    eye, target = (3, 2, -6), (0, 0, 10)
    w2, h2 = 24, 18
    e, dirs = raytracer.view_rays(w2, h2, eye, target)
    tilted = raytracer.render_view(w2, h2, depth, T.scene_of(name), eye=eye, target=target)
    ref, rlv = T.restate(T.scene_of(name), e, dirs, depth, np.arange(len(dirs)))
    assert (rlv > 0).sum() >= 50 and rlv.max() >= 2
    T.compare(tilted.reshape(-1, 3), ref, name, depth, "render_view, tilted")


def test_render_view_at_the_reference_pose():
    """render_view at the reference camera's pose is within 1e-12 of the rendered frame on mixed 64x48 d3.
    One unit in the last place of a direction is enough to miss that (a reflection chain turns it into
    5.8e-4 on one pixel of this frame, in the reference as on the GPU), so view_rays evaluates its
    directions in the reference's order of operations; the difference is printed before it is judged."""
    name, w, h, depth = "mixed", 64, 48, 3
    cam = Q.elems_of(name)[0].u.camera
    loc = Q.cam_location(Q.elems_of(name))
    view = raytracer.render_view(w, h, depth, T.scene_of(name), eye=tuple(loc), target=tuple(loc + np.array([0.0, 0.0, 1.0])),
                                 fov=cam.fov)
    frame = np.asarray(raytracer.render(w, h, T.scene_of(name), depth)).reshape(h, w, 3)
    diff = np.abs(view - frame)
    print("render_view against render: max", float(diff.max()), "pixels beyond 1e-12:", int((diff.max(axis=2) > 1e-12).sum()), flush=True)
    assert view.shape == (h, w, 3) and diff.max() <= 1e-12
