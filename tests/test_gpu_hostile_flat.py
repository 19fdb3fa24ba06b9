"""The triangle and plane paths on the flat hostile scenes (tests/hostile_flat.py).

The scenes reach what no other scene does: reflected directions that are not unit vectors (the
beams' ``bad`` lanes, the BVH walked by them), hit points and reflection origins far beyond
CULL_EXTENT (SceneHdr::ext bounds origins and spheres only), triangle and plane shadow targets
with negative and huge t*, the reference's zero and non-geometric triangle normals, scenes without
a sphere (empty sphere tables, candidate and occluder masks) and exact ties across the three kinds.
Their specular powers are 0 or 1, where pow is exact on both sides, so nothing here has a
tolerance: every frame equals the C oracle's in every bit and every reflection-chain level, the
filtered frame equals the brute-force one (RT_CFG_CULL = 0), and the attribute planes equal
tests/attr_ref.py in every byte.

Frames are 64x48 and 88x40 (partial 8x16 tiles), and 320x240 for five scenes (tiles small enough
for the beams and cones to cull between the unit spheres); depths are the scenes'.  Oracle frames are computed
once per process (hostile_flat.oracle_ref) and handed to the child processes (forced engines,
environment knobs: read once per process) as a file.
"""
import ctypes

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd.raytracer import render
from tests import attr_ref as A
from tests import hostile_flat as F
from tests.test_gpu_attrs import check as check_planes
from tests.test_gpu_attrs import gpu_frame as attr_frame
from tests.test_gpu_frames import bench_frames, nonbitwise
from tests.test_gpu_hostile import SIZES, _against_oracle, _child_run

pytestmark = pytest.mark.gpu

_GPU = {}


def _levels_render(name, w, h):
    """rt_render with levels (the side-stream kernels), once per process."""
    key = (name, w, h)
    if key not in _GPU:
        _GPU[key] = render(w, h, F.build(name), F.depth(name), levels=True)
    return _GPU[key]


# ---- 1, 2: every scene against the oracle and the brute-force scans ---------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", F.NAMES)
def test_flat_frame_equals_oracle(oracle, name, w, h):
    img, lv = _levels_render(name, w, h)
    ref, rlv = F.oracle_ref(oracle, name, w, h)
    _against_oracle(f"{name} {w}x{h}", img, lv, ref, rlv)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", F.NAMES)
def test_flat_filters_equal_brute_force(name, w, h):
    """The bench path's frame (two frames in flight, no side streams) with every filter on equals
    the brute-force frame and the levels render, bit for bit."""
    scene, d = F.build(name), F.depth(name)
    fast = bench_frames(scene, w, h, d)
    brute = bench_frames(scene, w, h, d, cull=False)
    n = nonbitwise(fast, brute)
    assert n == 0, f"{name} {w}x{h}: {n} pixels differ from the brute-force scans"
    n = nonbitwise(fast, _levels_render(name, w, h)[0])
    assert n == 0, f"{name} {w}x{h}: {n} pixels differ between the bench path and the levels render"


# ---- dense frames ---------------------------------------------------------------------------------
# At 64x48 an 8x8 tile of hit points on a floor is several units wide: the origin balls of the
# reflection beams and the hit balls of the shadow cones swallow the unit spheres next to them
# (sr >= 1) and cull little there.  At 320x240 they are smaller than the spheres, the beams and cones
# are as narrow as the benchmark's, and 25 times as many rays meet each construction (mirror_nonunit:
# 6694 rays that are not unit vectors end on a sphere, against 271).
@pytest.mark.parametrize("name", ["corridor_nonunit", "mirror_nonunit", "graze16", "mesh", "big_flat"])
def test_flat_dense_frame(oracle, name):
    w, h = 320, 240
    scene, d = F.build(name), F.depth(name)
    img, lv = render(w, h, scene, d, levels=True)
    ref, rlv = F.oracle_ref(oracle, name, w, h)
    _against_oracle(f"{name} {w}x{h}", img, lv, ref, rlv)
    fast = bench_frames(scene, w, h, d)
    assert nonbitwise(fast, bench_frames(scene, w, h, d, cull=False)) == 0
    assert nonbitwise(fast, img) == 0


# ---- 3, 4: child processes ------------------------------------------------------------------------
FUSED_AT_LEAST = ("mesh_small", "tie3_tps", "tie3_pst", "tie3_stp", "corridor", "planes_only")


@pytest.mark.parametrize("engine", ["fused", "wave"])
def test_flat_forced_engine(oracle, tmp_path, engine):
    """RT_ENGINE=fused / wave: levels and bits against the oracle.  The fused engine takes the
    scenes of at most 40 objects (the ties across kinds, the corridor, the sphere-free corridor and
    the small mesh among them); the wavefront engine takes all."""
    ran, skipped = _child_run(oracle, tmp_path, {"RT_ENGINE": engine}, engine, False, list(F.NAMES), F)
    print(f"RT_ENGINE={engine}: {ran} scenes, skipped {skipped}", flush=True)
    if engine == "wave":
        assert ran == len(F.NAMES) and not skipped
    else:
        assert not set(FUSED_AT_LEAST) & set(skipped), skipped


ENV_SCENES = ["corridor", "corridor_nonunit", "mirror_nonunit", "graze16", "pencil_wall", "pencil_fartri", "mesh",
              "behind_facing"]


@pytest.mark.parametrize("env", [{"RT_BVH_MIN": "2", "RT_BVH_LEVEL": "1"}, {"RT_BEAM_MIN": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_flat_environment_runs(oracle, tmp_path, env):
    """The BVH from the first reflection level on, over nine or ten spheres: traversed from origins
    5e5 units away (pencil_wall, graze16) and by directions that are not unit vectors
    (corridor_nonunit); and the wave beams at any size.  Against the oracle and brute force."""
    ran, skipped = _child_run(oracle, tmp_path, env, "any", True, ENV_SCENES, F)
    assert ran == len(ENV_SCENES) and not skipped


# ---- 5: attribute planes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.NAMES)
def test_flat_attribute_planes(name):
    """elem (at a tie, the earlier list index), t (negative, and 5e5), point, normal (the zero
    vector, the non-unit plane normals as written) and albedo, every byte."""
    w, h = 64, 48
    ref = A.frame(name, w, h)
    print(name, "kinds (miss, sphere, triangle, plane, distinct)", A.kinds(name, ref), flush=True)
    check_planes(attr_frame(name, w, h, "f64"), ref, "f64", what=name)
    if name in ("tie3_tps", "graze16"):
        check_planes(attr_frame(name, w, h, "f32"), ref, "f32", what=name)


# ---- 6: supersampling -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corridor_nonunit", "mirror_nonunit", "mesh", "pencil_wall"])
def test_flat_supersampling(oracle, name):
    spp, seed = 3, 0x5EED0F1A
    w, h = 64, 48
    scene, d = F.build(name), F.depth(name)
    img, lv = render(w, h, scene, d, levels=True, spp=spp, seed=seed)
    ref, rlv = F.oracle_ref(oracle, name, w, h, spp=spp, seed=seed)
    _against_oracle(f"{name} spp {spp}", img, lv, ref, rlv)
    fast = bench_frames(scene, w, h, d, spp=spp, seed=seed)
    assert nonbitwise(fast, bench_frames(scene, w, h, d, spp=spp, seed=seed, cull=False)) == 0
    assert nonbitwise(fast, img) == 0


# ---- 7: a pixel window ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planes_only", "mesh", "graze16"])
def test_flat_window_is_the_crop(oracle, name):
    w, h = 88, 40
    x0, y0, ww, wh = win = (5, 7, 37, 19)
    img, lv = render(w, h, F.build(name), F.depth(name), levels=True, window=win)
    assert img.shape == (wh, ww, 3) and lv.shape == (wh, ww)
    full, flv = _levels_render(name, w, h)
    assert nonbitwise(np.ascontiguousarray(img), np.ascontiguousarray(full[y0:y0 + wh, x0:x0 + ww])) == 0
    assert np.array_equal(lv, flv[y0:y0 + wh, x0:x0 + ww])
    ref, rlv = F.oracle_ref(oracle, name, w, h)
    _against_oracle(f"{name} window {win}", np.ascontiguousarray(img), lv, np.ascontiguousarray(ref[y0:y0 + wh, x0:x0 + ww]),
                    rlv[y0:y0 + wh, x0:x0 + ww])


# ---- 8: rt_update_scene through every scene ---------------------------------------------------------
def test_flat_scene_updates_equal_fresh_contexts(oracle):
    """One resident context walked by rt_update_scene through every scene in SCENES order and back
    to the first: the sphere count goes 9 -> 0 -> 10 -> 9 -> 10 -> 160 -> 0 -> 9, the triangle and plane counts
    up and down (tables, masks, BVH and beams resized or dropped).  Each frame equals a fresh
    context's and the oracle's, bit for bit."""
    import torch
    L = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    w, h = 64, 48

    def frame(p, d):
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float64, device="cuda")
        N.check(L.rt_launch(p, w, h, d, 16, 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, out.data_ptr(), None, st))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    walk = list(F.NAMES) + ["empty", F.NAMES[0]]  # from the largest scene to none, then back to the first
    n_sph = [sum(t[0] == "sphere" for t in F.build(name)) for name in walk]
    assert {(9, 0), (0, 10), (10, 160), (160, 0), (0, 9)} <= set(zip(n_sph, n_sph[1:]))
    el = N.marshal(F.build(walk[0]))
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    try:
        frame(p, F.depth(walk[0]))
        for name in walk[1:]:
            el = N.marshal(F.build(name))
            N.check(L.rt_update_scene(p, el, len(el)), "rt_update_scene")
            got = frame(p, F.depth(name))
            q = ctypes.c_void_p()
            N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(q)), "rt_prepare")
            try:
                fresh = frame(q, F.depth(name))
            finally:
                L.rt_release(q)
            assert np.all(np.isfinite(got)), name
            assert nonbitwise(got, fresh) == 0, f"{name}: differs from a fresh context"
            ref, _ = F.oracle_ref(oracle, name, w, h)
            assert nonbitwise(got, np.ascontiguousarray(ref)) == 0, f"{name}: differs from the oracle"
    finally:
        L.rt_release(p)
