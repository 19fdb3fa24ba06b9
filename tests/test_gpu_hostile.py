"""The culling filters and the camera on the hostile scenes (tests/hostile.py).

DESIGN §3: the filters only skip objects that provably cannot be hit, and pow is the only source
of bits that differ from the oracle's.  The hostile scenes reach the filter branches the benchmark
generator's scenes never do (origins in and on spheres, degenerate radii, lights on surfaces,
extents near CULL_EXTENT, axis-parallel rays, exact ties) and cameras other than (0, 0, -2) / fov 90
/ 4x3; their specular powers are 0 or 1, where pow is exact on both sides.  So every frame here must
equal the C oracle's bit for bit (and its reflection chains level for level), and the filtered
frame must equal the brute-force one (RT_CFG_CULL = 0) bit for bit.

Frames are 64x48 and 88x40 (partial 8x16 tiles); depths are the scenes' (tests/hostile.py).
Oracle frames are computed once per process (hostile.oracle_ref) and handed to the child
processes (forced engines, environment knobs: read once per process) as a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd.raytracer import render
from tests import hostile as H
from tests.test_gpu_frames import bench_frames, nonbitwise

pytestmark = pytest.mark.gpu
TOL = 1e-5
SIZES = [(64, 48), (88, 40)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_GPU = {}


def _levels_render(name, w, h):
    """rt_render with levels (the side-stream kernels), once per process."""
    key = (name, w, h)
    if key not in _GPU:
        _GPU[key] = render(w, h, H.build(name), H.depth(name), levels=True)
    return _GPU[key]


def _against_oracle(what, img, lv, ref, rlv):
    """Levels equal, finite, within the project's bar — and, the powers being 0 or 1, no pixel that
    is not bit-identical."""
    bad_lv = int((lv != rlv).sum())
    assert bad_lv == 0, f"{what}: {bad_lv} pixels with a different reflection chain, first {np.argwhere(lv != rlv)[:4].tolist()}"
    assert np.all(np.isfinite(img)), what
    err = float(np.abs(img - ref).max())
    n = nonbitwise(np.ascontiguousarray(img), np.ascontiguousarray(ref))
    print(f"{what}: max |delta| {err:.3g}, {n} of {lv.size} pixels not bit-identical", flush=True)
    assert err <= TOL, f"{what}: max |delta| {err}"
    if n:
        d = ~np.all(img.view(np.int64) == np.ascontiguousarray(ref).view(np.int64), axis=-1)
        raise AssertionError(f"{what}: {n} pixels not bit-identical to the oracle, first (row, col) "
                             f"{np.argwhere(d)[:6].tolist()}, levels there {rlv[d][:6].tolist()}")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", H.NAMES)
def test_hostile_frame_equals_oracle(oracle, name, w, h):
    img, lv = _levels_render(name, w, h)
    ref, rlv = H.oracle_ref(oracle, name, w, h)
    _against_oracle(f"{name} {w}x{h}", img, lv, ref, rlv)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", H.NAMES)
def test_hostile_filters_equal_brute_force(name, w, h):
    """The bench path's frame (two frames in flight, no side streams) with every filter on equals
    the brute-force frame and the levels render, bit for bit."""
    scene, d = H.build(name), H.depth(name)
    fast = bench_frames(scene, w, h, d)
    brute = bench_frames(scene, w, h, d, cull=False)
    n = nonbitwise(fast, brute)
    assert n == 0, f"{name} {w}x{h}: {n} pixels differ from the brute-force scans"
    n = nonbitwise(fast, _levels_render(name, w, h)[0])
    assert n == 0, f"{name} {w}x{h}: {n} pixels differ between the bench path and the levels render"


# ---- child processes: forced engines and environment knobs -------------------------------------
_CHILD = r"""
import ctypes, importlib, sys
import numpy as np
from eraytracer_amd import _native as N
from eraytracer_amd.raytracer import render
from tests.test_gpu_frames import bench_frames, nonbitwise
refs = np.load(sys.argv[1])
engine, brute, names = sys.argv[2], sys.argv[3] == '1', sys.argv[4].split(',')
H = importlib.import_module(sys.argv[5])
L = N.lib()
ran = 0
for name in names:
    sc, d = H.build(name), H.depth(name)
    el = N.marshal(sc)
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), 'rt_prepare')
    e = L.rt_engine(p, 1)
    L.rt_release(p)
    if engine == 'fused' and e != N.RT_ENGINE_FUSED:
        print('skipped', name, flush=True)
        continue
    if engine == 'wave':
        assert e == N.RT_ENGINE_WAVE, name
    for w, h in ((64, 48), (88, 40)):
        img, lv = render(w, h, sc, d, levels=True)
        ref, rlv = refs[f'{name}|{w}x{h}|rgb'], refs[f'{name}|{w}x{h}|lv']
        assert np.array_equal(lv, rlv), (name, w, h, 'levels', np.argwhere(lv != rlv)[:4].tolist())
        assert np.all(np.isfinite(img)), (name, w, h)
        assert float(np.abs(img - ref).max()) <= 1e-5, (name, w, h)
        n = nonbitwise(img, np.ascontiguousarray(ref))
        assert n == 0, (name, w, h, f'{n} pixels not bit-identical to the oracle')
        if brute:
            fast = bench_frames(sc, w, h, d)
            assert nonbitwise(fast, bench_frames(sc, w, h, d, cull=False)) == 0, (name, w, h, 'brute force')
            assert nonbitwise(fast, img) == 0, (name, w, h, 'bench path')
    ran += 1
print('hostile ok', ran, flush=True)
"""


def _refs_file(oracle, tmp_path, names, module=H):
    arrs = {}
    for name in names:
        for w, h in SIZES:
            ref, rlv = module.oracle_ref(oracle, name, w, h)
            arrs[f"{name}|{w}x{h}|rgb"], arrs[f"{name}|{w}x{h}|lv"] = ref, rlv
    path = str(tmp_path / "refs.npz")
    np.savez(path, **arrs)
    return path


def _child_run(oracle, tmp_path, env, engine, brute, names, module=H):
    """The child's (count of scenes it ran, names it skipped); module: the scene table's module
    (its build, depth and oracle_ref)."""
    path = _refs_file(oracle, tmp_path, names, module)
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, "-c", _CHILD, path, engine, "1" if brute else "0", ",".join(names),
                        module.__name__], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "hostile ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    ran = int(r.stdout.split("hostile ok")[1].split()[0])
    assert ran > 0
    skipped = [ln.split(None, 1)[1] for ln in r.stdout.splitlines() if ln.startswith("skipped ")]
    assert ran + len(skipped) == len(names)
    return ran, skipped


def _child(oracle, tmp_path, env, engine, brute, names):
    return _child_run(oracle, tmp_path, env, engine, brute, names)[0]


@pytest.mark.parametrize("engine", ["fused", "wave"])
def test_hostile_forced_engine(oracle, tmp_path, engine):
    """RT_ENGINE=fused / wave on every hostile scene (fused skipped where rt_engine refuses it):
    levels and bits against the oracle."""
    ran = _child(oracle, tmp_path, {"RT_ENGINE": engine}, engine, False, list(H.NAMES))
    if engine == "wave":
        assert ran == len(H.NAMES)


@pytest.mark.parametrize("env", [{"RT_BVH_MIN": "2", "RT_BVH_LEVEL": "1"}, {"RT_BEAM_MIN": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_hostile_environment_runs(oracle, tmp_path, env):
    """The BVH from the first reflection level on (axis-parallel rays through bvh_inv's clamp at
    every level of the lattice's centre pixel; ties and enclosing boxes in S160+G), and the wave
    beams at any size: against the oracle and the brute-force scans."""
    assert _child(oracle, tmp_path, env, "any", True, ["lattice", "s160+g"]) == 2


# ---- supersampling: k_pmask<true>'s corner beams -------------------------------------------------
@pytest.mark.parametrize("cam", ["fov150", "vga", "dz0"])
@pytest.mark.parametrize("base", H.CAMERA_BASES)
def test_hostile_camera_supersampling(oracle, base, cam):
    name, spp, seed = f"{base}@{cam}", 3, 0x5EED0005
    w, h = 64, 48
    img, lv = render(w, h, H.build(name), H.depth(name), levels=True, spp=spp, seed=seed)
    ref, rlv = H.oracle_ref(oracle, name, w, h, spp=spp, seed=seed)
    _against_oracle(f"{name} spp {spp}", img, lv, ref, rlv)
    fast = bench_frames(H.build(name), w, h, H.depth(name), spp=spp, seed=seed)
    assert nonbitwise(fast, bench_frames(H.build(name), w, h, H.depth(name), spp=spp, seed=seed, cull=False)) == 0
    assert nonbitwise(fast, img) == 0


# ---- rt_update_scene with only the camera changed ------------------------------------------------
@pytest.mark.parametrize("base", H.CAMERA_BASES)
def test_hostile_camera_update_equals_fresh_context(oracle, base):
    """One context walks through every hostile camera by rt_update_scene (lights and objects
    unchanged: only the header's camera fields, the camera's per-origin rows and the primary
    candidate masks may change): each frame equals a fresh context's and the oracle's, bit for bit."""
    import torch
    L = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    w, h, d = 64, 48, 5

    def frame(p):
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float64, device="cuda")
        N.check(L.rt_launch(p, w, h, d, 16, 0, 1, N.RT_OUT_F64, N.RT_ORDER_EXACT, out.data_ptr(), None, st))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    el = N.marshal(H.base(base))
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    try:
        frame(p)
        for cam in list(H.CAMERAS) + ["fov20"]:  # and back to an earlier camera
            name = f"{base}@{cam}"
            el = N.marshal(H.build(name))
            N.check(L.rt_update_scene(p, el, len(el)), "rt_update_scene")
            got = frame(p)
            q = ctypes.c_void_p()
            N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(q)), "rt_prepare")
            try:
                fresh = frame(q)
            finally:
                L.rt_release(q)
            assert np.all(np.isfinite(got)), name
            assert nonbitwise(got, fresh) == 0, f"{name}: differs from a fresh context"
            ref, _ = H.oracle_ref(oracle, name, w, h)
            assert nonbitwise(got, np.ascontiguousarray(ref)) == 0, f"{name}: differs from the oracle"
    finally:
        L.rt_release(p)
