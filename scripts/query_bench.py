"""rt_query_rays (k_query, csrc/rt_query.hip) measured on one MI355X: Mrays/s of

  (a) S64, the 1024x1024 camera rays with RT_QUERY_ONE_ORIGIN, all five planes, binary32 — against
      rt_launch_attrs of the same frame on the same build (k_attrs: tabled origin, no per-ray input);
  (b) the same rays shuffled;
  (c) S256, 2^20 random unit rays from inside the scene's box: the per-lane BVH walk, and with the
      scene compiled without a BVH (RT_BVH_MIN above its sphere count) the wave beams, which such
      waves turn off: every sphere tested.

Device events, 5 warm-up launches, then the median of 20, every launch timed on its own.  Each case
runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/query_bench.py [--out FILE]
"""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS = 5, 20
W = H = 1024
CASES = ("attrs", "a", "b", "c_bvh", "c_beam")


def camera_dirs(elems, w, h):
    """The unit directions from the camera through {x/w, y/h} of the screen (numpy: for timing, the
    screen's corners from the oracle, interpolated)."""
    from oracle import oracle as O
    O.build()
    c = elems[0].u.camera.location
    loc = np.array([c.x, c.y, c.z])
    p00, p10, p01 = (np.array(O.point_on_screen(elems[0], X, Y)) for X, Y in ((0, 0), (1, 0), (0, 1)))
    X, Y = np.meshgrid(np.arange(w) / w, np.arange(h) / h)
    pts = p00 + X[..., None] * (p10 - p00) + Y[..., None] * (p01 - p00)
    v = (pts - loc).reshape(-1, 3)
    return loc, np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True))


def timed(launch):
    import torch
    for _ in range(WARM):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def run_case(case):
    import torch
    from eraytracer_amd import _native as N
    from eraytracer_amd import scenes
    L = N.lib()
    scene = scenes.s64() if case in ("attrs", "a", "b") else scenes.s256()
    el = N.marshal(scene)
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    st = torch.cuda.current_stream().cuda_stream
    if case in ("attrs", "a", "b"):
        n = W * H
        loc, d = camera_dirs(el, W, H)
        if case == "b":
            d = d[np.random.RandomState(1).permutation(n)]
    else:
        n = 1 << 20
        rng = np.random.RandomState(2)
        c = np.array([[e.u.sphere.center.x, e.u.sphere.center.y, e.u.sphere.center.z] for e in el if e.kind == N.RT_SPHERE])
        loc = c.min(axis=0) + (c.max(axis=0) - c.min(axis=0)) * rng.uniform(size=(n, 3))
        v = rng.normal(size=(n, 3))
        d = v / np.linalg.norm(v, axis=1, keepdims=True)
    f32 = torch.float32
    buf = [torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=f32, device="cuda")] + \
          [torch.empty((n, 3), dtype=f32, device="cuda") for _ in range(3)]
    pl = N.RtAttrPlanes(ctypes.sizeof(N.RtAttrPlanes), N.RT_OUT_F32, *[b.data_ptr() for b in buf])
    d_o, d_d = torch.from_numpy(np.ascontiguousarray(loc)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    one = N.RT_QUERY_ONE_ORIGIN if loc.ndim == 1 else 0
    if case == "attrs":
        def launch():
            N.check(L.rt_launch_attrs(p, W, H, 0, 0, W, H, 16, 0, 1, 1, 0, 0, ctypes.byref(pl), st), "rt_launch_attrs")
    else:
        def launch():
            N.check(L.rt_query_rays(p, d_o.data_ptr(), d_d.data_ptr(), n, one, ctypes.byref(pl), st), "rt_query_rays")
    med, lo, hi = timed(launch)
    hits = int((buf[0] >= 0).sum())
    L.rt_release(p)
    print(f"RESULT {case} {n} {med:.4f} {lo:.4f} {hi:.4f} {hits}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    res = {}
    for case in CASES:
        env = dict(os.environ)
        if case == "c_beam":
            env["RT_BVH_MIN"] = "1000000"
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], env=env, capture_output=True,
                               text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {args.limit} s; stopping", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{case}: exit status {r.returncode}; stopping\n{r.stdout}\n{r.stderr}", flush=True)
            return 1
        _, _, n, med, lo, hi, hits = line[0].split()
        res[case] = (int(n), float(med), float(lo), float(hi), int(hits))
    what = {"attrs": f"rt_launch_attrs, S64 {W}x{H}, five planes f32 (the yardstick)",
            "a": f"(a) rt_query_rays, S64 {W}x{H} camera rays, one origin, five planes f32",
            "b": "(b) the same rays shuffled",
            "c_bvh": "(c) S256, 2^20 random unit rays, five planes f32: BVH walk",
            "c_beam": "(c) the same, no BVH (RT_BVH_MIN=1000000): wave beams (off for such waves: every sphere)"}
    out = [f"rt_query_rays (k_query, rt_query.hip): python scripts/query_bench.py; device events, {WARM} warm-up launches, "
           f"median of {REPS}; times in ms", f"{'case':<8}{'rays':>9}{'median':>10}{'min':>10}{'max':>10}{'Mrays/s':>10}{'hits':>9}"]
    for case in CASES:
        n, med, lo, hi, hits = res[case]
        out.append(f"{case:<8}{n:>9}{med:>10.4f}{lo:>10.4f}{hi:>10.4f}{n / med / 1e3:>10.1f}{hits:>9}   {what[case]}")
    out.append(f"(a) / rt_launch_attrs: {res['a'][1] / res['attrs'][1]:.2f}x the time; (b) / (a): {res['b'][1] / res['a'][1]:.2f}x; "
               f"(c) BVH / beams: {res['c_bvh'][1] / res['c_beam'][1]:.2f}x")
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
