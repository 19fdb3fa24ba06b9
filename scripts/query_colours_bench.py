"""rt_query_colours (k_trace, csrc/rt_trace.hip) measured on one MI355X: Mrays/s of

  (a) rt_launch_window, S64 1024x1024 at depth 5, binary32, on a fresh context — the yardstick, the
      wavefront engine on the camera's own rays;
  (b) rt_query_colours on the same camera rays with RT_QUERY_ONE_ORIGIN;
  (c) the same rays shuffled;
  (d) S256, 2^20 random unit rays from inside the scene's box at depth 4: the per-lane BVH walk, and
      with the scene compiled without a BVH (RT_BVH_MIN above its sphere count) the wave beams.

and, computed from the shapes, the work-space bytes written and read per ray: every level a ray's chain
hits stores one record (76 bytes) and loads it back, with the hit point of the level above (24 bytes)
for every level but the first.

Device events, 5 warm-up launches, then the median of 20, every launch timed on its own.  Each case
runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/query_colours_bench.py [--out FILE]
"""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.query_bench import W, H, WARM, REPS, camera_dirs, timed  # noqa: E402

CASES = ("a", "b", "c", "d_bvh", "d_beam")
REC_BYTES, ORIGIN_BYTES = 76, 24


def work_traffic(levels):
    """(bytes written, bytes read) per ray of the work space, from the rays' chain lengths."""
    lv = levels.astype(np.int64)
    return float(REC_BYTES * lv.mean()), float((REC_BYTES * lv + ORIGIN_BYTES * np.maximum(lv - 1, 0)).mean())


def run_case(case):
    import torch
    from eraytracer_amd import _native as N
    from eraytracer_amd import scenes
    L = N.lib()
    cam = case in ("a", "b", "c")
    scene = scenes.s64() if cam else scenes.s256()
    depth = 5 if cam else 4
    el = N.marshal(scene)
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    st = torch.cuda.current_stream().cuda_stream
    if cam:
        n = W * H
        loc, d = camera_dirs(el, W, H)
        if case == "c":
            d = d[np.random.RandomState(1).permutation(n)]
    else:
        n = 1 << 20
        rng = np.random.RandomState(2)
        c = np.array([[e.u.sphere.center.x, e.u.sphere.center.y, e.u.sphere.center.z] for e in el if e.kind == N.RT_SPHERE])
        loc = c.min(axis=0) + (c.max(axis=0) - c.min(axis=0)) * rng.uniform(size=(n, 3))
        v = rng.normal(size=(n, 3))
        d = v / np.linalg.norm(v, axis=1, keepdims=True)
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    lv = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    if case == "a":
        rows = L.rt_shard_rows(H, 16, 1)
        assert rows == H
        work_bytes = 0

        def launch():
            N.check(L.rt_launch_window(p, W, H, depth, 0, 0, W, H, 16, 0, 1, N.RT_OUT_F32, N.RT_ORDER_EXACT, 1, 0,
                                       rgb.data_ptr(), lv.data_ptr(), st), "rt_launch_window")
    else:
        d_o, d_d = torch.from_numpy(np.ascontiguousarray(loc)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
        one = N.RT_QUERY_ONE_ORIGIN if loc.ndim == 1 else 0
        work_bytes = L.rt_query_colours_work_bytes(n, depth)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")

        def launch():
            N.check(L.rt_query_colours(p, d_o.data_ptr(), d_d.data_ptr(), n, depth, one, N.RT_OUT_F32, rgb.data_ptr(),
                                       lv.data_ptr(), work.data_ptr(), work_bytes, st), "rt_query_colours")
    med, lo, hi = timed(launch)
    levels = lv.cpu().numpy()
    wr, rd = work_traffic(levels) if case != "a" else (0.0, 0.0)
    L.rt_release(p)
    print(f"RESULT {case} {n} {med:.4f} {lo:.4f} {hi:.4f} {int((levels > 0).sum())} {levels.astype(np.int64).mean():.3f} "
          f"{work_bytes} {wr:.1f} {rd:.1f}", flush=True)


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
        if case == "d_beam":
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
        f = line[0].split()[2:]
        res[case] = (int(f[0]), float(f[1]), float(f[2]), float(f[3]), int(f[4]), float(f[5]), int(f[6]), float(f[7]), float(f[8]))
    what = {"a": f"(a) rt_launch_window, S64 {W}x{H} d5 f32 with levels, fresh context (the yardstick)",
            "b": f"(b) rt_query_colours, S64 {W}x{H} camera rays d5, one origin, f32 with levels",
            "c": "(c) the same rays shuffled",
            "d_bvh": "(d) S256, 2^20 random unit rays d4, f32 with levels: BVH walk",
            "d_beam": "(d) the same, no BVH (RT_BVH_MIN=1000000): wave beams (off for such waves: every sphere)"}
    out = [f"rt_query_colours (k_trace, rt_trace.hip): python scripts/query_colours_bench.py; device events, {WARM} warm-up "
           f"launches, median of {REPS}; times in ms; work-space bytes per ray from the chain lengths (76 per level stored, "
           "76 + 24 per level loaded, 76 for level 0)",
           f"{'case':<8}{'rays':>9}{'median':>10}{'min':>10}{'max':>10}{'Mrays/s':>10}{'hits':>9}{'levels':>8}{'work MiB':>10}"
           f"{'B wr/ray':>10}{'B rd/ray':>10}"]
    for case in CASES:
        n, med, lo, hi, hits, mean_lv, wb, wr, rd = res[case]
        out.append(f"{case:<8}{n:>9}{med:>10.4f}{lo:>10.4f}{hi:>10.4f}{n / med / 1e3:>10.1f}{hits:>9}{mean_lv:>8.3f}"
                   f"{wb / 2 ** 20:>10.1f}{wr:>10.1f}{rd:>10.1f}   {what[case]}")
    out.append(f"(b) / (a): {res['b'][1] / res['a'][1]:.2f}x the time; (c) / (b): {res['c'][1] / res['b'][1]:.2f}x; "
               f"(d) BVH / beams: {res['d_bvh'][1] / res['d_beam'][1]:.2f}x")
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
