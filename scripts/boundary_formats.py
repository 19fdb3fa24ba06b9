"""What the one-shot boundary costs per output format: S64 at 4096^2 depth 5, one warm context.

  * rt_render into rt_host_alloc memory as f64, f32, u8 and u16: median total_ms and kernel_ms
    over the warm calls (the copy is PCIe-bound, so the bytes per pixel decide: 24, 12, 3, 6);
  * rt_render_ppm_file against rt_render_rawppm_file into /dev/shm;
  * rt_quantize alone on a resident f64 frame, timed with HIP events: bytes moved (24 B read and
    3 B written per pixel) over time, beside the 8 TB/s HBM peak.

Writes one JSON (default profiles/int_frames_boundary.json) and prints it.  The one condition,
which follows from the byte counts: u8 total_ms below f32 total_ms ("u8_below_f32")."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from eraytracer_amd import _native as N  # noqa: E402
from eraytracer_amd.raytracer import render, render_ppm_file  # noqa: E402
from eraytracer_amd.scenes import named  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int_frames_boundary.json"))
a = ap.parse_args()
W = H = a.size
scene = named("s64")
res = {"scene": "s64", "width": W, "height": H, "depth": 5, "warm_calls": a.calls, "rt_render": {}}

for prec, dt, maxv in (("f64", np.float64, 255), ("f32", np.float32, 255), ("u8", np.uint8, 255),
                       ("u16", np.uint16, 65535)):
    out = N.pinned_empty((H, W, 3), dt)
    tot, ker = [], []
    for i in range(a.calls + 2):  # two calls warm the context and its buffers
        st = {}
        render(W, H, scene, 5, precision=prec, max_value=maxv, out=out, stats=st)
        assert st["pinned"]
        if i >= 2:
            tot.append(st["total_ms"])
            ker.append(st["kernel_ms"])
    res["rt_render"][prec] = {"bytes_per_pixel": 3 * np.dtype(dt).itemsize,
                              "total_ms_median": round(statistics.median(tot), 3),
                              "kernel_ms_median": round(statistics.median(ker), 3),
                              "total_ms_min": round(min(tot), 3),
                              "mpx_s": round(W * H / statistics.median(tot) / 1e3, 1)}
    print(prec, res["rt_render"][prec], flush=True)
    del out
res["u8_below_f32"] = res["rt_render"]["u8"]["total_ms_median"] < res["rt_render"]["f32"]["total_ms_median"]

res["file_dev_shm"] = {}
with tempfile.TemporaryDirectory(dir="/dev/shm") as td:
    for what, binary in (("rt_render_ppm_file", False), ("rt_render_rawppm_file", True)):
        path = os.path.join(td, "frame.ppm")
        ts = []
        for i in range(5):
            t0 = time.perf_counter()
            render_ppm_file(W, H, scene, 5, path, binary=binary)
            if i >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
        res["file_dev_shm"][what] = {"ms_median": round(statistics.median(ts), 2), "file_bytes": os.path.getsize(path),
                                     "mpx_s": round(W * H / statistics.median(ts) / 1e3, 1)}
        os.remove(path)
        print(what, res["file_dev_shm"][what], flush=True)

import torch  # noqa: E402

L = N.lib()
frame = torch.from_numpy(np.array(render(W, H, scene, 5))).cuda()
q = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
st = torch.cuda.current_stream().cuda_stream
ms = []
for i in range(23):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    N.check(L.rt_quantize(frame.data_ptr(), N.RT_OUT_F64, W * H * 3, 255, N.RT_OUT_U8, q.data_ptr(), cnt.data_ptr(), st))
    e1.record()
    e1.synchronize()
    if i >= 3:
        ms.append(e0.elapsed_time(e1))
moved = W * H * 27
med = statistics.median(ms)
res["rt_quantize_f64_u8"] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "bytes_moved": moved,
                             "tb_s": round(moved / med / 1e9, 3), "hbm_peak_tb_s": 8.0,
                             "fraction_of_peak": round(moved / med / 1e9 / 8.0, 3), "clamped": int(cnt.item())}
print("rt_quantize", res["rt_quantize_f64_u8"], flush=True)

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(res, sort_keys=True))
