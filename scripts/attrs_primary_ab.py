"""rt_launch_attrs against k_primary on the bench's frame (S64 4096x4096), in one process on one GPU.

    python scripts/attrs_primary_ab.py [--size 4096] [--launches 24] [--warmup 5] [--out FILE]

Variants of rt_launch_attrs, each launch timed with a pair of device events on the launch's stream:
  (a) elem only              4 B per pixel written
  (b) all five planes, f32  44 B per pixel
  (c) all five planes, f64  84 B per pixel
The yardstick is k_primary on the same frame: rt_launch at depth 1 with RT_CFG_KERNEL_TIMING =
RT_KT_PRIMARY | RT_KT_PMASK, read back after every launch (rt_kernel_time with reset), in two series
P1 and P2 — one launch before and one after the three variants of every round, so the two series see
the same machine state the variants see and their difference is the yardstick's own spread.  k_attrs
builds its wave's beam and tests it against every 64-sphere chunk in every launch; k_primary reads
the result from k_pmask's table, computed once per frame geometry.  That difference is measured as
k_pmask's own time: the masks are invalidated before each round's P1 (rt_configure(RT_CFG_CULL, 1)
bumps the scene generation), so every P1 launch is preceded by one timed k_pmask.
Prints medians, minima and maxima, the condition of the issue
    median(a) <= max(median P1, median P2) + |median P1 - median P2| + median k_pmask
and for (b) and (c) the bytes written over the kernel time against the HBM peak.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eraytracer_amd import _native as N  # noqa: E402
from eraytracer_amd import scenes  # noqa: E402

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29  # spec; measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scene", default="s64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    L = N.lib()
    W = H = a.size
    px = W * H
    el = N.marshal(scenes.named(a.scene))
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    N.check(L.rt_configure(p, N.RT_CFG_SIDE_STREAMS, 0), "rt_configure")
    N.check(L.rt_configure(p, N.RT_CFG_KERNEL_TIMING, N.RT_KT_PRIMARY | N.RT_KT_PMASK), "rt_configure")
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    elem = torch.empty((H, W), dtype=torch.int32, device="cuda")
    planes = {}
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        planes[prec] = [torch.empty((H, W), dtype=dt, device="cuda")] + \
                       [torch.empty((H, W, 3), dtype=dt, device="cuda") for _ in range(3)]

    def attr_arg(prec, all_planes):
        code = N.RT_OUT_F64 if prec == "f64" else N.RT_OUT_F32
        ptrs = [t.data_ptr() for t in planes[prec]] if all_planes else [None] * 4
        return N.RtAttrPlanes(ctypes.sizeof(N.RtAttrPlanes), code, elem.data_ptr(), *ptrs)

    variants = {"a": (attr_arg("f64", False), 4), "b": (attr_arg("f32", True), 44), "c": (attr_arg("f64", True), 84)}

    def attrs(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.check(L.rt_launch_attrs(p, W, H, 0, 0, W, H, 16, 0, 1, 1, 0, 0, ctypes.byref(variants[name][0]), stream),
                "rt_launch_attrs")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def kt(kernel):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        N.check(L.rt_kernel_time(p, kernel, ctypes.byref(ms), ctypes.byref(n), 1), "rt_kernel_time")
        return ms.value, n.value

    def primary():
        N.check(L.rt_launch(p, W, H, 1, 16, 0, 1, N.RT_OUT_F32, N.RT_ORDER_EXACT, frame.data_ptr(), None, stream), "rt_launch")
        torch.cuda.synchronize()
        ms, n = kt(N.RT_KT_PRIMARY)
        assert n == 1, n
        return ms

    series = {k: [] for k in ("P1", "a", "b", "c", "P2", "pmask")}
    for i in range(a.warmup + a.launches):
        N.check(L.rt_configure(p, N.RT_CFG_CULL, 1), "rt_configure")  # the next launch computes the masks again
        kt(N.RT_KT_PMASK)
        row = {"P1": primary()}
        pm, n = kt(N.RT_KT_PMASK)
        assert n == 1, n
        row["pmask"] = pm
        for name in ("a", "b", "c"):
            row[name] = attrs(name)
        row["P2"] = primary()
        assert kt(N.RT_KT_PMASK)[1] == 0  # P2 ran on the cached masks
        if i >= a.warmup:
            for k, v in row.items():
                series[k].append(v)
    L.rt_release(p)

    med = {k: statistics.median(v) for k, v in series.items()}
    lines = [f"{a.scene} {W}x{H}, {a.launches} rounds after {a.warmup} warm-up rounds; a round is "
             "k_pmask + P1, (a), (b), (c), P2; times in ms",
             f"device: {torch.cuda.get_device_name(0)}",
             "series    median     min       max"]
    for k in ("P1", "P2", "pmask", "a", "b", "c"):
        v = series[k]
        lines.append(f"{k:8s} {med[k]:8.4f}  {min(v):8.4f}  {max(v):8.4f}")
    spread = abs(med["P1"] - med["P2"])
    bound = max(med["P1"], med["P2"]) + spread + med["pmask"]
    lines.append(f"k_primary medians {med['P1']:.4f} and {med['P2']:.4f}: spread {spread:.4f}; beam cost (k_pmask) {med['pmask']:.4f}")
    lines.append(f"condition: median(a) = {med['a']:.4f} <= {bound:.4f} = max k_primary median + spread + beam cost: "
                 f"{'holds' if med['a'] <= bound else 'DOES NOT HOLD'}")
    for k in ("b", "c"):
        tbs = variants[k][1] * px / (med[k] * 1e-3) / 1e12
        lines.append(f"({k}) {variants[k][1]} B/px written: {variants[k][1] * px / 1e6:.1f} MB in {med[k]:.4f} ms = {tbs:.3f} TB/s, "
                     f"{100 * tbs / HBM_PEAK_TBS:.1f} % of the {HBM_PEAK_TBS} TB/s peak, "
                     f"{100 * tbs / HBM_COPY_TBS:.1f} % of the {HBM_COPY_TBS} TB/s a float4 copy reaches")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
