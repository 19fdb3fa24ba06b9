"""What progressive supersampling (RT_PROGRESSIVE) costs, measured with device events:

    python scripts/progressive_cost.py [--parent-tree DIR] [--out profiles/progressive_cost.json]

partition  S256, depth 8, 16 spp at 1024^2 (no side streams, as bench.py's frames): (a) one-shot
           rt_launch_spp to f32, (b) rt_launch_samples [0,16) + rt_resolve to f32, (c) sixteen
           single-sample calls, each followed by a u8 resolve — alternated in one process, several
           rounds.  With --parent-tree (a built checkout of an earlier commit), (a) is also taken
           with that tree's package and library and with this one's, in alternating child processes.
resolve    rt_resolve of 4096^2 x 3 sums to each format, rt_quantize of the same array beside the
           integer ones; algorithmic bytes (8 read + the element written per value) over the time.
bench      with --parent-tree: bench.py's headline, the two trees alternated, --bench-runs each.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child measuring another checkout imports that checkout's package: --tree)
TREE = next((v.split("=", 1)[1] for v in sys.argv if v.startswith("--tree=")), ROOT)
sys.path.insert(0, TREE)
HBM_PEAK_GBS = 8000.0  # spec; a float4 copy reaches about 6300


def timer(reps, warm):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    return timed


def partition(a, only_oneshot=False):
    import ctypes

    import torch

    from eraytracer_amd import _native as N
    from eraytracer_amd import scenes
    L = N.lib()
    el = N.marshal(scenes.named(a.scene))
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    N.check(L.rt_configure(p, N.RT_CFG_SIDE_STREAMS, 0), "rt_configure")
    S, D, spp, seed = a.size, a.depth, a.spp, 0x5EED0005
    f32 = torch.empty((S, S, 3), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def one_shot():
        N.check(L.rt_launch_spp(p, S, S, D, 16, 0, 1, N.RT_OUT_F32, N.RT_ORDER_EXACT, spp, seed, f32.data_ptr(), None, st),
                "rt_launch_spp")
    timed = timer(a.reps, a.warm)
    if only_oneshot:
        out = {"one_shot_ms": [timed(one_shot) for _ in range(a.rounds)]}
        L.rt_release(p)
        return out
    acc = torch.empty((S, S, 3), dtype=torch.float64, device="cuda")
    u8 = torch.empty((S, S, 3), dtype=torch.uint8, device="cuda")
    res = torch.empty((S, S, 3), dtype=torch.float32, device="cuda")
    n = S * S * 3

    def samples(b, e):
        N.check(L.rt_launch_samples(p, S, S, D, 0, 0, S, S, 16, 0, 1, spp, seed, b, e, acc.data_ptr(), None, st),
                "rt_launch_samples")

    def whole():
        samples(0, spp)
        N.check(L.rt_resolve(acc.data_ptr(), n, spp, N.RT_OUT_F32, 0, res.data_ptr(), None, st), "rt_resolve")

    def single():
        for s in range(spp):
            samples(s, s + 1)
            N.check(L.rt_resolve(acc.data_ptr(), n, s + 1, N.RT_OUT_U8, 255, u8.data_ptr(), None, st), "rt_resolve")
    rows = {"one_shot_ms": [], "samples_resolve_f32_ms": [], "single_samples_u8_ms": []}
    for _ in range(a.rounds):  # alternated: a, b, c, a, b, c, ...
        for key, fn in zip(rows, (one_shot, whole, single)):
            rows[key].append(timed(fn))
    one_shot()
    whole()
    torch.cuda.synchronize()
    rows["f32_frames_equal"] = bool(torch.equal(f32.view(torch.int32), res.view(torch.int32)))
    L.rt_release(p)
    return rows


def resolve_alone(a):
    import torch

    from eraytracer_amd import _native as N
    L = N.lib()
    n = a.resolve_size * a.resolve_size * 3
    src = torch.rand(n, dtype=torch.float64, device="cuda") * 16.0
    mean = src / 16.0
    st = torch.cuda.current_stream().cuda_stream
    timed = timer(a.reps, a.warm)
    out = {"values": n}
    for name, fmt, dt, maxv in (("f64", N.RT_OUT_F64, torch.float64, 0), ("f32", N.RT_OUT_F32, torch.float32, 0),
                                ("u8", N.RT_OUT_U8, torch.uint8, 255), ("u16", N.RT_OUT_U16, torch.uint16, 65535)):
        dst = torch.empty(n, dtype=dt, device="cuda")
        nbytes = n * (8 + dst.element_size())
        ms = min(timed(lambda: N.check(L.rt_resolve(src.data_ptr(), n, 16, fmt, maxv, dst.data_ptr(), None, st)))
                 for _ in range(a.rounds))
        out[name] = {"ms": round(ms, 4), "bytes": nbytes, "gbs": round(nbytes / ms / 1e6, 1),
                     "of_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 3)}
        if maxv:
            ms = min(timed(lambda: N.check(L.rt_quantize(mean.data_ptr(), N.RT_OUT_F64, n, maxv, fmt, dst.data_ptr(),
                                                         None, st))) for _ in range(a.rounds))
            out[name]["rt_quantize_ms"] = round(ms, 4)
            out[name]["rt_quantize_gbs"] = round(nbytes / ms / 1e6, 1)
    return out


def child(a, what, tree=ROOT):
    env = dict(os.environ)
    env.pop("RT_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, f"--tree={os.path.abspath(tree)}"] + [f"--{k.replace('_', '-')}={getattr(a, k)}"
                                                                          for k in ("scene", "size", "depth", "spp", "reps",
                                                                                    "warm", "rounds", "resolve_size")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{what} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    print(f"{what} ({os.path.basename(os.path.abspath(tree))}) done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench(tree, a):
    env = dict(os.environ)
    env.pop("RT_LIB_PATH", None)
    tree = os.path.abspath(tree)
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps),
                        "--warmup", str(a.bench_warmup)], cwd=tree, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(f"bench.py ({os.path.basename(tree)}): {json.loads(line)['value']}", file=sys.stderr, flush=True)
    return json.loads(line)["value"]


def spread(xs):
    return {"min": round(min(xs), 4), "max": round(max(xs), 4), "mean": round(sum(xs) / len(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="s256")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resolve-size", type=int, default=4096)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of an earlier commit to compare against")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["partition", "one_shot", "resolve"])
    a = ap.parse_args()
    if a.child:
        res = {"partition": lambda: partition(a), "one_shot": lambda: partition(a, True),
               "resolve": lambda: resolve_alone(a)}[a.child]()
        print(json.dumps(res), flush=True)
        return
    out = {"config": {k: getattr(a, k) for k in ("scene", "size", "depth", "spp", "reps", "warm", "rounds", "resolve_size")},
           "hbm_peak_gbs": HBM_PEAK_GBS}
    part = child(a, "partition")
    A, B, C = part["one_shot_ms"], part["samples_resolve_f32_ms"], part["single_samples_u8_ms"]
    out["partition"] = {"one_shot_ms": spread(A), "samples_resolve_f32_ms": spread(B), "single_samples_u8_ms": spread(C),
                        "b_minus_a_ms": round(sum(B) / len(B) - sum(A) / len(A), 4),
                        "c_minus_a_ms": round(sum(C) / len(C) - sum(A) / len(A), 4),
                        "one_shot_spread_ms": round(max(A) - min(A), 4), "f32_frames_equal": part["f32_frames_equal"],
                        "rounds": {"a": A, "b": B, "c": C}}
    out["resolve"] = child(a, "resolve")
    if a.parent_tree:
        old, new = [], []
        for _ in range(2):  # alternated child processes
            old += child(a, "one_shot", a.parent_tree)["one_shot_ms"]
            new += child(a, "one_shot")["one_shot_ms"]
        out["one_shot_parent_vs_new_ms"] = {"parent": spread(old), "new": spread(new)}
        bo, bn = [], []
        for _ in range(a.bench_runs):
            bo.append(bench(a.parent_tree, a))
            bn.append(bench(ROOT, a))
        out["bench_headline"] = {"parent": bo, "new": bn, "steps": a.bench_steps, "warmup": a.bench_warmup}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
