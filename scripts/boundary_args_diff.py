"""Return codes of the boundary's entry points over a grid of bad-argument combinations, to compare
two builds of the library (RT_LIB_PATH picks the build; one process per build):

    RT_LIB_PATH=old.so python scripts/boundary_args_diff.py dump old.json
    RT_LIB_PATH=new.so python scripts/boundary_args_diff.py dump new.json
    python scripts/boundary_args_diff.py compare old.json new.json

Every combination is one the library answers without launching anything: it is refused by an
argument check, returns early (no values, no pixels), or ends at the device count (RT_ENODEV on a
machine without a GPU, where `dump` is meant to run; `dump --gpu` is the handful of calls whose check
sits behind the device count, for a machine with one).  Pointers are made-up addresses: no check
dereferences them.
"""
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eraytracer_amd import _native as N  # noqa: E402
from eraytracer_amd import records  # noqa: E402

PRECS = list(range(-1, 5))
MAXV = [0, 255, 256, 65535, 65536]
BIG = (1 << 20) + 1


def opts_blocks():
    """(label, RtOpts or None) over precision, max_value, order, spp, window, nshards, devices, struct_size."""
    full = ctypes.sizeof(N.RtOpts)
    windows = [(0, 0, 0, 0), (0, 0, 4, 4), (4, 4, 4, 4), (5, 0, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (1, 0, 0, 0),
               (0xFFFFFFFF, 0, 2, 2)]
    yield "null", None
    for prec, maxv, order, spp, win, ns, (first, ndev), size in itertools.product(
            PRECS, MAXV, (0, 1, 2), (0, 4096, 4097), windows, (0, 64, 65), ((0, 1), (-1, 1), (0, 0), (0, -1), (0, 2)),
            (full, N.RtOpts.spp.offset, N.RtOpts.max_value.offset, N.RtOpts.win_x0.offset, 0)):
        # thin the product: vary the late fields only around the defaults of the early ones
        plain = (prec in (0, 2) and maxv in (0, 255) and order == 0 and spp == 0)
        if not plain and (win != windows[0] or ns != 0 or (first, ndev) != (0, 1) or size != full):
            continue
        o = N.RtOpts(struct_size=size, first_dev=first, ndev=ndev, precision=prec, order=order, row_block=0, spp=spp,
                     nshards=ns, max_value=maxv, win_x0=win[0], win_y0=win[1], win_w=win[2], win_h=win[3])
        yield f"p{prec} m{maxv} o{order} s{spp} w{win} ns{ns} d{first},{ndev} z{size}", o


def calls(gpu):
    L = N.lib()
    scene = N.marshal(records.scene())
    bad_scene = N.marshal(records.scene()[:1])  # a lone camera
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "boundary_args_diff.ppm").encode()
    out = ctypes.create_string_buffer(8 * 8 * 3 * 8)
    optr = ctypes.addressof(out)
    if gpu:  # check 13 (nshards > RT_MAX_SHARDS) and the writers' way to it through rt_render
        o = N.RtOpts(struct_size=ctypes.sizeof(N.RtOpts), ndev=-1, nshards=65)
        yield "rt_render", "ns65", L.rt_render(scene, len(scene), 8, 8, 1, ctypes.byref(o), optr, None)
        yield "rt_render_ppm_file", "ns65", L.rt_render_ppm_file(scene, len(scene), 8, 8, 1, ctypes.byref(o), 255, path, None)
        yield "rt_render_rawppm_file", "ns65", L.rt_render_rawppm_file(scene, len(scene), 8, 8, 1, ctypes.byref(o), 255, path, None)
        return
    sizes = [(0, 0), (0, 8), (8, 0), (8, 8), (BIG, 8), (8, BIG)]
    for (label, o), (w, h), dst, sc in itertools.product(opts_blocks(), sizes, (None, optr), (scene, bad_scene)):
        ref = ctypes.byref(o) if o is not None else None
        yield "rt_render", f"{label} {w}x{h} out{dst is not None} sc{len(sc)}", L.rt_render(sc, len(sc), w, h, 1, ref, dst, None)
    for (label, o), (w, h), maxv, pth in itertools.product(opts_blocks(), sizes[:4], MAXV, (None, path)):
        ref = ctypes.byref(o) if o is not None else None
        what = f"{label} {w}x{h} m{maxv} path{pth is not None}"
        yield "rt_render_ppm_file", what, L.rt_render_ppm_file(scene, len(scene), w, h, 1, ref, maxv, pth, None)
        yield "rt_render_rawppm_file", what, L.rt_render_rawppm_file(scene, len(scene), w, h, 1, ref, maxv, pth, None)
    esz = {0: 8, 1: 4, 2: 1, 3: 2}
    limit = {2: 255, 3: 65535}
    for src, prec, nval, maxv, fmt, dst, cl in itertools.product((0, 0x1000, 0x1004, 0x1002), PRECS, (0, 100), MAXV, PRECS,
                                                                 (0, 0x2000, 0x2001), (0, 0x3000, 0x3004)):
        ok = (src and dst and prec in (0, 1) and fmt in (2, 3) and 0 < maxv <= limit[fmt] and src % esz[prec] == 0
              and dst % esz[fmt] == 0 and cl % 8 == 0)
        if not (ok and nval):  # a valid call with values launches
            yield "rt_quantize", f"{src:#x} p{prec} n{nval} m{maxv} f{fmt} {dst:#x} {cl:#x}", L.rt_quantize(
                src, prec, nval, maxv, fmt, dst, cl, None)
    for src, nval, samples, fmt, maxv, dst, cl in itertools.product((0, 0x1000, 0x1004), (0, 100), (0, 1, 4096, 4097), PRECS,
                                                                    MAXV, (0, 0x2000, 0x2001, 0x2002, 0x2004),
                                                                    (0, 0x3000, 0x3004)):
        ok = (src and dst and fmt in esz and 0 < samples <= 4096 and (fmt < 2 or 0 < maxv <= limit[fmt])
              and src % 8 == 0 and dst % esz[fmt] == 0 and cl % 8 == 0)
        if not (ok and nval):
            yield "rt_resolve", f"{src:#x} n{nval} s{samples} f{fmt} m{maxv} {dst:#x} {cl:#x}", L.rt_resolve(
                src, nval, samples, fmt, maxv, dst, cl, None)
    dims = (0, 64, 1 << 20)
    vp64 = ctypes.c_void_p * 65
    for slab, w, h, rb, ns, shard, prec, hdr, vals in itertools.product((0, 0x1000, 0x1001), dims, dims, (0, 16), (0, 1, 64, 65),
                                                                        (0, 1, 64), PRECS, (0, 0x2000), (0, 0x3000, 0x3001)):
        ok = (slab and hdr and vals and w and h and rb and 0 < ns <= 64 and shard < ns and prec in esz
              and (prec != 3 or (slab % 2 == 0 and vals % 2 == 0)))
        px = w * (-(-h // (rb * ns)) * rb) if rb and ns else 0
        if not ok or px >= 1 << 32:  # a valid slab of fewer than 2^32 pixels launches
            yield "rt_slab_pack", f"{slab:#x} {w}x{h} rb{rb} {shard}/{ns} p{prec} {hdr:#x} {vals:#x}", L.rt_slab_pack(
                slab, w, h, rb, shard, ns, prec, hdr, vals, None)
    for hole, vbase, w, h, rb, ns, prec, img, arrays in itertools.product((None, 0, 63), (0x3000, 0x3001), dims, dims, (0, 16),
                                                                          (0, 1, 64, 65), PRECS, (0, 0x4000, 0x4001),
                                                                          (True, False)):
        hdrs = vp64(*[0x2000 + 64 * s for s in range(65)])
        vals = vp64(*[vbase + 64 * s for s in range(65)])
        if hole is not None:
            hdrs[hole] = None
        ok = (arrays and img and w and h and rb and 0 < ns <= 64 and prec in esz and (hole is None or hole >= ns)
              and (prec != 3 or (img % 2 == 0 and vbase % 2 == 0)))
        px = w * (-(-h // (rb * ns)) * rb) if rb and ns else 0
        wide = img % 16 == 0 and w % {0: 4, 1: 4, 2: 16, 3: 8}.get(prec, 1) == 0
        per_wg = 256 * ({0: 4, 1: 4, 2: 16, 3: 8}.get(prec, 1) if wide else 1)
        if not ok or px >= 1 << 32 or -(-w // per_wg) * h >= 1 << 31:
            yield "rt_slab_unpack", f"hole{hole} {vbase:#x} {w}x{h} rb{rb} ns{ns} p{prec} {img:#x} arr{arrays}", L.rt_slab_unpack(
                hdrs if arrays else None, vals if arrays else None, w, h, rb, ns, prec, img, None)
    for slabs, w, h, rb, ns, prec, img in itertools.product((0, 0x1000), dims[:2], dims[:2], (0, 16), (0, 1, 65), PRECS,
                                                            (0, 0x4000)):
        if not (slabs and img and w and h and rb and ns and prec in esz):  # a valid call copies
            yield "rt_unshard", f"{slabs:#x} {w}x{h} rb{rb} ns{ns} p{prec} {img:#x}", L.rt_unshard(
                slabs, w, h, rb, ns, prec, img, None)
    n = ctypes.c_size_t(0)
    for src, prec, (w, h), maxv, txt, cap, ln in itertools.product((0, 0x1000), PRECS, ((0, 0), (8, 8), (0, 8)), MAXV,
                                                                   (0, 0x2000), (0, 1 << 20), (None, ctypes.byref(n))):
        ok = src and txt and ln is not None and prec in (0, 1)
        if not ok or (w * h == 0 and cap == 0):  # no pixels and no room for the header: refused before any copy
            yield "rt_ppm_format", f"{src:#x} p{prec} {w}x{h} m{maxv} {txt:#x} cap{cap} len{ln is not None}", L.rt_ppm_format(
                src, prec, w, h, maxv, txt, cap, ln, None)


def main():
    if sys.argv[1] == "dump":
        gpu = "--gpu" in sys.argv
        rows = [[e, what, rc] for e, what, rc in calls(gpu)]
        json.dump(rows, open([a for a in sys.argv[2:] if a != "--gpu"][0], "w"))
        return
    a, b = (json.load(open(p)) for p in sys.argv[2:4])
    assert [r[:2] for r in a] == [r[:2] for r in b], "the two dumps are of different grids"
    counts, diffs = {}, []
    for (e, what, ra), (_, _, rb) in zip(a, b):
        counts[e] = counts.get(e, 0) + 1
        if ra != rb:
            diffs.append((e, what, ra, rb))
    for e, c in counts.items():
        codes = sorted({r[2] for r in a if r[0] == e})
        print(f"{e:24s} {c:7d} combinations, return codes seen {codes}, differing {sum(d[0] == e for d in diffs)}")
    print(f"{'all':24s} {len(a):7d} combinations, differing {len(diffs)}")
    for d in diffs[:40]:
        print("DIFF", *d)
    sys.exit(1 if diffs else 0)


if __name__ == "__main__":
    main()
