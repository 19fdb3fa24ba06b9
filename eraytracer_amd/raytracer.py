"""Host-side mirror of raytracer.erl's strategy interface, backed by the MI355X kernel.

The reference's pixel loop is a strategy fun ``F(Width, Height, Scene, Recursion_depth)``
chosen by ``tracing_function/1`` (raytracer.erl:714-719) and called once by
``raytrace/5`` (raytracer.erl:723-733).  This module provides the same functions with
the same argument meaning and the same results, rendered by ``librtmi355x.so``:

* :func:`raytraced_pixel_list_simple`      — keys all 1, row-major (raytracer.erl:86-99)
* :func:`raytraced_pixel_list_concurrent`  — keys X+Y*Width, sorted (raytracer.erl:101-119, :155)
* :func:`raytraced_pixel_list_distributed` — same pixels and keys, rendered over every
  visible GPU of the process (raytracer.erl:121-149)
* :func:`raytraced_pixel_list_gpu`         — alias of the concurrent form (the new strategy atom ``gpu``)

plus :func:`raytrace`, :func:`go`, :func:`standalone`, :func:`tracing_function` and the
byte-exact ASCII P3 writer :func:`write_pixels_to_ppm` (raytracer.erl:667-685).
:func:`render` returns the framebuffer as a numpy array, for callers that do not want a
W*H-element list.

Error behaviour mirrors the reference: ``(0, 0, ...)`` returns ``'done'``; a width or
height of 0 with the other positive is a ``function_clause`` (ValueError here); a
malformed scene is a ``badarg`` (ValueError) instead of a crash in a worker process.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import time

import numpy as np

from . import _native as N
from .records import scene as default_scene
from .terms import Atom

DONE = Atom("done")


def _sizes_ok(width, height):
    for v, n in ((width, "Width"), (height, "Height")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"function_clause: {n} must be an integer, got {v!r}")
    if width == 0 and height == 0:
        return False
    if not (width > 0 and height > 0):
        raise ValueError("function_clause: Width > 0, Height > 0 required (raytracer.erl:88-89)")
    return True


def _depth_ok(depth):
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 0:
        raise ValueError(f"badarg: Recursion_depth must be a non-negative integer, got {depth!r}")
    if depth >= 1 << 32:  # the C ABI's uint32_t (no other depth limit: RT_ENOMEM when it does not fit)
        raise ValueError(f"badarg: Recursion_depth {depth} does not fit the library's 32-bit depth")


def _max_value_ok(max_value):
    if isinstance(max_value, bool) or not isinstance(max_value, int) or not 0 < max_value < 1 << 32:
        raise ValueError(f"badarg: MaxValue must be an integer in [1, 2^32), got {max_value!r}")


def _window_ok(window, width, height):
    """``window=(x0, y0, w, h)`` checked against the image (RT_WINDOW in include/rt_mi355x.h); None is
    the whole frame.  Returns the four integers."""
    if window is None:
        return 0, 0, width, height
    try:
        x0, y0, w, h = window
    except (TypeError, ValueError):
        raise ValueError(f"badarg: window must be (x0, y0, w, h), got {window!r}") from None
    for v in (x0, y0, w, h):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"badarg: window must hold integers, got {window!r}")
    x0, y0, w, h = int(x0), int(y0), int(w), int(h)
    if x0 < 0 or y0 < 0 or w < 1 or h < 1:
        raise ValueError(f"badarg: window {window!r} is empty or has a negative origin")
    if x0 + w > width or y0 + h > height:
        raise ValueError(f"badarg: window {window!r} leaves the {width}x{height} image")
    return x0, y0, w, h


def render(width: int, height: int, scene=None, depth: int = 5, *, precision: str = "f64",
           order: str = "exact", ndev: int = 1, first_dev: int = 0, row_block: int = 16,
           levels: bool = False, stats: dict | None = None, spp: int = 1, seed: int = 0, out=None,
           nshards: int = 0, max_value: int = 255, window=None):
    """Render through ``rt_render`` and return a ``(height, width, 3)`` array (float64 or
    float32), plus the per-pixel levels array if ``levels``.  ``'done'`` for 0x0.
    ``precision="u8"`` / ``"u16"``: an integer frame (uint8 / uint16) quantised on the GPU,
    every channel ``min(trunc(C*max_value), max_value)`` — the integers write_pixels_to_ppm/5
    prints; a negative or NaN channel is stored as 0 and ``stats["clamped"]`` is then true.
    ``out``: an existing C-contiguous array of that shape and dtype to render into (e.g.
    ``_native.pinned_empty``: pinned memory is written by DMA directly).  ``nshards``: row
    shards of the distributed split (default one per device; shard s on device s % ndev).
    ``spp`` > 1: stochastic supersampling as defined at RT_SUPERSAMPLING in
    include/rt_mi355x.h (not in the reference; levels then report sample 0).
    ``levels="hit"``: the levels array is the primary-hit mask (1 where the primary ray hits,
    RT_LEVELS_HIT) instead of the chain's level count — what the strategy funs need for the
    reference's integer pixels, without turning the fused shading kernels off.
    ``window=(x0, y0, w, h)``: render only that pixel window of the ``width`` x ``height`` image
    (RT_WINDOW in include/rt_mi355x.h): the result is ``(h, w, 3)`` (levels ``(h, w)``), bit for
    bit the crop ``[y0:y0+h, x0:x0+w]`` of the whole frame, and ``out`` must have that shape.  A
    window that is empty or leaves the image raises ValueError before the library is called."""
    if not _sizes_ok(width, height):
        return DONE
    _depth_ok(depth)
    x0, y0, ww, wh = _window_ok(window, width, height)
    prec, dt = {"f64": (N.RT_OUT_F64, np.float64), "f32": (N.RT_OUT_F32, np.float32),
                "u8": (N.RT_OUT_U8, np.uint8), "u16": (N.RT_OUT_U16, np.uint16)}[precision]
    _max_value_ok(max_value)
    if out is None:
        out = np.empty((wh, ww, 3), dtype=dt)
    elif out.shape != (wh, ww, 3) or out.dtype != dt or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {(wh, ww, 3)} {np.dtype(dt).name} array")
    if scene is None:
        scene = default_scene()
    elems = N.marshal(scene)
    L = N.lib()
    lv = np.empty((wh, ww), dtype=np.uint8) if levels else None
    opts = N.RtOpts(ctypes.sizeof(N.RtOpts), first_dev, ndev, prec,
                    {"exact": N.RT_ORDER_EXACT, "fast": N.RT_ORDER_FAST}[order], row_block,
                    lv.ctypes.data if levels else None, spp, nshards, seed,
                    N.RT_LEVELS_HIT if levels == "hit" else 0, max_value,
                    *((x0, y0, ww, wh) if window is not None else (0, 0, 0, 0)))
    st = N.RtStats()
    rc = L.rt_render(elems, len(elems), width, height, depth, ctypes.byref(opts), out.ctypes.data, ctypes.byref(st))
    if rc == N.RT_DONE:
        return DONE
    N.check(rc, "rt_render")
    if stats is not None:
        stats.update(kernel_ms=st.kernel_ms, total_ms=st.total_ms, pixels=st.pixels, ndev=st.ndev,
                     pinned=bool(st.flags & N.RT_STATS_PINNED), clamped=bool(st.flags & N.RT_STATS_CLAMPED))
    return (out, lv) if levels else out


def render_progressive(width: int, height: int, scene=None, depth: int = 5, *, spp: int, seed: int = 0, steps=1,
                       precision: str = "f64", max_value: int = 255, window=None):
    """A supersampled frame a few samples at a time (RT_PROGRESSIVE in include/rt_mi355x.h): an
    iterator of ``(samples_done, array)``, one item per batch of samples, the array the preview of
    the samples so far, ``(height, width, 3)`` (the window's shape with ``window``) in ``precision``.
    ``steps``: the batch size, or a sequence of batch sizes (``progressive.batch_ends``).  The last
    item's array is ``render(width, height, scene, depth, spp=spp, seed=seed, precision=precision,
    max_value=max_value, window=window)`` in every byte.  The sum stays on the device
    (``progressive.ProgressiveFrame``); every item is a copy to the host.  Bad arguments raise
    ValueError here, before the library is loaded and before the first item is asked for."""
    from . import progressive
    if not _sizes_ok(width, height):
        raise ValueError("function_clause: Width > 0, Height > 0 required (raytracer.erl:88-89)")
    _depth_ok(depth)
    ends = progressive.batch_ends(spp, steps)
    progressive.seed_ok(seed)
    progressive.format_ok(precision, max_value)
    _window_ok(window, width, height)
    if scene is None:
        scene = default_scene()
    N.marshal(scene)

    def frames():
        with progressive.ProgressiveFrame(scene, width, height, depth, spp=spp, seed=seed, window=window) as pf:
            for end in ends:
                pf.add(end - pf.samples_done)
                yield end, pf.resolve(precision, max_value).cpu().numpy()
    return frames()


ATTR_PLANES = ("elem", "t", "point", "normal", "albedo")  # rt_attr_planes' order


def _planes_ok(planes, precision):
    """The tuple of plane names; ValueError for names or a precision rt_attr_planes does not have."""
    if isinstance(planes, str) or not all(isinstance(n, str) for n in planes):
        raise ValueError(f"badarg: planes must be a sequence of names from {ATTR_PLANES}, got {planes!r}")
    names = tuple(planes)
    if not names or len(set(names)) != len(names) or any(n not in ATTR_PLANES for n in names):
        raise ValueError(f"badarg: planes must be distinct names from {ATTR_PLANES}, at least one, got {planes!r}")
    if precision not in ("f64", "f32"):
        raise ValueError(f"badarg: precision must be 'f64' or 'f32', got {precision!r}")
    return names


def _plane_buffers(names, precision, lead, dev):
    """A tensor on ``dev`` per name — ``lead`` or ``lead + (3,)`` — and the RtAttrPlanes pointing at them."""
    import torch
    fdt = torch.float64 if precision == "f64" else torch.float32
    buf = {n: torch.empty(lead if n in ("elem", "t") else lead + (3,), dtype=torch.int32 if n == "elem" else fdt,
                          device=dev) for n in names}
    return buf, N.RtAttrPlanes(ctypes.sizeof(N.RtAttrPlanes), N.RT_OUT_F64 if precision == "f64" else N.RT_OUT_F32,
                               *[buf[n].data_ptr() if n in buf else None for n in ATTR_PLANES])


@contextlib.contextmanager
def _prepared(L, elems, dev):
    """The scene ``elems`` prepared on ``dev``: (handle, current stream); synchronised, then released, on exit."""
    import torch
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(elems, len(elems), dev.index, ctypes.byref(p)), "rt_prepare")
    try:
        yield p, torch.cuda.current_stream(dev).cuda_stream
        torch.cuda.synchronize(dev)
    finally:
        L.rt_release(p)


def render_attributes(width: int, height: int, scene=None, *, planes=ATTR_PLANES, precision: str = "f64",
                      window=None, spp: int = 1, seed: int = 0, sample: int = 0, device: int = 0):
    """What every pixel's primary ray hits (``rt_launch_attrs``, RT_ATTRIBUTES in
    include/rt_mi355x.h): a dict of numpy arrays, one per name in ``planes``, shaped like the frame
    (the window's shape with ``window``): ``"elem"`` ``(h, w)`` int32, the index in ``scene`` of the
    object hit or -1; ``"t"`` ``(h, w)``, the distance or +inf; ``"point"``, ``"normal"`` and
    ``"albedo"`` ``(h, w, 3)``, all zero at a miss — float64 or, with ``precision="f32"``, the
    float32 roundings of the same values.  ``spp`` > 1: the ray of sample ``sample`` of an
    ``spp``-sample frame (RT_SUPERSAMPLING).  Bad arguments raise ValueError before the library is
    loaded."""
    if not _sizes_ok(width, height):
        raise ValueError("function_clause: Width > 0, Height > 0 required (raytracer.erl:88-89)")
    x0, y0, ww, wh = _window_ok(window, width, height)
    names = _planes_ok(planes, precision)
    for v, n in ((spp, "spp"), (sample, "sample"), (seed, "seed"), (device, "device")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"badarg: {n} must be an integer, got {v!r}")
    if not 1 <= spp <= N.RT_MAX_SPP:
        raise ValueError(f"badarg: spp must be in [1, {N.RT_MAX_SPP}], got {spp}")
    if not 0 <= sample < spp:
        raise ValueError(f"badarg: sample must be in [0, spp = {spp}), got {sample}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"badarg: seed must be in [0, 2^64), got {seed}")
    if device < 0:
        raise ValueError(f"badarg: device must not be negative, got {device}")
    if scene is None:
        scene = default_scene()
    elems = N.marshal(scene)
    L = N.lib()
    import torch
    dev = torch.device("cuda", int(device))
    buf, arg = _plane_buffers(names, precision, (wh, ww), dev)
    with _prepared(L, elems, dev) as (p, stream):
        # one shard of one row block per 16 rows: the slab is the window's rows
        N.check(L.rt_launch_attrs(p, width, height, x0, y0, ww, wh, 16, 0, 1, int(spp), int(seed), int(sample),
                                  ctypes.byref(arg), stream), "rt_launch_attrs")
    return {n: buf[n].cpu().numpy() for n in names}


def pick(width: int, height: int, x: int, y: int, scene=None):
    """What is under pixel (x, y) of the ``width`` x ``height`` frame: None where the primary ray
    hits nothing, else ``{"elem": i, "term": scene[i], "t": distance, "point": (x, y, z), "normal":
    (x, y, z), "albedo": (r, g, b)}`` — :func:`render_attributes` of the 1x1 window."""
    if not _sizes_ok(width, height):
        raise ValueError("function_clause: Width > 0, Height > 0 required (raytracer.erl:88-89)")
    for v, n in ((x, "x"), (y, "y")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"badarg: {n} must be an integer, got {v!r}")
    if not (0 <= x < width and 0 <= y < height):
        raise ValueError(f"badarg: pixel ({x}, {y}) is outside the {width}x{height} image")
    if scene is None:
        scene = default_scene()
    a = render_attributes(width, height, scene, window=(int(x), int(y), 1, 1))
    i = int(a["elem"][0, 0])
    if i < 0:
        return None
    return {"elem": i, "term": scene[i], "t": float(a["t"][0, 0]),
            **{n: tuple(float(v) for v in a[n][0, 0]) for n in ("point", "normal", "albedo")}}


def _triples(a, what, n=None, shared=False):
    """``a`` as a C-contiguous float64 ``(n, 3)`` array — or ``(3,)`` where ``shared`` allows one point
    for the whole batch; ValueError for anything that is not an array of real numbers of that shape."""
    try:
        arr = np.asarray(a)
    except Exception:
        raise ValueError(f"badarg: {what} is not an array") from None
    if arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.integer) or np.issubdtype(arr.dtype, np.floating)):
        raise ValueError(f"badarg: {what} must hold real numbers, got dtype {arr.dtype}")
    ok = (arr.ndim == 2 and arr.shape[1] == 3) or (shared and arr.shape == (3,))
    if not ok:
        raise ValueError(f"badarg: {what} must be (n, 3){' or (3,)' if shared else ''}, got {arr.shape}")
    if arr.ndim == 2 and n is not None and arr.shape[0] != n:
        raise ValueError(f"badarg: {what} holds {arr.shape[0]} rows, expected {n}")
    if arr.ndim == 2 and arr.shape[0] > N.RT_MAX_QUERY_RAYS:
        raise ValueError(f"badarg: {what} holds more than RT_MAX_QUERY_RAYS = {N.RT_MAX_QUERY_RAYS} rows")
    return np.array(arr, dtype=np.float64, order="C")  # (a copy: the caller's array may be read-only)


def _device_ok(device):
    if isinstance(device, bool) or not isinstance(device, (int, np.integer)) or device < 0:
        raise ValueError(f"badarg: device must be a non-negative integer, got {device!r}")


def nearest_hits(origins, directions, scene=None, *, planes=ATTR_PLANES, precision: str = "f64", device: int = 0):
    """The nearest hit of ``n`` rays of the caller's choosing (``rt_query_rays``, RT_QUERY in
    include/rt_mi355x.h): ``directions`` is ``(n, 3)``, used as given (not normalised); ``origins`` is
    ``(n, 3)`` or ``(3,)``, one origin for every ray.  Returns a dict of numpy arrays like
    :func:`render_attributes`, one per name in ``planes``: ``"elem"`` ``(n,)`` int32 and ``"t"`` ``(n,)``,
    ``"point"``, ``"normal"`` and ``"albedo"`` ``(n, 3)`` — a miss is -1, +inf and zeros.  Bad arguments
    raise ValueError before the library is loaded."""
    d = _triples(directions, "directions")
    n = d.shape[0]
    o = _triples(origins, "origins", n, shared=True)
    names = _planes_ok(planes, precision)
    _device_ok(device)
    if scene is None:
        scene = default_scene()
    elems = N.marshal(scene)
    if n == 0:  # nothing to launch (and an empty tensor has no address to hand over)
        fnp = np.float64 if precision == "f64" else np.float32
        return {p: np.empty((0,) if p in ("elem", "t") else (0, 3), dtype=np.int32 if p == "elem" else fnp) for p in names}
    L = N.lib()
    import torch
    dev = torch.device("cuda", int(device))
    buf, arg = _plane_buffers(names, precision, (n,), dev)
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with _prepared(L, elems, dev) as (ctx, stream):
        N.check(L.rt_query_rays(ctx, d_o.data_ptr(), d_d.data_ptr(), n, N.RT_QUERY_ONE_ORIGIN if o.ndim == 1 else 0,
                                ctypes.byref(arg), stream), "rt_query_rays")
    return {p: buf[p].cpu().numpy() for p in names}


def shadow_factors(lights, hits, elems, scene=None, *, device: int = 0):
    """``shadow_factor/4`` for ``n`` triples (``rt_query_shadow``): ``hits`` is ``(n, 3)``, ``lights``
    ``(n, 3)`` or ``(3,)`` (one light location for all), ``elems`` ``(n,)`` integers, the index in
    ``scene`` of the object each hit point lies on.  Returns a ``(n,)`` uint8 array: 1 where the nearest
    object along the ray from the light towards the hit point is that element (or a bit-identical copy
    of it), 0 otherwise.  Bad arguments raise ValueError before the library is loaded."""
    h = _triples(hits, "hits")
    n = h.shape[0]
    lt = _triples(lights, "lights", n, shared=True)
    try:
        e = np.asarray(elems)
    except Exception:
        raise ValueError("badarg: elems is not an array") from None
    if e.dtype == np.bool_ or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"badarg: elems must hold integers, got dtype {e.dtype}")
    if e.shape != (n,):
        raise ValueError(f"badarg: elems must be ({n},), got {e.shape}")
    if n and (e.min() < -(1 << 31) or e.max() >= 1 << 31):
        raise ValueError("badarg: elems must fit 32-bit integers")
    _device_ok(device)
    if scene is None:
        scene = default_scene()
    marshalled = N.marshal(scene)
    if n == 0:
        return np.empty((0,), dtype=np.uint8)
    L = N.lib()
    import torch
    dev = torch.device("cuda", int(device))
    d_l, d_h = torch.from_numpy(lt).to(dev), torch.from_numpy(h).to(dev)
    d_e = torch.from_numpy(np.array(e, dtype=np.int32, order="C")).to(dev)
    lit = torch.empty((n,), dtype=torch.uint8, device=dev)
    with _prepared(L, marshalled, dev) as (ctx, stream):
        N.check(L.rt_query_shadow(ctx, d_l.data_ptr(), d_h.data_ptr(), d_e.data_ptr(), n,
                                  N.RT_QUERY_ONE_ORIGIN if lt.ndim == 1 else 0, lit.data_ptr(), stream), "rt_query_shadow")
    return lit.cpu().numpy()


def trace_rays(origins, directions, depth, scene=None, *, precision: str = "f64", levels: bool = False, device: int = 0):
    """The colour each of ``n`` rays of the caller's choosing sees (``rt_query_colours``, RT_QUERY in
    include/rt_mi355x.h): ``pixel_colour_from_ray(Ray, Scene, depth)`` in the reference's fold order.
    ``directions`` is ``(n, 3)``, used as given (not normalised); ``origins`` is ``(n, 3)`` or ``(3,)``, one
    origin for every ray.  Returns an ``(n, 3)`` array — float64 or, with ``precision="f32"``, the float32
    roundings of the same values — and with ``levels=True`` also an ``(n,)`` uint8 array, the number of
    objects each ray's reflection chain hit (0: a miss).  Bad arguments raise ValueError before the
    library is loaded."""
    d = _triples(directions, "directions")
    n = d.shape[0]
    o = _triples(origins, "origins", n, shared=True)
    _depth_ok(depth)
    if precision not in ("f64", "f32"):
        raise ValueError(f"badarg: precision must be 'f64' or 'f32', got {precision!r}")
    if not isinstance(levels, (bool, np.bool_)):
        raise ValueError(f"badarg: levels must be a bool, got {levels!r}")
    _device_ok(device)
    if scene is None:
        scene = default_scene()
    elems = N.marshal(scene)
    fnp = np.float64 if precision == "f64" else np.float32
    if n == 0:  # nothing to launch (and an empty tensor has no address to hand over)
        rgb = np.empty((0, 3), dtype=fnp)
        return (rgb, np.empty((0,), dtype=np.uint8)) if levels else rgb
    L = N.lib()
    import torch
    dev = torch.device("cuda", int(device))
    need = L.rt_query_colours_work_bytes(n, int(depth))
    if need == 0 and depth != 0:
        raise ValueError(f"badarg: the work space of {n} rays at depth {depth} overflows size_t")
    rgb = torch.empty((n, 3), dtype=torch.float64 if precision == "f64" else torch.float32, device=dev)
    lv = torch.empty((n,), dtype=torch.uint8, device=dev) if levels else None
    work = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None  # (torch allocations are 16-byte aligned)
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with _prepared(L, elems, dev) as (ctx, stream):
        N.check(L.rt_query_colours(ctx, d_o.data_ptr(), d_d.data_ptr(), n, int(depth),
                                   N.RT_QUERY_ONE_ORIGIN if o.ndim == 1 else 0,
                                   N.RT_OUT_F64 if precision == "f64" else N.RT_OUT_F32, rgb.data_ptr(),
                                   lv.data_ptr() if levels else None, work.data_ptr() if need else None, need, stream),
                "rt_query_colours")
    out = rgb.cpu().numpy()
    return (out, lv.cpu().numpy()) if levels else out


def _vec3(v, what):
    try:
        a = np.array(v, dtype=np.float64)
    except Exception:
        raise ValueError(f"badarg: {what} is not a vector of three numbers: {v!r}") from None
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"badarg: {what} must be three finite numbers, got {v!r}")
    return a


def view_rays(width: int, height: int, eye, target, up=(0, 1, 0), fov=90):
    """The rays of a look-at pinhole camera: ``(eye (3,), directions (height*width, 3))``, float64,
    row-major, computed in numpy::

        fwd   = normalize(target - eye)
        right = normalize(cross(up, fwd))
        down  = cross(fwd, right)
        hw    = tan(fov / 2)            (fov in degrees, the horizontal angle)
        hh    = hw * height / width
        pixel (x, y) looks along  normalize(fwd + (x/W - 0.5) 2 hw right + (y/H - 0.5) 2 hh down)

    With ``eye`` at the reference camera looking along +z and ``up = (0, 1, 0)``, ``right`` is +x and
    ``down`` is +y: the image has the reference's orientation (``point_on_screen/3``,
    raytracer.erl:486-503).  The direction is evaluated as the reference evaluates its own, on a screen
    of width 1 at the focal distance ``F = 1 / (2 hw)`` (``focal_length/2``, :483-484): the vector above
    times F, ``F fwd + (x/W - 0.5) right + ((y/H - 0.5) H/W) down``, with the angle as ``fov * (pi / 180) /
    2`` and ``vector_normalize/1``'s multiplication by ``1 / mag`` — so that a frame aimed like the
    reference camera is the rendered frame, not a neighbour of it one rounding away (a reflection chain
    can turn one unit in the last place of a direction into another colour).  ValueError for
    ``target == eye``, an ``up`` parallel to ``fwd`` and a ``fov`` outside (0, 180)."""
    if not _sizes_ok(width, height):
        raise ValueError("function_clause: Width > 0, Height > 0 required (raytracer.erl:88-89)")
    e, t, u = _vec3(eye, "eye"), _vec3(target, "target"), _vec3(up, "up")
    if isinstance(fov, bool) or not isinstance(fov, (int, float, np.integer, np.floating)) or not 0 < fov < 180:
        raise ValueError(f"badarg: fov must be a number of degrees in (0, 180), got {fov!r}")
    fwd = t - e
    if not fwd.any():
        raise ValueError("badarg: target == eye: the camera looks nowhere")
    fwd = fwd * (1 / math.sqrt(fwd @ fwd))
    right = np.cross(u, fwd)
    if not math.sqrt(right @ right) > 1e-12 * math.sqrt(u @ u):
        raise ValueError("badarg: up is parallel to the viewing direction (or zero)")
    right = right * (1 / math.sqrt(right @ right))
    down = np.cross(fwd, right)
    focal = 1 / (2 * math.tan(float(fov) * (math.pi / 180) / 2))
    sx = np.arange(width) / width - 0.5
    sy = (np.arange(height) / height - 0.5) * (height / width)
    v = (focal * fwd)[None, None, :] + sx[None, :, None] * right[None, None, :] + sy[:, None, None] * down[None, None, :]
    m2 = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    d = v * (1 / np.sqrt(m2))[..., None]
    return e, np.ascontiguousarray(d.reshape(height * width, 3))


def render_view(width: int, height: int, depth: int, scene=None, *, eye, target, up=(0, 1, 0), fov=90,
                precision: str = "f64", device: int = 0):
    """A frame from a camera that is aimed: the ``(height, width, 3)`` colours of exactly the rays
    :func:`view_rays` returns, traced by :func:`trace_rays` — nothing else.  The scene's own #camera{}
    is not used (the reference camera's path, :func:`render`, is untouched)."""
    e, d = view_rays(width, height, eye, target, up, fov)
    return trace_rays(e, d, depth, scene, precision=precision, device=device).reshape(height, width, 3)


def _has_lights(scene) -> bool:
    from .records import tag
    return any(tag(t) == "point_light" for t in scene)


def _pixel_list(img, lv, scene, keyed: bool):
    """The strategy's result list with the reference's exact term types: the integer zeros
    #colour{r=0,g=0,b=0} where the reference returns them — no primary hit (?BACKGROUND_COLOUR,
    raytracer.erl:82, :201), depth 0 (:186-187; the hit mask is 0 there) or a scene without point
    lights (lighting_function/6 folds from #vector{0,0,0}, :250) — floats everywhere else
    (specular_term's math:pow/2 always yields a float, :289).  Keys: 1 (simple, :95) or
    X+Y*Width (:112, :173).  lv: the primary-hit mask or the level counts (0 = no hit either way)."""
    flat = img.reshape(-1, 3).tolist()
    zero = (lv.reshape(-1) == 0) if _has_lights(scene) else np.ones(len(flat), dtype=bool)
    ints = (0, 0, 0)
    if keyed:
        return [(i, ints if z else (r, g, b)) for i, ((r, g, b), z) in enumerate(zip(flat, zero.tolist()))]
    return [(1, ints if z else (r, g, b)) for (r, g, b), z in zip(flat, zero.tolist())]


def _strategy(Width, Height, Scene, Recursion_depth, keyed, ndev=1):
    if not _sizes_ok(Width, Height):
        return DONE
    if Scene is None:
        Scene = default_scene()
    img, lv = render(Width, Height, Scene, Recursion_depth, levels="hit", ndev=ndev)
    return _pixel_list(img, lv, Scene, keyed)


def raytraced_pixel_list_simple(Width, Height, Scene, Recursion_depth):
    """raytraced_pixel_list_simple/4 (raytracer.erl:86-99): ``[{1, {R,G,B}}]`` row-major."""
    return _strategy(Width, Height, Scene, Recursion_depth, keyed=False)


def raytraced_pixel_list_concurrent(Width, Height, Scene, Recursion_depth):
    """raytraced_pixel_list_concurrent/4 (raytracer.erl:101-119): ``[{X+Y*W, {R,G,B}}]``
    sorted by key (the master's lists:keysort, :155), i.e. row-major."""
    return _strategy(Width, Height, Scene, Recursion_depth, keyed=True)


def raytraced_pixel_list_distributed(Width, Height, Scene, Recursion_depth):
    """raytraced_pixel_list_distributed/4 (raytracer.erl:121-149): the same pixels and
    keys as concurrent; rows are sharded over every GPU visible to this process."""
    return _strategy(Width, Height, Scene, Recursion_depth, keyed=True, ndev=-1)


raytraced_pixel_list_gpu = raytraced_pixel_list_concurrent


def tracing_function(strategy):
    """tracing_function/1 (raytracer.erl:714-719), plus the ``gpu`` atom."""
    table = {
        "simple": raytraced_pixel_list_simple,
        "concurrent": raytraced_pixel_list_concurrent,
        "distributed": raytraced_pixel_list_distributed,
        "gpu": raytraced_pixel_list_gpu,
    }
    try:
        return table[str(strategy)]
    except KeyError:
        raise ValueError(f"function_clause: unknown strategy {strategy!r}") from None


def _erl_int(x: float) -> int:
    """trunc/1 of a float (toward zero)."""
    return int(x)


def write_pixels_to_ppm(Width, Height, MaxValue, Pixels, Filename):
    """write_pixels_to_ppm/5 (raytracer.erl:667-685): ASCII P3, every channel written as
    ``min(trunc(C*MaxValue), MaxValue)`` followed by one space; keys are ignored.
    Accepts the pixel list or a (H, W, 3) array."""
    with open(Filename, "w", encoding="ascii", newline="\n") as f:
        f.write("P3\n")
        f.write(f"{Width} {Height}\n")
        f.write(f"{MaxValue}\n")
        if isinstance(Pixels, np.ndarray):
            x = np.minimum(np.trunc(Pixels.astype(np.float64).reshape(-1, 3) * MaxValue), MaxValue)
            if np.all(x > -2.0 ** 62):
                rows = x.astype(np.int64).tolist()
            else:  # BEAM integers are unbounded: exact Python ints for huge negative values
                rows = [[int(v) for v in px] for px in x.tolist()]
            f.write("".join(f"{r} {g} {b} " for r, g, b in rows))
        else:
            parts = []
            for _key, (r, g, b) in Pixels:
                parts.append(f"{min(_erl_int(r * MaxValue), MaxValue)} {min(_erl_int(g * MaxValue), MaxValue)} "
                             f"{min(_erl_int(b * MaxValue), MaxValue)} ")
            f.write("".join(parts))


def write_pixels_to_p6(Width, Height, MaxValue, Pixels, Filename):
    """The binary sibling of :func:`write_pixels_to_ppm` (not in the reference): the header
    ``P6\\nW H\\nMaxValue\\n`` followed by the same integers ``min(trunc(C*MaxValue), MaxValue)``
    as samples, 1 byte each for MaxValue <= 255, else 2 bytes each, most significant byte first.
    Accepts the pixel list or a (H, W, 3) array; a value P3 would print as negative cannot be a
    sample and raises ValueError (so does a NaN), before the file is opened.  The host mirror of
    rt_render_rawppm_file."""
    if isinstance(MaxValue, bool) or not isinstance(MaxValue, int) or not 0 < MaxValue <= N.RT_MAX_INT_VALUE:
        raise ValueError(f"badarg: MaxValue must be an integer in [1, {N.RT_MAX_INT_VALUE}], got {MaxValue!r}")
    if isinstance(Pixels, np.ndarray):
        c = Pixels.astype(np.float64).reshape(-1)
    else:
        c = np.array([[float(r), float(g), float(b)] for _key, (r, g, b) in Pixels], dtype=np.float64).reshape(-1)
    if c.size != Width * Height * 3:
        raise ValueError(f"badarg: {c.size} channels for a {Width}x{Height} frame")
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.trunc(c * float(MaxValue))
        bad = ~(t >= 0)  # negative (not -0.0) or NaN
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"channel {k % 3} of pixel {k // 3} is {c[k]!r}: no unsigned sample holds it")
    q = np.minimum(t, float(MaxValue)).astype(">u2" if MaxValue > 255 else np.uint8)
    with open(Filename, "wb") as f:
        f.write(f"P6\n{Width} {Height}\n{MaxValue}\n".encode("ascii"))
        f.write(q.tobytes())


def quantize_gpu(img, max_value: int = 255, dtype=np.uint8):
    """An array of binary64 or binary32 channels quantised on the GPU (rt_quantize) to ``dtype``
    (uint8 or uint16): ``(array of img's shape, clamped_count)``, the count being the values
    stored as 0 because they were negative or NaN.  The sibling of :func:`ppm_text_gpu`."""
    import torch
    L = N.lib()
    dt = np.dtype(dtype)
    fmt = {np.dtype(np.uint8): N.RT_OUT_U8, np.dtype(np.uint16): N.RT_OUT_U16}[dt]
    prec = N.RT_OUT_F64 if img.dtype == np.float64 else N.RT_OUT_F32
    src = np.ascontiguousarray(img, dtype=np.float64 if prec == N.RT_OUT_F64 else np.float32)
    d = torch.from_numpy(src).cuda()
    out = torch.empty(max(src.size, 1) * dt.itemsize, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    N.check(L.rt_quantize(d.data_ptr(), prec, src.size, max_value, fmt, out.data_ptr(), cnt.data_ptr(), st),
            "rt_quantize")
    torch.cuda.synchronize()
    return out[: src.size * dt.itemsize].cpu().numpy().view(dt).reshape(src.shape), int(cnt.item())


def raytrace(Width=4, Height=3, Filename="/tmp/traced.ppm", Recursion_depth=5, Function=None):
    """raytrace/1,5 (raytracer.erl:721-733): render scene() with Function, write the PPM.
    The GPU strategy goes through rt_render_ppm_file (the P3 text is produced on the GPU,
    byte-identical to write_pixels_to_ppm)."""
    if Function is None:
        Function = raytraced_pixel_list_gpu
    if Function is raytraced_pixel_list_gpu:
        return render_ppm_file(Width, Height, default_scene(), Recursion_depth, Filename)
    pixels = Function(Width, Height, default_scene(), Recursion_depth)
    return write_pixels_to_ppm(Width, Height, 255, pixels, Filename)


def render_ppm_file(width: int, height: int, scene, depth: int, filename: str, *, max_value: int = 255,
                    ndev: int = 1, first_dev: int = 0, spp: int = 1, seed: int = 0, binary: bool = False,
                    window=None):
    """Render and write the P3 file natively (rt_render_ppm_file): raytrace/5 + write_pixels_to_ppm/5.
    ``binary=True``: the P6 file of the same integers (rt_render_rawppm_file; see
    :func:`write_pixels_to_p6`); a frame with a negative value raises RtError (RT_ERANGE) and
    no file is written.  ``window=(x0, y0, w, h)``: the file is that window of the image, a
    ``w`` x ``h`` file (see :func:`render`)."""
    if not _sizes_ok(width, height):
        return DONE
    _depth_ok(depth)
    if binary:
        _max_value_ok(max_value)
    win = _window_ok(window, width, height) if window is not None else (0, 0, 0, 0)
    elems = N.marshal(scene)
    opts = N.RtOpts(ctypes.sizeof(N.RtOpts), first_dev, ndev, N.RT_OUT_F64, N.RT_ORDER_EXACT, 16, None, spp, 0, seed,
                    0, 0, *win)
    what = "rt_render_rawppm_file" if binary else "rt_render_ppm_file"
    rc = getattr(N.lib(), what)(elems, len(elems), width, height, depth, ctypes.byref(opts), max_value,
                                str(filename).encode(), None)
    if rc == N.RT_DONE:
        return DONE
    N.check(rc, what)
    return "ok"


def ppm_text_gpu(img, max_value: int = 255) -> bytes:
    """The P3 bytes of an (H, W, 3) frame formatted on the GPU (rt_ppm_format); RT_ERANGE
    (a channel below -2^31 after scaling) raises."""
    import torch
    L = N.lib()
    h, w, _ = img.shape
    prec = N.RT_OUT_F64 if img.dtype == np.float64 else N.RT_OUT_F32
    d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    cap = L.rt_ppm_bound(w, h, max_value)
    buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = ctypes.c_size_t(0)
    st = torch.cuda.current_stream().cuda_stream
    N.check(L.rt_ppm_format(d.data_ptr(), prec, w, h, max_value, buf.data_ptr(), cap, ctypes.byref(n), st),
            "rt_ppm_format")
    return bytes(buf[: n.value].cpu().numpy())


def go(Strategy, Width=None, Height=None, Filename=None, Recursion_depth=None):
    """go/1 (4x3, depth 5, /tmp/traced.ppm; raytracer.erl:707-708, :721-722) and go/5 (:710-712)."""
    if Width is None:
        return raytrace(Function=tracing_function(Strategy))
    return raytrace(Width, Height, Filename, Recursion_depth, tracing_function(Strategy))


def standalone(Width, Height, Filename, Recursion_depth, Strategy):
    """standalone/1,5 (raytracer.erl:688-705): time raytrace/5 (PPM write included, as in
    the reference) and print ``Done in ~w seconds``."""
    t0 = time.perf_counter()
    raytrace(int(Width), int(Height), Filename, int(Recursion_depth), tracing_function(Strategy))
    dt = time.perf_counter() - t0
    print(f"Done in {dt!r} seconds")
    return dt


if __name__ == "__main__":  # python -m eraytracer_amd.raytracer W H File Depth Strategy (cf. run*.sh)
    import sys
    if len(sys.argv) != 6:
        sys.exit("usage: python -m eraytracer_amd.raytracer Width Height Filename Depth Strategy")
    standalone(*sys.argv[1:])
