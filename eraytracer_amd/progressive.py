"""Progressive supersampling (RT_PROGRESSIVE in include/rt_mi355x.h): a supersampled frame rendered
a few samples at a time into a binary64 sum that stays on the device, and a preview of the samples
so far whenever one is wanted.  The preview after the last sample is the frame ``rt_launch_window``
renders in one go, in every byte.

:class:`ProgressiveFrame` owns a prepared context and the sum, as ``dist.FrameRenderer`` owns its
slabs.  Arguments are checked before the library is loaded.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .dist import INT_LIMITS, PRECISIONS as FORMATS, shard_global_rows, shard_rows


def _int_ok(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def spp_ok(spp):
    if not _int_ok(spp) or not 1 <= spp <= N.RT_MAX_SPP:
        raise ValueError(f"badarg: spp must be an integer in [1, {N.RT_MAX_SPP}], got {spp!r}")
    return int(spp)


def seed_ok(seed):
    if not _int_ok(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"badarg: seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def format_ok(precision, max_value):
    """The (RT_OUT_* format, max_value) of a preview; max_value is read for "u8" / "u16" only."""
    if precision not in FORMATS:
        raise ValueError(f"badarg: precision must be one of {sorted(FORMATS)}, got {precision!r}")
    if precision in INT_LIMITS and (not _int_ok(max_value) or not 0 < max_value <= INT_LIMITS[precision]):
        raise ValueError(f"badarg: MaxValue of a {precision} frame must be an integer in "
                         f"[1, {INT_LIMITS[precision]}], got {max_value!r}")
    return FORMATS[precision], int(max_value) if precision in INT_LIMITS else 0


def batch_ends(spp, steps=1):
    """``samples_done`` after each batch of a ``spp``-sample frame: increasing, the last one ``spp``.
    ``steps``: an int, the size of every batch, or a sequence of batch sizes; a sequence that ends
    before ``spp`` is continued with its last size, and the batch that reaches ``spp`` is cut there.
    ``batch_ends(4, (1, 1, 2)) == [1, 2, 4]``, ``batch_ends(8, 3) == [3, 6, 8]``."""
    spp = spp_ok(spp)
    if _int_ok(steps):
        sizes = [steps]
    else:
        try:
            sizes = list(steps)
        except TypeError:
            raise ValueError(f"badarg: steps must be a positive integer or a sequence of them, got {steps!r}") from None
    if not sizes or not all(_int_ok(s) and s >= 1 for s in sizes):
        raise ValueError(f"badarg: steps must be a positive integer or a sequence of them, got {steps!r}")
    ends, done, i = [], 0, 0
    while done < spp:
        done = min(spp, done + int(sizes[min(i, len(sizes) - 1)]))
        ends.append(done)
        i += 1
    return ends


class ProgressiveFrame:
    """One supersampled frame (or pixel window, or shard of either) refined a few samples at a time.

    ``add(n)`` launches the next ``n`` samples (``rt_launch_samples``) on the current torch stream
    and ``resolve()`` turns the sum so far into a preview (``rt_resolve``) on it; neither waits
    for the device.  ``sum`` is the binary64 slab, ``rt_shard_rows(win_h, row_block, nshards)`` rows of
    ``win_w * 3``, of which the first ``valid_rows`` lie inside the image; a preview has those rows.
    Once ``samples_done == spp`` the "f64" / "f32" preview is the slab ``rt_launch_window`` writes
    for the same arguments, in every byte.  ``levels`` (if requested) holds sample 0's level counts
    after the first ``add``."""

    def __init__(self, scene, width: int, height: int, depth: int, *, spp: int, seed: int = 0, device: int = 0,
                 window=None, levels: bool = False, row_block: int = 16, shard: int = 0, nshards: int = 1):
        from .raytracer import _depth_ok, _sizes_ok, _window_ok
        if not _sizes_ok(width, height):
            raise ValueError("function_clause: Width > 0, Height > 0 required")
        _depth_ok(depth)
        self.spp = spp_ok(spp)
        self.seed = seed_ok(seed)
        if not (_int_ok(row_block) and _int_ok(shard) and _int_ok(nshards)) or row_block < 1 or \
                not 0 <= shard < nshards <= N.RT_MAX_SHARDS:
            raise ValueError(f"badarg: row_block {row_block!r}, shard {shard!r} of {nshards!r}")
        self.win = _window_ok(window, width, height)
        self.w, self.h, self.depth = width, height, depth
        self.rb, self.shard, self.nshards = int(row_block), int(shard), int(nshards)
        el = N.marshal(scene)
        import torch
        self.torch = torch
        self.L = N.lib()
        self.device = torch.device("cuda", device)
        ww, wh = self.win[2:]
        self.rows = shard_rows(wh, self.rb, self.nshards)
        self.valid_rows = int((shard_global_rows(wh, self.rb, self.nshards, self.shard) >= 0).sum())
        self._p = ctypes.c_void_p()
        N.check(self.L.rt_prepare(el, len(el), device, ctypes.byref(self._p)), "rt_prepare")
        self.sum = torch.empty((self.rows, ww, 3), dtype=torch.float64, device=self.device)
        self.levels = torch.empty((self.rows, ww), dtype=torch.uint8, device=self.device) if levels else None
        self._clamped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.samples_done = 0

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def add(self, n: int = 1) -> int:
        """Launch the next ``n`` samples (fewer if fewer are left; none once the frame is complete)
        and return ``samples_done``."""
        if not _int_ok(n) or n < 1:
            raise ValueError(f"badarg: add(n) takes a positive integer, got {n!r}")
        end = min(self.spp, self.samples_done + int(n))
        if end > self.samples_done:
            lv = self.levels.data_ptr() if self.levels is not None else None
            N.check(self.L.rt_launch_samples(self._p, self.w, self.h, self.depth, *self.win, self.rb, self.shard,
                                             self.nshards, self.spp, self.seed, self.samples_done, end,
                                             self.sum.data_ptr(), lv, self._stream()), "rt_launch_samples")
            self.samples_done = end
        return self.samples_done

    def resolve(self, precision: str = "f64", max_value: int = 255):
        """The preview of ``samples_done`` samples as a device tensor ``(valid_rows, win_w, 3)`` of
        float64, float32, uint8 or uint16: sum / samples_done, for "u8" / "u16" quantised as
        ``min(trunc(C*max_value), max_value)`` (a negative or NaN channel is stored as 0 and counted:
        :meth:`clamped`)."""
        fmt, mv = format_ok(precision, max_value)
        if self.samples_done == 0:
            raise ValueError("resolve() before the first add(): there is no sample to show")
        torch = self.torch
        dt = {"f64": torch.float64, "f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}[precision]
        out = torch.empty((self.valid_rows, self.win[2], 3), dtype=dt, device=self.device)
        self._clamped.zero_()
        N.check(self.L.rt_resolve(self.sum.data_ptr(), out.numel(), self.samples_done, fmt, mv, out.data_ptr(),
                                  self._clamped.data_ptr(), self._stream()), "rt_resolve")
        return out

    def clamped(self) -> int:
        """The values the last integer :meth:`resolve` stored as 0 because they were negative or NaN
        (waits for the device); 0 after a float preview."""
        self.torch.cuda.synchronize(self.device)
        return int(self._clamped.item())

    def restart(self, scene=None):
        """Begin the frame again: the next :meth:`add` starts at sample 0, which stores into the sum.
        With ``scene``, the context's scene is replaced first (``rt_update_scene``; waits for the
        launches in flight)."""
        if scene is not None:
            el = N.marshal(scene)
            self.torch.cuda.synchronize(self.device)
            N.check(self.L.rt_update_scene(self._p, el, len(el)), "rt_update_scene")
        self.samples_done = 0

    def close(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            self.torch.cuda.synchronize(self.device)
            self.L.rt_release(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
