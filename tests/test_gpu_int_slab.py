"""Integer frames through the multi-GPU gather, on the GPU: the HIP slab codec on RT_OUT_U8 /
RT_OUT_U16 slabs against the test-side restatement (tests/slab_int_ref.py), rt_unshard of integer
slabs, and dist.FrameRenderer / dist.CompactGather with precision "u8" / "u16" against rt_render's
integer frames.  Device buffers are byte tensors throughout: the codec takes pointers."""
import ctypes
import functools

import numpy as np
import pytest

from eraytracer_amd import _native as N
from eraytracer_amd import records, scenes
from eraytracer_amd.raytracer import render
from tests.test_gpu_int_frames import huge_scene, ref_quant

pytestmark = pytest.mark.gpu
SB = {"u8": 1, "u16": 2}
NP_DT = {"u8": np.uint8, "u16": np.uint16}
TOP = {"u8": 255, "u16": 65535}
PREC = {"u8": N.RT_OUT_U8, "u16": N.RT_OUT_U16}


def dev_bytes(a):
    """A numpy array's bytes as a flat uint8 device tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def host_samples(t, prec, shape):
    """A device tensor's bytes as a numpy array of the format's samples."""
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().view(NP_DT[prec]).reshape(shape)


def random_frame(w, h, prec, seed):
    """About 70 % zero pixels; of the rest, some with a single non-zero channel; the format's largest
    sample; 16-bit samples with one zero byte (0x0100, 0x0001)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, TOP[prec] + 1, size=(h, w, 3), dtype=np.int64)
    f[rng.random((h, w)) < 0.7] = 0
    single = rng.random((h, w)) < 0.08
    ch = rng.integers(0, 3, size=(h, w))
    for c in range(3):
        f[..., c] = np.where(single & (ch != c), 0, f[..., c])
    lo = 0x0100 if prec == "u16" else 1
    f[single & (ch == 0), 0] = lo
    f[single & (ch == 1), 1] = 0x0001
    f[single & (ch == 2), 2] = TOP[prec]
    f[0, 0] = (lo, 0, 0)
    f[h - 1, w - 1] = (0, 0, TOP[prec])
    return f.astype(NP_DT[prec])


def shard_slabs(frame, rb, ns, prec):
    """Every shard's slab of `frame` (numpy, [rows, w, 3]); padding rows hold 0xAB bytes."""
    from eraytracer_amd.dist import shard_global_rows, shard_rows
    h, w = frame.shape[:2]
    rows = shard_rows(h, rb, ns)
    out = []
    for s in range(ns):
        g = shard_global_rows(h, rb, ns, s)
        slab = np.full((rows, w, 3), 0xABAB & TOP[prec], dtype=NP_DT[prec])
        slab[g >= 0] = frame[g[g >= 0]]
        out.append(slab)
    return out


def round_trip(frame, rb, ns, prec):
    """Pack every shard of `frame` with the HIP codec and with IntRefCodec: count, offsets, mask and
    values byte for byte (header and values pre-filled with garbage).  Shard s's values start
    (s + 1) % 4 bytes (u8) or 2 ((s + 1) % 2) bytes (u16) into their allocation, as rows of rank 0's
    byte matrix do: the decode must not depend on it.  The HIP decode returns the frame exactly.
    Returns the reference headers."""
    import torch

    from eraytracer_amd.dist import SlabCodec
    from tests.slab_int_ref import IntRefCodec
    h, w = frame.shape[:2]
    sb = SB[prec]
    codec, ref = SlabCodec(w, h, rb, ns, prec), IntRefCodec(w, h, rb, ns, sb)
    assert codec.header_bytes == ref.header_bytes
    nval = ref.px * 3 * sb
    hdrs, vals, ref_hdrs = [], [], []
    for s, slab in enumerate(shard_slabs(frame, rb, ns, prec)):
        voff = (s + 1) % 4 if sb == 1 else 2 * ((s + 1) % 2)
        hd = torch.full((codec.header_bytes,), 0xCD, dtype=torch.uint8, device="cuda")
        vbuf = torch.full((nval + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        vd = vbuf[voff: voff + nval]
        assert vd.data_ptr() % 4 == voff
        codec.pack(dev_bytes(slab), s, hd, vd)
        hr = torch.empty(ref.header_bytes, dtype=torch.uint8)
        vr = torch.full((nval,), 0xEE, dtype=torch.uint8)
        ref.pack(torch.from_numpy(slab.reshape(-1).view(np.uint8).copy()), s, hr, vr)
        torch.cuda.synchronize()
        n = int(hr[:8].view(torch.int64)[0])
        hdc, vbc = hd.cpu(), vbuf.cpu()
        # count, offsets and mask agree (bytes between the offsets and the mask are padding)
        assert torch.equal(hdc[:8], hr[:8])
        assert torch.equal(hdc[64:64 + 4 * ref.nblk], hr[64:64 + 4 * ref.nblk])
        assert torch.equal(hdc[ref.mask_at:], hr[ref.mask_at:])
        assert torch.equal(vbc[voff: voff + 3 * sb * n], vr[: 3 * sb * n])
        assert bool((vbc[:voff] == 0xEE).all()) and bool((vbc[voff + 3 * sb * n:] == 0xEE).all())
        hdrs.append(hd)
        vals.append(vd)
        ref_hdrs.append(hr)
    img = torch.full((h * w * 3 * sb,), 0x33, dtype=torch.uint8, device="cuda")
    assert img.data_ptr() % 16 == 0
    codec.unpack(hdrs, vals, img)
    torch.cuda.synchronize()
    assert np.array_equal(host_samples(img, prec, (h, w, 3)), frame)
    return ref_hdrs


# (80, 70, 16, 3): the wide decode for both formats, with row padding; (72, 33, 7, 3): wide for u16
# (72 = 9 * 8), element-wise for u8; (33, 17, 4, 2): odd width, groups straddling mask words;
# (100, 9, 16, 8): shards without a single image row; (4112, 20, 16, 2): u8 with two column groups
# (4112 = 257 * 16: the second has one active thread), u16 with three (514 threads)
SHAPES = [(80, 70, 16, 3), (72, 33, 7, 3), (33, 17, 4, 2), (100, 9, 16, 8), (257, 31, 5, 4), (4112, 20, 16, 2)]


@pytest.mark.parametrize("prec", ["u8", "u16"])
@pytest.mark.parametrize("w,h,rb,ns", SHAPES)
def test_int_slab_codec_matches_reference_format(prec, w, h, rb, ns):
    round_trip(random_frame(w, h, prec, w * 1000 + h * 10 + ns), rb, ns, prec)


@pytest.mark.parametrize("content", ["zero", "full", "first_block", "last_block"])
@pytest.mark.parametrize("w,h", [(64, 64), (4112, 16)])
@pytest.mark.parametrize("prec", ["u8", "u16"])
def test_int_slab_codec_frame_content(prec, w, h, content):
    """Non-zero pixels nowhere, everywhere, or only in the first or only in the last 256-pixel block
    (one shard, rb = 16): the count and the block offsets follow."""
    import torch
    px = w * h
    nblk = -(-px // 256)
    lo, hi = {"zero": (0, 0), "full": (0, px), "first_block": (0, 256), "last_block": ((nblk - 1) * 256, px)}[content]
    rng = np.random.default_rng(w + h)
    flat = np.zeros((px, 3), dtype=NP_DT[prec])
    flat[lo:hi] = rng.integers(1, TOP[prec] + 1, size=(hi - lo, 3))
    (hr,) = round_trip(flat.reshape(h, w, 3), 16, 1, prec)
    count = int(hr[:8].view(torch.int64)[0])
    off = hr[64:64 + 4 * nblk].view(torch.int32).to(torch.int64)
    blk0 = torch.arange(nblk, dtype=torch.int64) * 256
    assert count == hi - lo
    assert torch.equal(off, blk0.clamp(lo, hi) - lo)


@pytest.mark.parametrize("w", [64, 33])
@pytest.mark.parametrize("prec", ["u8", "u16"])
def test_int_slab_unpack_into_an_unaligned_view(prec, w):
    """rt_slab_unpack into an image that starts one sample into a larger device buffer (such an image
    takes the element-wise kernel whatever its width): the aligned decode's bytes, and the guard bytes
    on both sides keep their value."""
    import torch

    from eraytracer_amd.dist import SlabCodec
    h, rb, ns, sb = 48, 16, 2, SB[prec]
    frame = random_frame(w, h, prec, 6448 + w)
    codec = SlabCodec(w, h, rb, ns, prec)
    hdrs, vals = [], []
    for s, slab in enumerate(shard_slabs(frame, rb, ns, prec)):
        hdrs.append(torch.empty(codec.header_bytes, dtype=torch.uint8, device="cuda"))
        vals.append(torch.empty(slab.size * sb, dtype=torch.uint8, device="cuda"))
        codec.pack(dev_bytes(slab), s, hdrs[-1], vals[-1])
    n, guard = h * w * 3 * sb, 0x5A
    buf = torch.full((n + 32,), guard, dtype=torch.uint8, device="cuda")
    view = buf[sb: sb + n]
    aligned = torch.full((n,), guard, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == sb and aligned.data_ptr() % 16 == 0
    codec.unpack(hdrs, vals, view)
    codec.unpack(hdrs, vals, aligned)
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.equal(out[sb: sb + n], aligned.cpu())
    assert np.array_equal(host_samples(aligned, prec, (h, w, 3)), frame)
    assert bool((out[:sb] == guard).all()) and bool((out[sb + n:] == guard).all())


# ---- rendered shards ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f64_frame(name, w, h, d):
    img = render(w, h, scenes.named(name), d)
    img.setflags(write=False)
    return img


RENDERED = [("default", 64, 40, 5, 3, 16),  # a partial bottom block
            ("s64", 96, 72, 3, 2, 8)]


@pytest.mark.parametrize("prec,maxv", [("u8", 255), ("u8", 7), ("u16", 65535)])
@pytest.mark.parametrize("name,w,h,d,ns,rb", RENDERED)
def test_quantised_shards_through_the_codec_equal_rt_render(name, w, h, d, ns, rb, prec, maxv):
    """rt_launch (binary64) per shard -> rt_quantize of the slab's rows inside the image ->
    rt_slab_pack -> rt_slab_unpack, and rt_unshard of the same integer slabs: rt_render's integer
    frame byte for byte, which is the P3 writer's rule applied to the binary64 frame."""
    import torch

    from eraytracer_amd.dist import SlabCodec, shard_global_rows
    L = N.lib()
    scene = scenes.named(name)
    want = render(w, h, scene, d, precision=prec, max_value=maxv)
    rule, bad = ref_quant(f64_frame(name, w, h, d), maxv, NP_DT[prec])
    assert bad == 0 and np.array_equal(want, rule)
    el = N.marshal(scene)
    p = ctypes.c_void_p()
    N.check(L.rt_prepare(el, len(el), 0, ctypes.byref(p)), "rt_prepare")
    try:
        st = torch.cuda.current_stream().cuda_stream
        sb = SB[prec]
        codec = SlabCodec(w, h, rb, ns, prec)
        rows = L.rt_shard_rows(h, rb, ns)
        slab_bytes = rows * w * 3 * sb
        islabs = torch.full((ns * slab_bytes,), 0xAB, dtype=torch.uint8, device="cuda")  # [ns][rows][w*3]
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        hdrs, vals = [], []
        for s in range(ns):
            fslab = torch.full((rows, w, 3), float("nan"), dtype=torch.float64, device="cuda")
            N.check(L.rt_launch(p, w, h, d, rb, s, ns, N.RT_OUT_F64, N.RT_ORDER_EXACT, fslab.data_ptr(), None, st))
            valid = int((shard_global_rows(h, rb, ns, s) >= 0).sum()) * w * 3
            islab = islabs[s * slab_bytes: (s + 1) * slab_bytes]
            N.check(L.rt_quantize(fslab.data_ptr(), N.RT_OUT_F64, valid, maxv, PREC[prec], islab.data_ptr(),
                                  cnt.data_ptr(), st), "rt_quantize")
            hdrs.append(torch.empty(codec.header_bytes, dtype=torch.uint8, device="cuda"))
            vals.append(torch.empty(slab_bytes, dtype=torch.uint8, device="cuda"))
            codec.pack(islab, s, hdrs[-1], vals[-1])
        img = torch.full((h * w * 3 * sb,), 0x33, dtype=torch.uint8, device="cuda")
        codec.unpack(hdrs, vals, img)
        img2 = torch.full((h * w * 3 * sb,), 0x33, dtype=torch.uint8, device="cuda")
        N.check(L.rt_unshard(islabs.data_ptr(), w, h, rb, ns, PREC[prec], img2.data_ptr(), st), "rt_unshard")
        torch.cuda.synchronize()
        assert int(cnt.item()) == 0  # (the NaN padding rows were not quantised)
        assert np.array_equal(host_samples(img, prec, (h, w, 3)), want)
        assert np.array_equal(host_samples(img2, prec, (h, w, 3)), want)
        nz = sum(int(hd[:8].cpu().view(torch.int64)[0]) for hd in hdrs)
        assert nz == int((want != 0).any(-1).sum())
    finally:
        L.rt_release(p)


# ---- dist.FrameRenderer with integer precision -----------------------------------------------
FR = ("s64", 96, 80, 5)


@functools.lru_cache(maxsize=None)
def int_frame(name, w, h, d, prec, maxv):
    img = render(w, h, scenes.named(name), d, precision=prec, max_value=maxv)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("inflight", [1, 4])
@pytest.mark.parametrize("prec,maxv", [("u8", 255), ("u16", 65535), ("u8", 7)])
def test_frame_renderer_integer_world_one(prec, maxv, inflight):
    import torch

    from eraytracer_amd.dist import FrameRenderer
    name, w, h, d = FR
    fr = FrameRenderer(scenes.named(name), w, h, d, precision=prec, max_value=maxv, inflight=inflight)
    try:
        assert fr.dtype == {"u8": torch.uint8, "u16": torch.uint16}[prec]
        assert all(s.dtype == fr.dtype and tuple(s.shape) == (fr.rows, w, 3) for s in fr.slabs)
        for s in fr.slabs:
            s.view(torch.uint8).fill_(0xAB)
        fr.fork()
        for _ in range(inflight + 1):
            fr.launch()
        fr.join()
        assert fr.gather() is fr.slab  # a world-1 caller consumes the integer slab
        assert fr.clamped() == 0
        for i, s in enumerate(fr.slabs):
            got = host_samples(s[:h], prec, (h, w, 3))
            assert np.array_equal(got, int_frame(name, w, h, d, prec, maxv)), f"slot {i}"
    finally:
        fr.close()


@pytest.mark.parametrize("world,assemble", [(2, False), (3, False), (3, True)])
@pytest.mark.parametrize("prec,maxv", [("u8", 255), ("u16", 65535)])
def test_frame_renderer_integer_shards_reassemble(prec, maxv, world, assemble):
    """Every rank's FrameRenderer on one device (rank 0 of an assembling world renders nothing): the
    integer slabs, packed and decoded as rank 0 would, are rt_render's integer frame."""
    import torch

    from eraytracer_amd.dist import FrameRenderer, SlabCodec
    name, w, h, d = FR
    ns = world - 1 if assemble else world
    codec = SlabCodec(w, h, 16, ns, prec)
    hdrs, vals = [], []
    for r in range(world):
        fr = FrameRenderer(scenes.named(name), w, h, d, rank=r, world=world, precision=prec, max_value=maxv,
                           inflight=2, assemble=assemble)
        try:
            assert fr.nshards == ns and fr.renders == (not assemble or r > 0)
            if r == 0:
                assert fr.frame.dtype == fr.dtype and tuple(fr.frame.shape) == (h, w, 3)
            for s in fr.slabs:
                s.view(torch.uint8).fill_(0xAB)
            fr.fork()
            fr.launch()
            fr.join()
            torch.cuda.synchronize()
            if not fr.renders:
                assert bool((fr.slabs[0].view(torch.uint8) == 0xAB).all()), "rank 0 rendered rows"
                continue
            assert fr.clamped() == 0
            hdrs.append(torch.empty(codec.header_bytes, dtype=torch.uint8, device="cuda"))
            vals.append(torch.empty(fr.slab.numel() * SB[prec], dtype=torch.uint8, device="cuda"))
            codec.pack(fr.slabs[0], fr.shard, hdrs[-1], vals[-1])
            torch.cuda.synchronize()
        finally:
            fr.close()
    img = torch.full((h * w * 3 * SB[prec],), 0x33, dtype=torch.uint8, device="cuda")
    codec.unpack(hdrs, vals, img)
    torch.cuda.synchronize()
    assert np.array_equal(host_samples(img, prec, (h, w, 3)), int_frame(name, w, h, d, prec, maxv))


def test_frame_renderer_clamped_counts_sum_over_the_shards():
    """A scene with a negative colour: every rank counts the values it stored as 0, padding rows are
    not counted, and the shards' counts sum to the whole frame's."""
    from eraytracer_amd.dist import FrameRenderer
    w, h, d = 24, 18, 3
    sc = huge_scene()
    want, wcnt = ref_quant(render(w, h, sc, d), 255, np.uint8)
    assert wcnt > 0
    for world in (1, 3):
        total = 0
        for r in range(world):
            fr = FrameRenderer(sc, w, h, d, rank=r, world=world, row_block=4, precision="u8")
            try:
                fr.slab.fill_(0xAB)
                fr.launch()
                total += fr.clamped()
                if world == 1:
                    assert np.array_equal(host_samples(fr.slab[:h], "u8", (h, w, 3)), want)
            finally:
                fr.close()
        assert total == wcnt, f"world {world}"
    fr = FrameRenderer(records.scene(), w, h, d, precision="u8")
    try:
        fr.launch()
        fr.launch()
        assert fr.clamped() == 0
    finally:
        fr.close()


def test_compact_gather_of_integer_frames_over_rccl_one_rank():
    """dist.CompactGather with byte buffers (dtype uint8, px_elems 3) and the HIP codec at
    precision "u8", end to end over a one-rank nccl group with frames in flight on their own
    streams: each of five frames equals the one-shard frame."""
    import os
    import socket

    import torch
    import torch.distributed as dist

    from eraytracer_amd.dist import CompactGather, FrameRenderer, SlabCodec
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        name, w, h, d = FR
        fr = FrameRenderer(scenes.named(name), w, h, d, precision="u8", inflight=3)
        frame = torch.full((h, w, 3), 0x33, dtype=torch.uint8, device="cuda")
        cg = CompactGather(SlabCodec(w, h, 16, 1, "u8"), 1, 0, fr.slab.numel(), torch.uint8, fr.device, frame,
                           px_elems=3)
        got = []

        def keep(f):
            torch.cuda.current_stream().wait_event(cg.frame_ready)
            got.append(f.clone())
            torch.cuda.synchronize()  # before the next decode overwrites the frame

        fr.fork()
        for _ in range(5):
            fr.launch()
            with torch.cuda.stream(fr.stream):
                out = cg.submit(fr.slab, 0)
            if out is not None:
                keep(out)
        cg.drain(on_frame=keep)
        fr.join()
        torch.cuda.synchronize()
        assert len(got) == 5
        for i, g in enumerate(got):
            assert np.array_equal(g.cpu().numpy(), int_frame(name, w, h, d, "u8", 255)), f"frame {i}"
        fr.close()
    finally:
        dist.destroy_process_group()
