"""Integer frames through the multi-GPU gather, the parts that need no GPU: the test-side
restatement of the integer slab format (tests/slab_int_ref.py), dist.CompactGather moving integer
values as bytes over gloo (px_elems), the bench self-check on integer frames, and the argument
checks the codec and FrameRenderer make before any device call."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from eraytracer_amd import _native as N
from eraytracer_amd import scenes
from eraytracer_amd.dist import shard_global_rows, shard_rows
from tests.slab_int_ref import IntRefCodec
from tests.slab_ref import layout

W, H, RB = 40, 37, 4
NP_DT = {1: np.uint8, 2: np.uint16}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def expected_frame(frame_no, sb):
    """Frame `frame_no` as a numpy (H, W, 3) array of 1- or 2-byte samples: pixel (x, r) is
    non-zero when (x + r + frame_no) % 3 == 0; such a pixel may have a single non-zero channel, and
    16-bit samples include 0x0100 and 0x0001 (one zero byte each)."""
    r, x = np.arange(H)[:, None], np.arange(W)[None, :]
    keep = (x + r + frame_no) % 3 == 0
    top = 255 if sb == 1 else 65535
    c0 = (frame_no * 37 + r * 5 + x) % (top + 1)
    c1 = np.where((x + r) % 2 == 0, 0, top - c0)
    c2 = np.where(x % 5 == 0, 0x0100 if sb == 2 else 1, 0) + np.where(x % 7 == 0, 1, 0)
    f = np.stack(np.broadcast_arrays(c0, c1, c2), -1) * keep[..., None]
    f[0, 0] = (0, 0, 1 if sb == 1 else 0x0100)  # kept whatever frame_no: a single non-zero byte
    return f.astype(NP_DT[sb])


def sparse_slab(frame_no, shard, ns, sb):
    """`shard`'s slab of that frame (uint8 bytes, [rows, W, 3 sb]); padding rows past the image hold
    0xAB (never read)."""
    rows = shard_rows(H, RB, ns)
    g = shard_global_rows(H, RB, ns, shard)
    slab = np.full((rows, W, 3), 0xABAB & (0xFF if sb == 1 else 0xFFFF), dtype=NP_DT[sb])
    slab[g >= 0] = expected_frame(frame_no, sb)[g[g >= 0]]
    return torch.from_numpy(slab.view(np.uint8).reshape(rows, W, 3 * sb).copy())


@pytest.mark.parametrize("sb", [1, 2])
def test_int_ref_codec_round_trip_and_layout(sb):
    for world in (1, 2, 3):
        codec = IntRefCodec(W, H, RB, world, sb)
        px, nblk, mask_at, hb = layout(W, H, RB, world)
        assert (codec.px, codec.header_bytes) == (px, hb) == (shard_rows(H, RB, world) * W, mask_at + 32 * nblk)
        want = expected_frame(2, sb)
        hdrs, vals, total = [], [], 0
        for s in range(world):
            slab = sparse_slab(2, s, world, sb)
            h = torch.full((hb,), 0x5A, dtype=torch.uint8)
            v = torch.full((px * 3 * sb,), 0xEE, dtype=torch.uint8)
            codec.pack(slab, s, h, v)
            g = shard_global_rows(H, RB, world, s)
            mine = want[g[g >= 0]].reshape(-1, 3)
            nz = (mine != 0).any(-1)
            n = int(h[:8].view(torch.int64)[0])
            assert n == int(nz.sum())
            # the values: the non-zero pixels' samples in slab order, native endian; nothing after them
            assert np.array_equal(v.numpy()[: n * 3 * sb], mine[nz].reshape(-1).view(np.uint8))
            assert bool((v[n * 3 * sb:] == 0xEE).all())
            # offsets: non-zero pixels before each 256-pixel block; mask: one bit per slab pixel
            flat = np.zeros(nblk * 256, dtype=bool)
            flat[: len(nz)] = nz  # (the slab's image rows are a prefix)
            off = h[64: 64 + 4 * nblk].view(torch.int32).numpy()
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(flat.reshape(-1, 256).sum(1))[:-1]]))
            assert np.array_equal(np.unpackbits(h[mask_at:].numpy(), bitorder="little"), flat.astype(np.uint8))
            hdrs.append(h)
            vals.append(v)
            total += n
        assert total == int((want != 0).any(-1).sum())
        frame = torch.full((H, W, 3 * sb), 0x77, dtype=torch.uint8)
        codec.unpack(hdrs, vals, frame)
        assert np.array_equal(frame.numpy().reshape(-1).view(NP_DT[sb]).reshape(H, W, 3), want)


# ---- dist.CompactGather with integer values as bytes ------------------------------------------
def _compact_worker(rank, world, port, out_path, nframes, first, sb):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from eraytracer_amd.dist import CompactGather
    ns, shard = world - first, max(rank - first, 0)  # first = 1: rank 0 assembles
    rows = shard_rows(H, RB, ns)
    codec = IntRefCodec(W, H, RB, ns, sb)
    frame = torch.empty((H, W, 3 * sb), dtype=torch.uint8) if rank == 0 else None
    cg = CompactGather(codec, world, rank, rows * W * 3 * sb, torch.uint8, "cpu", frame, first=first,
                       px_elems=3 * sb)
    frames = []
    for f in range(nframes):
        slab = None if first and rank == 0 else sparse_slab(f, shard, ns, sb)
        out = cg.submit(slab, shard)
        if out is not None:
            frames.append(out.clone())
    cg.drain(on_frame=lambda fr: frames.append(fr.clone()))
    if rank == 0:
        np.save(out_path, torch.stack(frames).numpy())
    else:
        assert not frames
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("px_elems", [3, 6])
@pytest.mark.parametrize("world,first", [(2, 0), (3, 0), (3, 1), (4, 1)])
def test_gloo_compact_gather_of_integer_frames(tmp_path, world, first, px_elems):
    """CompactGather with dtype=torch.uint8 and px_elems 3 (u8) / 6 (u16 samples as bytes): exactly
    count * px_elems bytes travel per rank, and every frame arrives complete, exact and in order,
    also with an assembling rank 0."""
    out = str(tmp_path / "frames.npy")
    nframes, sb = 6, px_elems // 3
    mp.spawn(_compact_worker, args=(world, _free_port(), out, nframes, first, sb), nprocs=world, join=True)
    frames = np.load(out)
    assert frames.shape == (nframes, H, W, px_elems) and frames.dtype == np.uint8
    for f in range(nframes):
        got = frames[f].reshape(-1).view(NP_DT[sb]).reshape(H, W, 3)
        assert np.array_equal(got, expected_frame(f, sb)), f"frame {f}"


def test_compact_gather_default_px_elems_is_three():
    from eraytracer_amd.dist import CompactGather
    from tests.slab_ref import RefCodec
    cg = CompactGather(RefCodec(W, H, RB, 1), 1, 0, 10, torch.float32, "cpu", None)
    assert cg.px_elems == 3


def _verify_worker(rank, world, port, out_path, corrupt, sb):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from eraytracer_amd.dist import CompactGather, verify_compact_gather
    rows = shard_rows(H, RB, world)
    codec = IntRefCodec(W, H, RB, world, sb)
    dt = {1: torch.uint8, 2: torch.uint16}[sb]
    frame = torch.empty((H, W, 3), dtype=dt) if rank == 0 else None  # a frame of the samples' own type
    cg = CompactGather(codec, world, rank, rows * W * 3 * sb, torch.uint8, "cpu", frame, px_elems=3 * sb)

    def make_slab(i):
        s = sparse_slab(i, rank, world, sb)
        if corrupt and rank == world - 1 and i == 1:
            s[0, 3, 3 * sb - 1] ^= 1  # one wrong sample (its most significant byte) on the last rank
        return s

    try:
        n = verify_compact_gather(cg, make_slab, lambda i: torch.from_numpy(expected_frame(i, sb)), rank, nframes=3)
        res = f"ok {n}"
    except RuntimeError as e:
        res = f"error {e}"
    if rank == 0:
        with open(out_path, "w") as f:
            f.write(res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("corrupt", [False, True])
def test_gloo_self_check_on_integer_frames(tmp_path, corrupt, sb):
    """dist.verify_compact_gather compares uint8 / uint16 frames directly: equal frames pass, one
    wrong sample on the last rank is caught and located."""
    out = str(tmp_path / "res.txt")
    mp.spawn(_verify_worker, args=(3, _free_port(), out, corrupt, sb), nprocs=3, join=True)
    res = open(out).read()
    if corrupt:
        assert res.startswith("error") and "frame 1" in res and "1 pixels" in res, res
    else:
        assert res == "ok 3", res


# ---- argument checks made before any device call ------------------------------------------------
def test_integer_codec_refusals_need_no_device(native):
    L = native.lib()
    w, h, rb, ns = 64, 32, 16, 2
    fake = 0x10000  # non-null "device" addresses: every refusal below comes before they are used
    for prec in (N.RT_OUT_U8, N.RT_OUT_U16):
        assert L.rt_slab_pack(None, w, h, rb, 0, ns, prec, fake, fake, None) == N.RT_EBADARG
        assert L.rt_slab_pack(fake, w, h, rb, 0, ns, prec, None, fake, None) == N.RT_EBADARG
        assert L.rt_slab_pack(fake, w, h, rb, 0, ns, prec, fake, None, None) == N.RT_EBADARG
        assert L.rt_slab_pack(fake, w, h, rb, ns, ns, prec, fake, fake, None) == N.RT_EBADARG  # shard >= nshards
    hp = (ctypes.c_void_p * 2)(fake, None)  # a null shard pointer
    vp = (ctypes.c_void_p * 2)(fake, fake)
    assert L.rt_slab_unpack(hp, vp, w, h, rb, 2, N.RT_OUT_U16, fake, None) == N.RT_EBADARG
    assert L.rt_slab_unpack(vp, hp, w, h, rb, 2, N.RT_OUT_U8, fake, None) == N.RT_EBADARG
    assert L.rt_slab_unpack(vp, vp, w, h, rb, 2, N.RT_OUT_U16, None, None) == N.RT_EBADARG
    # 16-bit samples: an odd slab, values or image pointer
    assert L.rt_slab_pack(fake + 1, w, h, rb, 0, ns, N.RT_OUT_U16, fake, fake, None) == N.RT_EBADARG
    assert L.rt_slab_pack(fake, w, h, rb, 0, ns, N.RT_OUT_U16, fake, fake + 1, None) == N.RT_EBADARG
    odd = (ctypes.c_void_p * 2)(fake, fake + 3)
    assert L.rt_slab_unpack(vp, odd, w, h, rb, 2, N.RT_OUT_U16, fake, None) == N.RT_EBADARG
    assert L.rt_slab_unpack(vp, vp, w, h, rb, 2, N.RT_OUT_U16, fake + 1, None) == N.RT_EBADARG
    # no such precision
    assert L.rt_slab_pack(fake, w, h, rb, 0, ns, 4, fake, fake, None) == N.RT_EBADARG
    assert L.rt_slab_unpack(vp, vp, w, h, rb, 2, 4, fake, None) == N.RT_EBADARG
    assert L.rt_unshard(fake, w, h, rb, ns, 4, fake, None) == N.RT_EBADARG
    assert L.rt_unshard(None, w, h, rb, ns, N.RT_OUT_U8, fake, None) == N.RT_EBADARG
    assert L.rt_unshard(fake, w, h, rb, ns, N.RT_OUT_U16, None, None) == N.RT_EBADARG


def test_abi_is_unchanged_by_the_integer_gather(native):
    assert native.lib().rt_abi_version() == 5
    assert {"rt_slab_pack", "rt_slab_unpack", "rt_unshard", "rt_slab_header_bytes"} <= set(N.EXPORTS)


@pytest.mark.parametrize("precision,bad", [("u8", 0), ("u8", 256), ("u16", 0), ("u16", 65536), ("u8", True),
                                           ("u8", 7.0)])
def test_frame_renderer_refuses_a_max_value_outside_the_format(precision, bad):
    """Checked before a context, a stream or a buffer is made, so it runs without a device."""
    from eraytracer_amd.dist import PRECISIONS, FrameRenderer
    assert PRECISIONS["u8"] == N.RT_OUT_U8 and PRECISIONS["u16"] == N.RT_OUT_U16
    with pytest.raises(ValueError, match="MaxValue"):
        FrameRenderer(scenes.s64(), 32, 32, 3, precision=precision, max_value=bad)
