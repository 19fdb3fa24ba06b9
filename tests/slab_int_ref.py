"""Test-side restatement of the compact slab format for integer slabs (include/rt_mi355x.h,
"compact slab transfer"; RT_OUT_U8 / RT_OUT_U16), on byte buffers.  The header is that of
tests/slab_ref.py (the same `layout`); values are the non-zero pixels' three samples in slab order,
``3 * sample_bytes`` bytes per pixel, and a pixel is non-zero iff any of its samples is — which is
iff any of its bytes is, so the restatement never needs the samples' type.  Torch CPU ops on
uint8 views, used as the checker of the HIP codec and as a stand-in codec for the gloo tests of
eraytracer_amd.dist.CompactGather with ``dtype=torch.uint8``.  Not part of the product.
"""
import numpy as np
import torch

from eraytracer_amd.dist import shard_global_rows, shard_rows
from tests.slab_ref import layout


def as_bytes(t):
    """A contiguous tensor of any dtype as its flat bytes (a view)."""
    return t.reshape(-1).view(torch.uint8)


class IntRefCodec:
    def __init__(self, width, height, row_block, world, sample_bytes):
        assert sample_bytes in (1, 2)
        self.w, self.h, self.rb, self.world = width, height, row_block, world
        self.pb = 3 * sample_bytes  # bytes per pixel
        self.px, self.nblk, self.mask_at, self.header_bytes = layout(width, height, row_block, world)
        self.rows = shard_rows(height, row_block, world)

    def nonzero_mask(self, slab, shard):
        valid = torch.from_numpy(shard_global_rows(self.h, self.rb, self.world, shard) >= 0)
        nz = (as_bytes(slab).reshape(self.rows, self.w, self.pb) != 0).any(-1) & valid[:, None]
        return nz.reshape(-1)

    def pack(self, slab, shard, header, values):
        nz = self.nonzero_mask(slab, shard)
        pad = torch.zeros(self.nblk * 256, dtype=torch.bool)
        pad[: self.px] = nz
        words = pad.reshape(-1, 64).to(torch.int64) << torch.arange(64, dtype=torch.int64)
        mask = words.sum(1)  # wraps into the sign bit for bit 63, as u64 bits
        per_blk = pad.reshape(-1, 256).sum(1).to(torch.int64)
        off = torch.cumsum(per_blk, 0) - per_blk
        header.zero_()
        header[:8] = torch.tensor([int(nz.sum())], dtype=torch.int64).view(torch.uint8)
        header[64: 64 + 4 * self.nblk] = off.to(torch.int32).view(torch.uint8)
        header[self.mask_at:] = mask.view(torch.uint8)
        sel = as_bytes(slab).reshape(self.px, self.pb)[nz]
        as_bytes(values)[: sel.numel()] = sel.reshape(-1)

    def unpack(self, headers, values, frame):
        out = as_bytes(frame).reshape(self.h, self.w, self.pb)
        out.zero_()
        for s in range(self.world):
            hdr = headers[s]
            words = hdr[self.mask_at:].view(torch.int64)
            bits = ((words[:, None] >> torch.arange(64, dtype=torch.int64)) & 1).reshape(-1)[: self.px].bool()
            n = int(hdr[:8].view(torch.int64)[0])
            assert int(bits.sum()) == n
            slab = torch.zeros((self.px, self.pb), dtype=torch.uint8)
            slab[bits] = as_bytes(values[s])[: self.pb * n].reshape(n, self.pb)
            g = shard_global_rows(self.h, self.rb, self.world, s)
            keep = np.nonzero(g >= 0)[0]
            out[torch.from_numpy(g[keep])] = slab.reshape(self.rows, self.w, self.pb)[torch.from_numpy(keep)]
