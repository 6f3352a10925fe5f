"""Resized frames kept on the device between epochs.

Every training frame is read three times per epoch (as frame 0, -1 and +1 of neighbouring items) and again in every epoch;
decoding it is the loader's whole host cost.  `FrameCache` keeps, per image FILE, the unflipped Lanczos pyramid at the
network's size in one uint8 arena in HBM (`depthcore.data.slot_layout`: 489 600 bytes at 192 x 640 x 4 scales), and a warm
batch is served from the slots by one `dc_data_cached_levels` call (GpuPreprocessor.cached): no file, no decode, no upload.

Why the UNFLIPPED pyramid is enough: mirroring commutes with Pillow's 8-bit Lanczos resize byte for byte when the integer
coefficient table is mirror-symmetric -- output pixel out-1-o reads the mirrored span of pixel o (`x0' = in - x0 - n`) with
the taps reversed -- so `resize(flip(x)) == flip(resize(x))` at every level, and the mirror is applied when a slot is read.
`tables_mirror_symmetric` checks exactly that on the table the kernels use; a native width whose table fails it is not cached
(`FrameCache.symmetric`), a halving inside the pyramid that fails it refuses the cache.  Heights need nothing: there is no
vertical flip.

Policy: fill until full, never evict.  Access is a uniform shuffle, so every eviction policy has the hit ratio
capacity / frames, and write-once slots need no ordering beyond the loader's one stream.  When the arena is full the frames
a batch lacks are built in `overflow` slots at the arena's tail, which the next batch overwrites.

Two halves, like the loader: the index (`lookup` / `insert` / `stats`) is host logic and runs without a GPU; `build`
fills slots with the existing ragged resize kernels.
"""
import numpy as np
import torch

from . import _lib
from .data import resample_table, slot_layout


def tables_symmetric(bounds, kk, in_size):
    """True when the coefficient table (bounds (out, 2) [first source index, tap count], kk (out, ksize)) of an axis of
    `in_size` pixels is its own mirror image: pixel out-1-o covers [in - x0 - n, in - x0) with the taps of pixel o reversed."""
    bounds, kk = np.asarray(bounds), np.asarray(kk)
    out = len(bounds)
    for o in range(out):
        x0, n = int(bounds[o, 0]), int(bounds[o, 1])
        m0, mn = int(bounds[out - 1 - o, 0]), int(bounds[out - 1 - o, 1])
        if mn != n or m0 != in_size - x0 - n or not np.array_equal(kk[out - 1 - o, :n], kk[o, :n][::-1]):
            return False
    return True


def tables_mirror_symmetric(in_size, out_size):
    """`tables_symmetric` of the table the resize kernels use for in_size -> out_size (equal sizes: no pass, trivially true)."""
    if int(in_size) == int(out_size):
        return True
    bounds, kk = resample_table(in_size, out_size)
    return tables_symmetric(bounds, kk, int(in_size))


class FrameCache:
    """path -> slot of the device arena.  budget_bytes: the whole arena, `overflow` scratch slots at its tail included."""

    def __init__(self, height, width, num_scales, budget_bytes, overflow, device=None):
        self.height, self.width, self.num_scales = int(height), int(width), int(num_scales)
        self.level_offsets, self.slot_bytes = slot_layout(height, width, num_scales)
        self.overflow = int(overflow)
        self.capacity = int(budget_bytes) // self.slot_bytes - self.overflow
        if self.overflow < 0 or self.capacity < 1:
            raise ValueError("a frame cache of %d bytes holds %d slots of %d bytes: it needs one slot and the %d overflow slots of a "
                             "batch at least (%d bytes)" % (budget_bytes, int(budget_bytes) // self.slot_bytes, self.slot_bytes,
                                                            self.overflow, (self.overflow + 1) * self.slot_bytes))
        for s in range(self.num_scales - 1):
            if not tables_mirror_symmetric(self.width >> s, self.width >> (s + 1)):
                raise ValueError("the Lanczos table %d -> %d is not mirror-symmetric: a flipped item cannot be served from an "
                                 "unflipped pyramid at this width" % (self.width >> s, self.width >> (s + 1)))
        self.device = torch.device(device) if device is not None else None
        self._arena = None
        self._symmetric = {}
        self.slots = {}
        self.stats = dict.fromkeys(("hits", "misses", "decoded", "inserted", "bypassed"), 0)

    # ------------------------------------------------------------------------------------------------------------ host index
    def __len__(self):
        return len(self.slots)

    def lookup(self, path):
        """The slot of a path, or None."""
        return self.slots.get(path)

    def insert(self, path):
        """The slot a path has or is given now; None when the cache is full (the path is not remembered)."""
        slot = self.slots.get(path)
        if slot is None and len(self.slots) < self.capacity:
            slot = self.slots[path] = len(self.slots)
            self.stats["inserted"] += 1
        return slot

    def overflow_slot(self, k):
        """Scratch slot k of the batch that is being built."""
        if not 0 <= k < self.overflow:
            raise IndexError("overflow slot %d of %d" % (k, self.overflow))
        return self.capacity + k

    def symmetric(self, native_width):
        """The gate of a native width -> `width`, evaluated once per width."""
        if native_width not in self._symmetric:
            self._symmetric[native_width] = tables_mirror_symmetric(native_width, self.width)
        return self._symmetric[native_width]

    def clear(self):
        """Forget every path and zero the stats; the arena stays (its slots are overwritten as they are given out again)."""
        self.slots.clear()
        for k in self.stats:
            self.stats[k] = 0

    # ---------------------------------------------------------------------------------------------------------- device arena
    @property
    def arena(self):
        if self._arena is None:
            if self.device is None or self.device.type != "cuda":
                raise _lib.DepthcoreError("the frame cache's arena lives on a GPU device")
            self._arena = torch.empty((self.capacity + self.overflow) * self.slot_bytes, dtype=torch.uint8, device=self.device)
        return self._arena

    def build(self, pre, packed_u8, frames):
        """Fill slots from decoded native frames with the existing kernels, flip 0.  packed_u8: 1-D uint8 device tensor;
        frames: [(byte offset in packed_u8, Hn, Wn, slot)].  Scale 0 goes straight into the slot with the two passes of
        `pre.ragged_resize` (width, then height); each further level takes two more, level s-1 in the arena -> a mid
        buffer -> level s in the arena: source and destination are never the same buffer within one launch."""
        if not frames:
            return
        arena = self.arena
        base = np.array([slot for _, _, _, slot in frames], np.int64) * self.slot_bytes
        src, src_off, sizes = packed_u8, [off for off, _, _, _ in frames], [(hn, wn) for _, hn, wn, _ in frames]
        for s in range(self.num_scales):
            h, w = self.height >> s, self.width >> s
            pre.ragged_resize(src, src_off, sizes, arena, base + self.level_offsets[s], h, w)
            src, src_off, sizes = arena, base + self.level_offsets[s], [(h, w)] * len(frames)
