"""Per-item data step on the device: datasets/mono_dataset.py:92-118 `preprocess` and the image part of
:139-211 `__getitem__`, for a whole batch of decoded frames at once.

The reference runs this in `num_workers` CPU processes per item with Pillow / torchvision; here the decoded frames are
uploaded once as uint8 HWC and everything downstream (flip, Lanczos pyramid, ColorJitter, ToTensor) happens in HBM through
libdepthcore's `dc_data_*` entry points, byte-exact with the CPU pipeline (tests/test_data_gpu.py, oracle/data_ref.py).
Random draws stay on the host (`sample_item`), in the reference's order.  There is no CPU path.
`GpuPreprocessor.__call__` takes a batch of one native size; `GpuPreprocessor.ragged` takes items of different native sizes
packed back to back (what a shuffled KITTI loader delivers, depthcore/loader.py) and makes scale 0 with two launches over
the whole batch (`dc_data_ragged_resize_axis`, tests/test_data_ragged_gpu.py); `GpuPreprocessor.cached` takes frames whose
resized pyramids already sit in cache slots (depthcore/frame_cache.py) and makes the same dict without any resize, in two
launches (`dc_data_cached_levels`, tests/test_data_cached_gpu.py); `GpuPreprocessor.sequence` takes the n + 2 frames of one
ConvGRU item (`dc_data_seq_levels`, tests/test_seq_data_gpu.py), and `GpuPreprocessor.sequence_batch` the items of a step that
trains several sequences in lockstep, stacked time-major by `seq_rows` (`dc_data_seq_batch_levels`,
tests/test_seq_batch_data_gpu.py).

Each shared piece is written once: `jitter_rows` is the rule that turns ColorJitter draws into the kernels' (steps, params)
rows and `jitter_tables` lays them out for a frame-major batch (`_levels`, `cached`; `sequence` lays out its own (window,
frame, level) rows with `jitter_rows`); `_levels` is the one level loop behind scale 0 (`__call__` and `ragged` differ only
in how they make scale 0); `_inputs` is the one builder of the output dict (`_levels`, `cached`); `ragged_resize` is the
two-pass resize of images of different sizes (`ragged` for scale 0, `FrameCache.build` for every level of a slot).
"""
import ctypes
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, stream

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
NO_OP = -1
# mirror of `dc_ragged_img` (include/depthcore.h)
RAGGED_IMG = np.dtype([("src_off", np.int64), ("dst_off", np.int64), ("Hi", np.int32), ("Wi", np.int32), ("table", np.int32),
                       ("flip", np.int32)])
# mirror of `dc_cached_img`
CACHED_IMG = np.dtype([("slot_off", np.int64), ("flip", np.int32), ("reserved", np.int32)])


def resample_table(in_size, out_size):
    """Pillow's 8-bit Lanczos coefficient table of one axis (host, exact): bounds (out, 2) int32, kk (out, ksize) int32."""
    L = _lib.lib()
    ksize = L.dc_resample_ksize(int(in_size), int(out_size))
    if ksize <= 0:
        raise _lib.DepthcoreError("bad resample sizes %r -> %r" % (in_size, out_size))
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    check(L.dc_resample_table(int(in_size), int(out_size), bounds.ctypes.data, kk.ctypes.data), "dc_resample_table")
    return bounds, kk


def slot_layout(height, width, num_scales):
    """A cache slot (dc_data_cached_levels): the byte offset of every level of the pyramid -- level s is a tightly packed
    (height >> s, width >> s, 3) uint8 image behind the levels before it -- and the size of the slot."""
    height, width, num_scales = int(height), int(width), int(num_scales)
    if not 1 <= num_scales <= _lib.MAX_SCALES or height <= 0 or width <= 0 or height % (1 << (num_scales - 1)) or width % (1 << (num_scales - 1)):
        raise _lib.DepthcoreError("%d x %d is not divisible by 2^(%d - 1), or num_scales is outside 1..%d"
                                  % (height, width, num_scales, _lib.MAX_SCALES))
    offsets, total = [], 0
    for s in range(num_scales):
        offsets.append(total)
        total += (height >> s) * (width >> s) * 3
    return offsets, total


def sample_item(is_train=True, rng=random, brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1)):
    """The random draws of one item in the reference's order (datasets/mono_dataset.py:139-140, :186-188):
    do_color_aug, do_flip, then ColorJitter.get_params (the four factors, then the order of the four transforms).
    -> (do_flip, jitter) with jitter = None or (order, factors) indexed by BRIGHTNESS..HUE."""
    do_color_aug = is_train and rng.random() > 0.5
    do_flip = is_train and rng.random() > 0.5
    jitter = None
    if do_color_aug:
        factors = [rng.uniform(*brightness), rng.uniform(*contrast), rng.uniform(*saturation), rng.uniform(*hue)]
        order = [0, 1, 2, 3]
        rng.shuffle(order)
        jitter = (tuple(order), tuple(factors))
    return bool(do_flip), jitter


WINDOW_FIRST = (1, 0, 2)      # first frame of the centre, left and right window of a sequence item, in the reference's order
WINDOW_FRAMES = (0, -1, 1)    # and the frame id each window is handed out under


def seq_rows(j, S, count=1):
    """THE row rule of lockstep sequence batches: S items of n frames are stacked time-major, frame j of item s is row
    j * S + s -- so frames j .. j + count - 1 of all S items are the contiguous rows this slice names.  Every stacked tensor
    (colours, K / inv_K, depth_gt, features, hidden states) follows it; S = 1 is the single sequence."""
    return slice(j * S, (j + count) * S)


def seq_item_rows(s, S, n):
    """The rows of item s alone, in frame order: the strided slice s, s + S, ..., s + (n - 1) * S of a time-major stack."""
    return slice(s, s + (n - 1) * S + 1, S)


def sample_sequence(is_train, rng, n, num_scales=4, brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1)):
    """The random draws of one sequence item in the reference's order (datasets/kitti_dataset_seq.py:104-131, :159-175):
    do_flip FIRST, then do_color_aug (the opposite of `sample_item`), then -- only when do_color_aug -- one fresh
    ColorJitter draw per window (centre, left, right), per frame j of the window and per level s, in that nesting: the
    four factors, then the shuffle of the order, as `sample_item` draws them.
    -> (do_flip, jitters) with jitters = None or jitters[w][j][s] = (order, factors)."""
    do_flip = is_train and rng.random() > 0.5
    do_color_aug = is_train and rng.random() > 0.5
    jitters = None
    if do_color_aug:
        jitters = []
        for _ in WINDOW_FIRST:
            window = []
            for _ in range(n):
                levels = []
                for _ in range(num_scales):
                    factors = [rng.uniform(*brightness), rng.uniform(*contrast), rng.uniform(*saturation), rng.uniform(*hue)]
                    order = [0, 1, 2, 3]
                    rng.shuffle(order)
                    levels.append((tuple(order), tuple(factors)))
                window.append(levels)
            jitters.append(window)
    return bool(do_flip), jitters


def hue_shift(hue_factor):
    """torchvision functional_pil.adjust_hue: `np.uint8(hue_factor * 255)` (truncation toward zero, wrap to 8 bits)."""
    return int(hue_factor * 255) & 0xFF


def jitter_rows(draws):
    """ColorJitter draws [(order, factors)] as the kernels read them, one row per draw (an order names all four
    transforms, as `sample_item` and `sample_sequence` draw it): -> (steps (m, 4), the ops in the order they are applied;
    params (m, 4) float32, the parameter of each step -- the factor of its op, or for HUE its `hue_shift`)."""
    steps = np.array([order for order, _ in draws], np.intp).reshape(-1, 4)
    by_op = np.array([(f[BRIGHTNESS], f[CONTRAST], f[SATURATION], hue_shift(f[HUE])) for _, f in draws], np.float32).reshape(-1, 4)
    return steps, by_op[np.arange(len(steps))[:, None], steps]


def jitter_tables(jitters, Fn, B, out=None):
    """The jitter tables of a frame-major batch (image f * B + b is frame f of item b): jitters holds one entry per item,
    None or (order, factors), and an item's draw applies to all of its Fn frames.  -> None when no item is jittered, else
    (steps (Fn * B, 4) int32, params (Fn * B, 4) float32), `NO_OP` steps and zero params for the unjittered items.
    out: (steps, params) contiguous arrays of the caller's to fill instead of new ones (views of one upload buffer)."""
    if jitters is None or all(j is None for j in jitters):
        return None
    steps, params = out if out is not None else (np.empty((Fn * B, 4), np.int32), np.empty((Fn * B, 4), np.float32))
    steps[...] = NO_OP
    params[...] = 0
    items = [b for b, j in enumerate(jitters) if j is not None]
    steps.reshape(Fn, B, 4)[:, items], params.reshape(Fn, B, 4)[:, items] = jitter_rows([jitters[b] for b in items])
    return steps, params


class GpuPreprocessor:
    """inputs-dict builder: native frames (uint8 HWC on the device) -> ("color" / "color_aug", frame, scale) float tensors."""

    def __init__(self, height, width, num_scales=4, frame_idxs=(0, -1, 1), device="cuda"):
        self.height, self.width, self.num_scales = int(height), int(width), int(num_scales)
        self.frame_idxs = tuple(frame_idxs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DepthcoreError("GpuPreprocessor needs a GPU device; there is no CPU path")
        self._tables = {}
        self._ragged = {}
        self._seq_tab = None

    def _table(self, in_size, out_size):
        key = (in_size, out_size)
        if key not in self._tables:
            bounds, kk = resample_table(in_size, out_size)
            self._tables[key] = (torch.from_numpy(bounds).to(self.device), torch.from_numpy(kk).to(self.device), kk.shape[1])
        return self._tables[key]

    def _resize(self, img, out_h, out_w, flip):
        """(n, H, W, 3) uint8 -> (n, out_h, out_w, 3): width pass (carrying the mirror), then height pass."""
        L = _lib.lib()
        n, H, W, _ = img.shape
        st = stream(img)
        fp = flip.data_ptr() if flip is not None else None
        if W != out_w:
            bounds, kk, ks = self._table(W, out_w)
            dst = torch.empty((n, H, out_w, 3), dtype=torch.uint8, device=img.device)
            check(L.dc_data_resize_axis(img.data_ptr(), dst.data_ptr(), n, H, W, out_w, 1, bounds.data_ptr(), kk.data_ptr(), ks, fp, st),
                  "dc_data_resize_axis")
            img = dst
        elif flip is not None:
            dst = torch.empty_like(img)
            check(L.dc_data_flip(img.data_ptr(), dst.data_ptr(), n, H, W, fp, st), "dc_data_flip")
            img = dst
        if H != out_h:
            bounds, kk, ks = self._table(H, out_h)
            dst = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=img.device)
            check(L.dc_data_resize_axis(img.data_ptr(), dst.data_ptr(), n, H, out_w, out_h, 0, bounds.data_ptr(), kk.data_ptr(), ks, None, st),
                  "dc_data_resize_axis")
            img = dst
        return img

    def _to_tensor(self, img):
        L = _lib.lib()
        n, H, W, _ = img.shape
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=img.device)
        check(L.dc_data_to_tensor(img.data_ptr(), out.data_ptr(), n, H * W, stream(img)), "dc_data_to_tensor")
        return out

    def __call__(self, native, flips=None, jitters=None):
        """native: (F, B, Hn, Wn, 3) uint8 device tensor, frame-major in the order of `frame_idxs` (the decoded
        ("color", f, -1) images of B items); flips: B booleans; jitters: B entries, None or (order, factors).
        One item's flip / jitter applies to all of its frames and scales (mono_dataset.py:94-97).
        -> {("color", f, s), ("color_aug", f, s)}: (B, 3, h, w) float32."""
        if native.dtype != torch.uint8 or native.dim() != 5 or native.shape[-1] != 3 or not native.is_cuda or not native.is_contiguous():
            raise _lib.DepthcoreError("native frames must be a contiguous (F, B, H, W, 3) uint8 device tensor")
        Fn, B, Hn, Wn, _ = native.shape
        if Fn != len(self.frame_idxs):
            raise _lib.DepthcoreError("%d frame slabs for frame_idxs %r" % (Fn, self.frame_idxs))
        flip = None
        if flips is not None and any(flips):
            flip = torch.tensor([1 if flips[b] else 0 for _ in range(Fn) for b in range(B)], dtype=torch.uint8).to(native.device)
        return self._levels(self._resize(native.view(Fn * B, Hn, Wn, 3), self.height, self.width, flip), Fn, B, jitters)

    # ---- ragged batches: items of different native sizes (a shuffled KITTI batch mixes five) --------------------------------
    def _ragged_tables(self, axis, in_sizes, out_size):
        """The concatenated Lanczos tables of one axis (mirror of dc_ragged_table), grown when a new native size shows up:
        -> (index of each size or -1 for out_size itself, host tab, device tab, host bounds, device bounds, device kk)."""
        store = self._ragged.setdefault((axis, out_size), {"index": {}, "tab": [], "bounds": [], "kk": [], "dev": None})
        for size in in_sizes:
            if size != out_size and size not in store["index"]:
                bounds, kk = resample_table(size, out_size)
                store["index"][size] = len(store["tab"])
                store["tab"].append((sum(b.size for b in store["bounds"]), sum(k.size for k in store["kk"]), kk.shape[1], size))
                store["bounds"].append(bounds.reshape(-1))
                store["kk"].append(kk.reshape(-1))
                store["dev"] = None
        if store["dev"] is None and store["tab"]:
            tab = np.array(store["tab"], np.int32)
            bounds, kk = np.concatenate(store["bounds"]), np.concatenate(store["kk"])
            store["dev"] = (tab, torch.from_numpy(tab).to(self.device), bounds, torch.from_numpy(bounds).to(self.device),
                            torch.from_numpy(kk).to(self.device))
        return [store["index"].get(size, -1) for size in in_sizes], store["dev"]

    def _ragged_pass(self, src, dst, desc, out_size, axis, tables):
        L = _lib.lib()
        desc_dev = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        tab = tab_dev = bounds = bounds_dev = kk_dev = None
        if tables is not None:
            tab, tab_dev, bounds, bounds_dev, kk_dev = tables
        check(L.dc_data_ragged_resize_axis(
            src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), desc.ctypes.data, desc_dev.data_ptr(), len(desc), out_size, axis,
            tab.ctypes.data if tab is not None else None, tab_dev.data_ptr() if tab is not None else None,
            len(tab) if tab is not None else 0, bounds.ctypes.data if tab is not None else None,
            bounds_dev.data_ptr() if tab is not None else None, bounds.size if tab is not None else 0,
            kk_dev.data_ptr() if tab is not None else None, kk_dev.numel() if tab is not None else 0, stream(src)),
            "dc_data_ragged_resize_axis")

    def ragged_resize(self, src, src_off, sizes, dst, dst_off, h, w, flips=None):
        """Images of different sizes -> (h, w, 3) each, in two launches (dc_data_ragged_resize_axis): the width pass into a
        mid buffer, carrying the mirror, then the height pass into dst.  src, dst: 1-D uint8 device tensors (they may be the
        same one: no launch reads and writes one buffer); image i is (Hn, Wn, 3) = sizes[i] at byte src_off[i] of src and
        lands at byte dst_off[i] of dst; flips: one entry per image, or None."""
        hn, wn = np.array(sizes, np.int64).reshape(-1, 2).T
        xtab, xdev = self._ragged_tables(1, wn.tolist(), w)
        ytab, ydev = self._ragged_tables(0, hn.tolist(), h)
        mid_end = np.cumsum(hn * (w * 3))
        dx, dy = np.zeros(len(hn), RAGGED_IMG), np.zeros(len(hn), RAGGED_IMG)
        dx["src_off"], dx["dst_off"], dx["Hi"], dx["Wi"], dx["table"] = src_off, mid_end - hn * (w * 3), hn, wn, xtab
        if flips is not None:
            dx["flip"] = np.asarray(flips, bool)
        dy["src_off"], dy["dst_off"], dy["Hi"], dy["Wi"], dy["table"] = dx["dst_off"], dst_off, hn, w, ytab
        mid = torch.empty(int(mid_end[-1]), dtype=torch.uint8, device=src.device)
        self._ragged_pass(src, mid, dx, w, 1, xdev)
        self._ragged_pass(mid, dst, dy, h, 0, ydev)

    def ragged(self, packed_u8, sizes, flips=None, jitters=None):
        """`__call__` for a batch whose items have DIFFERENT native sizes.  packed_u8: 1-D uint8 device tensor holding the
        decoded frames back to back, frame-major like `__call__` (image f * B + b is frame f of item b, (Hn_b, Wn_b, 3));
        sizes: B pairs (Hn, Wn) -- the frames of an item share its size (they come from one drive); flips / jitters as in
        `__call__`.  Scale 0 comes from two launches over the whole batch (dc_data_ragged_resize_axis, width then height);
        the further scales and everything behind the resize run on the uniform path.  -> the dict of `__call__`."""
        Fn, B = len(self.frame_idxs), len(sizes)
        if packed_u8.dtype != torch.uint8 or packed_u8.dim() != 1 or not packed_u8.is_cuda or not packed_u8.is_contiguous():
            raise _lib.DepthcoreError("packed frames must be a contiguous 1-D uint8 device tensor")
        if B == 0 or (flips is not None and len(flips) != B) or (jitters is not None and len(jitters) != B):
            raise _lib.DepthcoreError("sizes, flips and jitters have one entry per item")
        n, h, w = Fn * B, self.height, self.width
        sizes = np.tile(np.array(sizes, np.int64).reshape(B, 2), (Fn, 1))
        nbytes = sizes[:, 0] * sizes[:, 1] * 3
        img = torch.empty((n, h, w, 3), dtype=torch.uint8, device=packed_u8.device)
        self.ragged_resize(packed_u8, np.cumsum(nbytes) - nbytes, sizes, img.view(-1), np.arange(n) * (h * w * 3), h, w,
                           np.tile(np.asarray(flips, bool), Fn) if flips is not None else None)
        return self._levels(img, Fn, B, jitters)

    def _levels(self, img, Fn, B, jitters):
        """Scale 0 (n, height, width, 3) uint8, already flipped -> every key of `__call__` (scales 1.. resized from it)."""
        L = _lib.lib()
        n = Fn * B
        steps = params = sums = None
        tables = jitter_tables(jitters, Fn, B)
        aug = tables is not None
        if aug:
            steps, params = (torch.from_numpy(t).to(img.device) for t in tables)
            sums = torch.empty(n, dtype=torch.int64, device=img.device)
        color, color_aug = [], []
        for s in range(self.num_scales):
            h, w = self.height // (2 ** s), self.width // (2 ** s)
            if s:
                img = self._resize(img, h, w, None)
            color.append(torch.empty((n, 3, h, w), dtype=torch.float32, device=img.device))
            if aug:
                color_aug.append(torch.empty_like(color[s]))
            check(L.dc_data_jitter_to_tensor(img.data_ptr(), color[s].data_ptr(), color_aug[s].data_ptr() if aug else None, n, h * w,
                                             steps.data_ptr() if aug else None, params.data_ptr() if aug else None,
                                             sums.data_ptr() if aug else None, stream(img)), "dc_data_jitter_to_tensor")
            if s == 0:
                # the photometric kernels gather from pixel-interleaved RGBx: written here, once per item, from the same uint8
                # level (same division by 255 -> the same values as ("color", f, 0)) instead of repacked in every training step
                packed = torch.empty((n, h, w, 4), dtype=torch.float32, device=img.device)
                check(L.dc_data_to_rgbx(img.data_ptr(), packed.data_ptr(), n, h * w, stream(img)), "dc_data_to_rgbx")
        return self._inputs(color, color_aug if aug else None, packed, B)

    def _inputs(self, color, color_aug, packed, B):
        """The dict of `__call__` from frame-major tensors: color[s] (Fn * B, 3, h, w) per level, color_aug the same or None
        (no item is jittered: "color_aug" is "color"), packed (Fn * B, height, width, 4) for level 0."""
        Fn, out = len(self.frame_idxs), {}
        for s, c in enumerate(color):
            c = c.view((Fn, B) + c.shape[1:])
            a = color_aug[s].view_as(c) if color_aug is not None else c
            for i, f in enumerate(self.frame_idxs):
                out[("color", f, s)] = c[i]
                out[("color_aug", f, s)] = a[i]
            if s == 0:
                pk = packed.view((Fn, B) + packed.shape[1:])
                for i, f in enumerate(self.frame_idxs):
                    out[("color_packed", f, 0)] = pk[i]
        return out

    def cached(self, arena, slots, flips=None, jitters=None):
        """`ragged` for a batch whose frames already sit in cache slots (depthcore/frame_cache.py): arena is a 1-D uint8 device
        tensor of slots of `slot_layout(height, width, num_scales)` bytes, each the UNFLIPPED resized pyramid of one frame;
        slots: the slot index of every image, frame-major like `ragged` (image f * B + b is frame f of item b); flips /
        jitters: one entry per item.  One dc_data_cached_levels call (two launches) -> the dict of `__call__`."""
        Fn = len(self.frame_idxs)
        if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_cuda or not arena.is_contiguous():
            raise _lib.DepthcoreError("the arena must be a contiguous 1-D uint8 device tensor")
        n = len(slots)
        B = n // Fn
        if n == 0 or n != B * Fn or (flips is not None and len(flips) != B) or (jitters is not None and len(jitters) != B):
            raise _lib.DepthcoreError("one slot per frame of every item, flips and jitters one entry per item")
        L = _lib.lib()
        S, dev = self.num_scales, arena.device
        _, slot_bytes = slot_layout(self.height, self.width, S)
        aug = jitters is not None and any(j is not None for j in jitters)
        # descriptors, steps and params travel in ONE host-to-device copy: [desc n x 16 | steps n x 16 | params n x 16] bytes
        host = np.zeros(n * (48 if aug else 16), np.uint8)
        desc = host[:n * 16].view(CACHED_IMG)
        desc["slot_off"] = np.asarray(slots, np.int64) * slot_bytes
        if flips is not None:
            desc["flip"] = np.tile(np.asarray(flips, bool), Fn)
        if aug:
            jitter_tables(jitters, Fn, B, out=(host[n * 16:n * 32].view(np.int32).reshape(n, 4), host[n * 32:].view(np.float32).reshape(n, 4)))
        host_dev = torch.from_numpy(host).to(dev)
        base = host_dev.data_ptr()
        sums = torch.empty(n * S, dtype=torch.int64, device=dev) if aug else None
        color = [torch.empty((n, 3, self.height >> s, self.width >> s), dtype=torch.float32, device=dev) for s in range(S)]
        color_aug = [torch.empty_like(c) for c in color] if aug else None
        packed = torch.empty((n, self.height, self.width, 4), dtype=torch.float32, device=dev)
        ptrs = _lib.c_void_p * S
        check(L.dc_data_cached_levels(
            arena.data_ptr(), arena.numel(), desc.ctypes.data, base, n, self.height, self.width, S,
            ptrs(*[c.data_ptr() for c in color]), ptrs(*[c.data_ptr() for c in color_aug]) if aug else None, packed.data_ptr(),
            base + n * 16 if aug else None, base + n * 32 if aug else None, sums.data_ptr() if aug else None, stream(arena)),
            "dc_data_cached_levels")
        return self._inputs(color, color_aug, packed, B)

    # ---- sequence items: n + 2 consecutive frames read as three windows of n (datasets/kitti_dataset_seq.py) ---------------
    seq_lds_budget = 0      # dc_data_seq_plan's LDS budget in bytes; 0 = the library's default.  Moves the on-chip tail's start.

    def _seq_tables(self):
        """Host and device copies of the halving tables of levels 1.. (the layout dc_data_seq_levels reads), made once."""
        if self._seq_tab is None:
            parts = []
            for s in range(1, self.num_scales):
                for size in (self.width, self.height):
                    bounds, kk = resample_table(size >> (s - 1), size >> s)
                    parts += [bounds.reshape(-1), kk.reshape(-1)]
            host = np.concatenate(parts) if parts else np.zeros(0, np.int32)
            self._seq_tab = (host, torch.from_numpy(host).to(self.device) if parts else None)
        return self._seq_tab

    def sequence_plan(self, n, jitter=False):
        """dc_data_seq_plan for this preprocessor's sizes: where the on-chip tail starts, its LDS, the scratch it needs."""
        plan = _lib.SeqPlan()
        check(_lib.lib().dc_data_seq_plan(int(n), self.height, self.width, self.num_scales, 1 if jitter else 0, int(self.seq_lds_budget),
                                          plan), "dc_data_seq_plan")
        return plan

    def sequence(self, native, flip=False, jitters=None):
        """One sequence item.  native: (n + 2, Hn, Wn, 3) uint8 device tensor, consecutive frames of one drive; flip: the
        item's do_flip; jitters: None or jitters[w][j][s] = (order, factors) (`sample_sequence`).  The frames are resized
        to level 0 once (no resize when the native size is the target's, as torchvision's Resize returns the image), then
        one dc_data_seq_levels call makes every level with the reference's chain -- the mirror accumulating from level to
        level, each level resized from the jittered one before it.
        -> the ALREADY STACKED dict `Trainer._process_batch` takes: ("color", f, s) (n, 3, h, w) for f in 0, -1, 1,
        ("color_aug", f, s) the same tensor objects (the reference has no such key: both networks and the loss read
        "color"), ("color_packed", f, 0) (n, H, W, 4).  Without jitters the three windows are slices [1:n+1], [0:n], [2:n+2]
        of ONE (n + 2)-frame pyramid; with jitters every window has its own images."""
        if native.dtype != torch.uint8 or native.dim() != 4 or native.shape[-1] != 3 or not native.is_cuda or not native.is_contiguous():
            raise _lib.DepthcoreError("native frames must be a contiguous (n + 2, H, W, 3) uint8 device tensor")
        n = native.shape[0] - 2
        if n < 1:
            raise _lib.DepthcoreError("a sequence item has n + 2 >= 3 frames, got %d" % native.shape[0])
        L, S, dev, H, W = _lib.lib(), self.num_scales, native.device, self.height, self.width
        aug = jitters is not None
        n_img = 3 * n if aug else n + 2
        steps = params = None
        if aug:
            if len(jitters) != 3 or any(len(win) != n or any(len(lv) != S for lv in win) for win in jitters):
                raise _lib.DepthcoreError("jitters[w][j][s]: 3 windows of %d frames of %d levels" % (n, S))
            # [steps (3n, S, 4) int32 | params (3n, S, 4) float32]: one copy; image w * n + j, level s holds jitters[w][j][s]
            host = np.empty(n_img * S * 8, np.int32)
            host[:n_img * S * 4].reshape(-1, 4)[...], host[n_img * S * 4:].view(np.float32).reshape(-1, 4)[...] = jitter_rows(
                [draw for win in jitters for levels in win for draw in levels])
            host_dev = torch.from_numpy(host).to(dev)
            steps, params = host_dev.data_ptr(), host_dev.data_ptr() + n_img * S * 16
        level0 = self._resize(native, H, W, None)
        plan = self.sequence_plan(n, aug)
        tab_host, tab_dev = self._seq_tables()
        scratch = torch.empty(max(int(plan.scratch_bytes), 16), dtype=torch.uint8, device=dev)
        color = [torch.empty((n_img, 3, H >> s, W >> s), dtype=torch.float32, device=dev) for s in range(S)]
        packed = torch.empty((n_img, H, W, 4), dtype=torch.float32, device=dev)
        ptrs = _lib.c_void_p * S
        check(L.dc_data_seq_levels(level0.data_ptr(), n, H, W, S, 1 if flip else 0, ptrs(*[c.data_ptr() for c in color]), packed.data_ptr(),
                                   steps, params, tab_host.ctypes.data if tab_dev is not None else None,
                                   tab_dev.data_ptr() if tab_dev is not None else None, tab_host.size, scratch.data_ptr(), scratch.numel(),
                                   int(self.seq_lds_budget), stream(native)), "dc_data_seq_levels")
        out = {}
        for w, (first, f) in enumerate(zip(WINDOW_FIRST, WINDOW_FRAMES)):
            lo = w * n if aug else first
            for s in range(S):
                out[("color", f, s)] = out[("color_aug", f, s)] = color[s][lo:lo + n]
            out[("color_packed", f, 0)] = packed[lo:lo + n]
        return out

    def sequence_batch_plan(self, items, n, jitter=False):
        """dc_data_seq_batch_plan: `sequence_plan` for a step of `items` sequence items (n_img and the scratch scale with it)."""
        plan = _lib.SeqPlan()
        check(_lib.lib().dc_data_seq_batch_plan(int(items), int(n), self.height, self.width, self.num_scales, 1 if jitter else 0,
                                                int(self.seq_lds_budget), plan), "dc_data_seq_batch_plan")
        return plan

    def sequence_batch(self, packed_u8, sizes, n, flips=None, jitters=None):
        """A step of S = len(sizes) sequence items that train in lockstep.  packed_u8: 1-D uint8 device tensor, the n + 2 native
        frames of every item back to back, item-major; sizes: S pairs (Hn, Wn) -- an item's frames share its size; flips: one
        do_flip per item; jitters: one `sample_sequence` draw (or None) per item -- when any item has one the whole step takes
        the jittered layout and the items without a draw carry no-op steps, which leaves their bytes those of the plain chain.
        Level 0 comes from `_resize` when the items share a native size and from the ragged passes (`ragged_resize`) when
        they do not; then ONE dc_data_seq_batch_levels call, the launches of a single item's `sequence`.
        -> the stacked dict of `sequence` with n * S rows per key, TIME-MAJOR: frame j of item s is row j * S + s
        (`seq_rows`), and each item's rows hold the bytes `sequence` gives for that item alone.  Un-jittered the three
        windows are the slices [S:(n+1)S], [0:nS], [2S:(n+2)S] of one (n + 2) * S-row pyramid."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        S_it, n = len(sizes), int(n)
        if packed_u8.dtype != torch.uint8 or packed_u8.dim() != 1 or not packed_u8.is_cuda or not packed_u8.is_contiguous():
            raise _lib.DepthcoreError("packed frames must be a contiguous 1-D uint8 device tensor")
        flips = [False] * S_it if flips is None else [bool(f) for f in flips]
        jitters = [None] * S_it if jitters is None else list(jitters)
        if S_it < 1 or n < 1 or len(flips) != S_it or len(jitters) != S_it:
            raise _lib.DepthcoreError("sizes, flips and jitters have one entry per item, and a sequence item has n >= 1 centre frames")
        if packed_u8.numel() != sum(h * w * 3 for h, w in sizes) * (n + 2):
            raise _lib.DepthcoreError("packed frames: %d bytes are not n + 2 = %d frames of each of the sizes %r"
                                      % (packed_u8.numel(), n + 2, sizes))
        L, S, dev, H, W = _lib.lib(), self.num_scales, packed_u8.device, self.height, self.width
        aug = any(j is not None for j in jitters)
        per_item = 3 * n if aug else n + 2
        n_img = per_item * S_it
        steps = params = None
        if aug:
            if any(j is not None and (len(j) != 3 or any(len(win) != n or any(len(lv) != S for lv in win) for win in j)) for j in jitters):
                raise _lib.DepthcoreError("jitters[item][w][j][s]: 3 windows of %d frames of %d levels" % (n, S))
            # [steps (items, 3n, S, 4) int32 | params (items, 3n, S, 4) float32]: one copy; each item's rows as `sequence` lays them out
            host = np.empty(n_img * S * 8, np.int32)
            st, pa = host[:n_img * S * 4].reshape(S_it, -1, 4), host[n_img * S * 4:].view(np.float32).reshape(S_it, -1, 4)
            st[...] = NO_OP
            pa[...] = 0
            for it, j in enumerate(jitters):
                if j is not None:
                    st[it], pa[it] = jitter_rows([draw for win in j for levels in win for draw in levels])
            host_dev = torch.from_numpy(host).to(dev)
            steps, params = host_dev.data_ptr(), host_dev.data_ptr() + n_img * S * 16
        frames = S_it * (n + 2)
        if len(set(sizes)) == 1:
            level0 = self._resize(packed_u8.view((frames,) + sizes[0] + (3,)), H, W, None)
        else:
            per_frame = np.repeat(np.array(sizes, np.int64).reshape(S_it, 2), n + 2, axis=0)
            nbytes = per_frame[:, 0] * per_frame[:, 1] * 3
            level0 = torch.empty((frames, H, W, 3), dtype=torch.uint8, device=dev)
            self.ragged_resize(packed_u8, np.cumsum(nbytes) - nbytes, per_frame, level0.view(-1), np.arange(frames) * (H * W * 3), H, W)
        plan = self.sequence_batch_plan(S_it, n, aug)
        tab_host, tab_dev = self._seq_tables()
        scratch = torch.empty(max(int(plan.scratch_bytes), 16), dtype=torch.uint8, device=dev)
        color = [torch.empty((n_img, 3, H >> s, W >> s), dtype=torch.float32, device=dev) for s in range(S)]
        packed = torch.empty((n_img, H, W, 4), dtype=torch.float32, device=dev)
        ptrs = _lib.c_void_p * S
        check(L.dc_data_seq_batch_levels(level0.data_ptr(), S_it, n, H, W, S, (ctypes.c_int * S_it)(*[int(f) for f in flips]),
                                         ptrs(*[c.data_ptr() for c in color]), packed.data_ptr(), steps, params,
                                         tab_host.ctypes.data if tab_dev is not None else None,
                                         tab_dev.data_ptr() if tab_dev is not None else None, tab_host.size, scratch.data_ptr(),
                                         scratch.numel(), int(self.seq_lds_budget), stream(packed_u8)), "dc_data_seq_batch_levels")
        out = {}
        for w, (first, f) in enumerate(zip(WINDOW_FIRST, WINDOW_FRAMES)):
            rows = seq_rows(w * n if aug else first, S_it, n)
            for s in range(S):
                out[("color", f, s)] = out[("color_aug", f, s)] = color[s][rows]
            out[("color_packed", f, 0)] = packed[rows]
        return out

    def intrinsics(self, K, batch):
        """("K", s), ("inv_K", s) for a normalised 4x4 intrinsics matrix (mono_dataset.py:170-180), repeated over the batch."""
        out = {}
        for s in range(self.num_scales):
            Ks = np.array(K, dtype=np.float32).copy()
            Ks[0, :] *= self.width // (2 ** s)
            Ks[1, :] *= self.height // (2 ** s)
            inv = np.linalg.pinv(Ks)
            out[("K", s)] = torch.from_numpy(Ks).to(self.device).unsqueeze(0).repeat(batch, 1, 1).contiguous()
            out[("inv_K", s)] = torch.from_numpy(inv).to(self.device).unsqueeze(0).repeat(batch, 1, 1).contiguous()
        return out
