"""Batches for the training loop (reference trainer.py:152-164: two shuffled `DataLoader`s with drop_last).

The reference's loader forks `num_workers` processes that each decode, resize, jitter and convert one item with Pillow.
Here the only host work is DECODING: the frames of a batch are decoded on a thread pool (PIL releases the GIL while it
decodes) straight into a pinned staging buffer, one host-to-device copy moves them, and the data step runs on the device
over the ragged batch (GpuPreprocessor.ragged: a shuffled KITTI batch mixes five native sizes).  No worker processes:
nothing forks after the GPU has been initialised.

Two halves:
  * host -- `plan` (which items, which random draws) and `decode_batch` (files -> one packed uint8 buffer): no GPU needed;
  * device -- upload + data step on a side stream of the loader's own, handed to the consumer's stream with an event.
    `_StagedLoader._device_half` is that half for every kind of job, and the one place that states its order: the copy
    and the event that frees the staging buffer, the data step, the intrinsics, "depth_gt", the extras, the batch's
    event.  A loader's `_upload` only says what its data step is (`ragged`; slots + `FrameCache.build` + `cached`;
    `sequence`); `_wait` joins a job's pool tasks, `_device_state` makes the preprocessor and the stream on first use.
Every GPU call is made by the consuming thread (the pool threads only decode), so a training step that is being captured
into a hipGraph never meets a launch or an allocation of another thread.

Sampling is a function of (seed, epoch) alone: one `random.Random` gives the permutation and then, in item order, the
draws of `sample_item` -- batches do not depend on thread timing.  `rank` / `world_size` take a strided shard of the same
permutation, the same number of steps on every rank.

`cache_bytes` > 0 adds a cache of resized frames in HBM (depthcore/frame_cache.py): the host then decodes only the frames
the cache lacks, and a warm batch is gathered from cache slots in two launches.  The batches are the same, bit for bit.

A dataset with `device_depth` whose velodyne scans are present (KITTIRAWDataset) gets its "depth_gt" on the device: the pool
threads read each item's scan into the staging buffer behind the frames, the one copy carries them and the projection's
descriptors, and `ops.lidar_depth_maps_staged` runs on the loader's stream -- with or without the frame cache.

`SequenceLoader` is the same machine for the ConvGRU front-end's items (datasets/kitti_dataset_seq.py): one item of n + 2
consecutive frames per step, already stacked over its n positions (GpuPreprocessor.sequence), its n scans behind the frames;
`items_per_step = S` delivers S such items per step, stacked time-major (GpuPreprocessor.sequence_batch).

`decode_packed` is the evaluation scripts' host half: the files of a split decoded on the calling thread and packed the way
`GpuPreprocessor.ragged` reads them (evaluate_depth.py, evaluate_depth_gru.py, evaluate_depth_fusion_v3.py).
"""
import collections
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import lidar
from .data import GpuPreprocessor, sample_item, sample_sequence
from .frame_cache import FrameCache

MAX_THREADS = 16      # decode threads: bounded by the option and by this, never by the machine's core count


def epoch_rng(seed, epoch):
    """The generator of one epoch's permutation and draws."""
    return random.Random("depthcore.loader/%d/%d" % (seed, epoch))


try:
    import pyarrow
except ImportError:         # optional: only the way the decoded pixels leave Pillow depends on it
    pyarrow = None


def _pixels(rgb):
    """(H, W, 3) uint8 view or copy of a loaded RGB image.  Pillow keeps RGB as four bytes per pixel; `np.asarray` repacks
    them through `tobytes`, chunk by chunk under the interpreter lock -- with a dozen decode threads that starves the thread
    launching the training step (and the step starves the decoders).  Pillow's Arrow export hands out its own memory
    instead, and the 4 -> 3 byte copy into the staging buffer is then one numpy loop that runs without the lock."""
    if pyarrow is not None and hasattr(rgb, "__arrow_c_array__"):
        try:
            flat = pyarrow.array(rgb).flatten().to_numpy(zero_copy_only=True)
            return flat.reshape(rgb.height, rgb.width, 4)[:, :, :3]
        except (ValueError, pyarrow.ArrowException):      # an image spread over several memory blocks has no zero-copy export
            pass
    return np.asarray(rgb)


def _decode_into(path, dst):
    with open(path, "rb") as f:
        with Image.open(f) as img:
            rgb = img if img.mode == "RGB" else img.convert("RGB")
            if (rgb.height, rgb.width) != dst.shape[:2]:
                raise ValueError("%s is %dx%d, its item's first frame %dx%d: the frames of an item share one size"
                                 % (path, rgb.height, rgb.width, dst.shape[0], dst.shape[1]))
            rgb.load()
            dst[...] = _pixels(rgb)


def decode_packed(paths):
    """The image files of an evaluation split decoded to RGB on the calling thread and packed back to back, in the order
    given -> (packed 1-D uint8, sizes [(Hn, Wn)]): what `GpuPreprocessor.ragged` takes once it is on the device."""
    imgs = []
    for path in paths:
        if not os.path.exists(path):
            raise FileNotFoundError("image %s of the split does not exist" % path)
        with open(path, "rb") as f:
            imgs.append(np.asarray(Image.open(f).convert("RGB")))
    return np.concatenate([im.reshape(-1) for im in imgs]), [im.shape[:2] for im in imgs]


def _read_into(path, dst):
    """The bytes of a file (a velodyne scan) into a uint8 view of the staging buffer."""
    with open(path, "rb") as f:
        if f.readinto(dst) != dst.size or f.read(1):
            raise ValueError("%s changed size while the batch was being read" % path)


def _image_size(path):
    with open(path, "rb") as f:
        with Image.open(f) as img:          # reads the header only
            return img.height, img.width


class _StagedLoader:
    """What BatchLoader and SequenceLoader share: the decode pool, the two pinned staging buffers, the velodyne scans that
    travel behind the frames, the device half of a job (`_wait`, `_device_state`, `_device_half`) and the epoch iteration
    with its prefetch.  A subclass gives `dataset`, `__len__`, `plan` (-> [arguments of `_submit`]),
    `_submit(*plan entry, alloc=)` (-> job dict with "buf", "futures", "scans") and `_upload(job, slot)` (-> (batch dict,
    event), through `_device_half`); `cache` is None unless the subclass has a frame cache and a `_submit_cached`."""
    cache = None

    def _init_staging(self, num_workers, device, seed, shuffle, prefetch):
        self.seed, self.shuffle = int(seed), bool(shuffle)
        self.prefetch = max(0, min(int(prefetch), 2))        # two staging buffers: at most two batches ahead
        self.device = torch.device(device)
        self.epoch = 0
        self.threads = max(1, min(int(num_workers), MAX_THREADS))
        self._pool = None
        self._pre = self._intrinsics = self._side = None
        self._staging, self._copied = [None, None], [None, None]
        self._jobs = collections.deque()

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _pool_(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix="depthcore-decode")
        return self._pool

    def _scan_job(self, sources, flips, frame_bytes):
        """The velodyne half of a job: sources = [(scan path, calibration folder, camera)], one map each.  The scans go into
        the staging buffer behind the frames, back to back from the next 16-byte boundary, the descriptors of the projection
        (lidar.descriptors) behind them, and `_lidar_depth` turns them into "depth_gt" after the one upload -- no further
        copy, nothing that waits for the device."""
        nbytes = [os.path.getsize(path) for path, _, _ in sources]
        if any(n % 16 for n in nbytes):
            raise ValueError("a velodyne scan is rows of four float32: %s has %d bytes"
                             % next((s[0], n) for s, n in zip(sources, nbytes) if n % 16))
        calib = [lidar.velo_to_image(calib_dir, cam) for _, calib_dir, cam in sources]
        off = (frame_bytes + 15) // 16 * 16
        end = off + sum(nbytes)
        width, height = self.dataset.full_res_shape
        desc = lidar.descriptors([n // 16 for n in nbytes], np.stack([c[0] for c in calib]), [c[1] for c in calib],
                                 out_size=(height, width), flips=flips)
        return {"off": off, "end": end, "total": end + desc.host.size, "paths": [s[0] for s in sources], "nbytes": nbytes, "desc": desc}

    def _read_scans(self, scans, buf):
        """One pool task per scan, reading the file at its offset of the staging buffer -> the futures."""
        buf[scans["end"]:scans["total"]] = scans["desc"].host
        futures, off = [], scans["off"]
        for path, n in zip(scans["paths"], scans["nbytes"]):
            futures.append(self._pool_().submit(_read_into, path, buf[off:off + n]))
            off += n
        return futures

    def _lidar_depth(self, scans, dev):
        """"depth_gt" (B, 1, 375, 1242) of an uploaded job (dev: the device copy of its staging bytes), on the current stream."""
        from . import ops
        points = dev[scans["off"]:scans["end"]].view(torch.float32).view(-1, 4)
        return ops.lidar_depth_maps_staged(points, scans["desc"], dev[scans["end"]:scans["total"]])

    def _stage(self, slot, nbytes):
        """Pinned staging buffer `slot`, free again: the copy that last read it has completed."""
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()
            self._copied[slot] = None
        if self._staging[slot] is None or self._staging[slot].numel() < nbytes:
            self._staging[slot] = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8).pin_memory()
        return self._staging[slot].numpy()

    @staticmethod
    def _pending(job):
        """The pool tasks of a submitted job."""
        return job["futures"] + ([job["meta"]] if job.get("meta") is not None else [])

    @staticmethod
    def _wait(job):
        """Wait for the pool tasks of a job -> its extras: the results of the `meta` task (if any) stacked over the items."""
        for fut in job["futures"]:
            fut.result()
        metas = job["meta"].result() if job.get("meta") is not None else []
        return {k: np.stack([m[k] for m in metas]) for k in (metas[0] if metas else {})}

    def _device_state(self, batch):
        """The preprocessor, the intrinsics repeated over `batch` and the loader's own stream, made on first use."""
        if self._pre is None:
            ds = self.dataset
            self._pre = GpuPreprocessor(ds.height, ds.width, ds.num_scales, ds.frame_idxs, self.device)
            self._intrinsics = self._pre.intrinsics(ds.K, batch)
            self._side = torch.cuda.Stream(self.device)

    def _device_half(self, job, slot, extras, data_step, copy=True):
        """The device half of a job whose pool tasks are done, all of it in order on the loader's stream -> (batch dict,
        event that completes it).  copy: the job's bytes go up from staging buffer `slot` in one copy, and the event that
        frees the buffer (`_stage`) is recorded right behind it; `data_step(device bytes, or None without a copy)` -> the
        batch; then the intrinsics, "depth_gt" from the job's scans, the extras, and -- last -- the batch's event.  That
        order is what keeps a batch valid while it is held and a cache slot written before any batch reads it."""
        with torch.cuda.stream(self._side):
            dev = None
            if copy:
                nbytes = job["buf"].size
                dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                dev.copy_(self._staging[slot][:nbytes], non_blocking=True)
                self._copied[slot] = torch.cuda.Event()
                self._copied[slot].record(self._side)
            batch = data_step(dev)
            batch.update(self._intrinsics)
            if job["scans"]:
                batch["depth_gt"] = self._lidar_depth(job["scans"], dev)
            for k, v in extras.items():
                batch[k] = torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
            ready = torch.cuda.Event()
            ready.record(self._side)
        return batch, ready

    def __iter__(self):
        """One epoch (`set_epoch`) of batches: dicts of device tensors only, the same keys and shapes every step."""
        for job in self._jobs:                      # an abandoned iteration: let its decodes finish before the buffers go on
            if "futures" in job:
                for fut in self._pending(job):
                    fut.result()
        self._jobs.clear()
        batches = self.plan()
        nxt = 0
        submit = self._submit if self.cache is None else self._submit_cached

        def submit_until(last):
            # batch j decodes into staging buffer j % 2: `_stage` waits for the copy of batch j - 2, which has been issued by
            # then (batch j - 2 is the one being handed out, or an earlier one)
            nonlocal nxt
            while nxt < len(batches) and nxt <= last:
                slot = nxt % 2
                job = submit(*batches[nxt], alloc=lambda nbytes, slot=slot: self._stage(slot, nbytes))
                job["slot"] = slot
                self._jobs.append(job)
                nxt += 1

        for step in range(len(batches)):
            submit_until(step)
            cur = self._jobs.popleft()
            if "futures" in cur:
                cur = dict(zip(("batch", "ready"), self._upload(cur, cur["slot"])))
            submit_until(step + self.prefetch)
            # the next batch's copy and data step go out now if its frames are already decoded: they run under this step
            if self._jobs and "futures" in self._jobs[0] and all(f.done() for f in self._pending(self._jobs[0])):
                job = self._jobs[0]
                self._jobs[0] = dict(zip(("batch", "ready"), self._upload(job, job["slot"])))
            consumer = torch.cuda.current_stream(self.device)
            consumer.wait_event(cur["ready"])
            for t in cur["batch"].values():
                t.record_stream(consumer)
            yield cur["batch"]

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None


class BatchLoader(_StagedLoader):
    def __init__(self, dataset, batch_size, num_workers=12, device="cuda", seed=0, shuffle=True, rank=0, world_size=1, prefetch=2,
                 cache_bytes=0):
        """cache_bytes > 0: keep resized frames on the device (depthcore/frame_cache.py) in an arena of that many bytes --
        a frame is decoded the first time a batch needs it and served from its slot afterwards.  0: no cache."""
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.cache = None
        if cache_bytes:
            self.cache = FrameCache(dataset.height, dataset.width, dataset.num_scales, cache_bytes,
                                    len(dataset.frame_idxs) * self.batch_size, device)
        self.is_train = bool(dataset.is_train)
        self.rank, self.world_size = int(rank), int(world_size)
        self._init_staging(num_workers, device, seed, shuffle, prefetch)

    # ------------------------------------------------------------------------------------------------------------ host half
    def __len__(self):
        """Steps per epoch: the same on every rank (drop_last over the rank's shard)."""
        return len(self.dataset) // self.world_size // self.batch_size

    def plan(self, epoch=None):
        """The epoch's batches: [(indices, draws)], draws = one `sample_item` result per item, in item order."""
        rng = epoch_rng(self.seed, self.epoch if epoch is None else epoch)
        order = list(range(len(self.dataset)))
        if self.shuffle:
            rng.shuffle(order)
        order = order[self.rank::self.world_size][:len(self) * self.batch_size]
        batches = []
        for i in range(len(self)):
            indices = order[i * self.batch_size:(i + 1) * self.batch_size]
            batches.append((indices, [sample_item(self.is_train, rng) for _ in indices]))
        return batches

    def _scans(self, indices, flips, frame_bytes):
        """The velodyne half of a job for a dataset that projects "depth_gt" on the device (`device_depth` with scans present),
        else None (`_scan_job`: one scan per item)."""
        ds = self.dataset
        if not (getattr(ds, "device_depth", False) and getattr(ds, "load_depth", False)):
            return None
        return self._scan_job([ds.depth_source(i) for i in indices], flips, frame_bytes)

    def _submit(self, indices, draws, alloc, device_depth=True):
        """Start decoding a batch: sizes from the headers of each item's first frame, then one task per frame writing at
        its offset of `alloc(total bytes)` (frame-major: image f * B + b).  -> job dict with the futures.  device_depth:
        the scans of a dataset with `device_depth` travel behind the frames (`_scans`) instead of a host-built "depth_gt"."""
        ds = self.dataset
        paths = [ds.frame_paths(i) for i in indices]
        sizes = [_image_size(p[0]) for p in paths]
        files = [(paths[b][f], h, w) for f in range(len(ds.frame_idxs)) for b, (h, w) in enumerate(sizes)]
        return dict(self._job(indices, draws, files, alloc, device_depth), sizes=sizes)

    def _job(self, indices, draws, files, alloc, device_depth=True):
        """What `_submit` and `_submit_cached` share: files = [(path, Hn, Wn)] are decoded back to back into
        `alloc(total bytes)` (never called when there is nothing to stage), one pool task each, the scans behind them, and
        one more task collects the items' metadata.  -> job dict."""
        ds = self.dataset
        flips = [bool(d[0]) for d in draws]
        frame_bytes = sum(h * w * 3 for _, h, w in files)
        scans = self._scans(indices, flips, frame_bytes) if device_depth else None
        total = scans["total"] if scans else frame_bytes
        buf = alloc(total)[:total] if total else None
        futures, off = [], 0
        for path, h, w in files:
            futures.append(self._pool_().submit(_decode_into, path, buf[off:off + h * w * 3].reshape(h, w, 3)))
            off += h * w * 3
        if scans:
            futures += self._read_scans(scans, buf)
        meta = self._pool_().submit(lambda: [ds.metadata(i, fl, device_depth=scans is not None) for i, fl in zip(indices, flips)])
        return {"buf": buf, "frame_bytes": frame_bytes, "flips": flips, "jitters": [d[1] for d in draws], "futures": futures,
                "meta": meta, "scans": scans}

    def _submit_cached(self, indices, draws, alloc):
        """`_submit` with the frame cache on: only the frames the cache lacks are decoded, each file once however often the
        batch names it (frame 0 stands in for a missing neighbour), back to back into `alloc(total bytes)`; a batch whose
        frames are all cached touches no image file and -- unless the dataset's scans travel with it (`_scans`: they are not
        cached) -- no staging buffer.  The size of a missing frame comes from the header of
        its item's first missing frame.  A native width whose Lanczos table is not mirror-symmetric cannot be cached
        (FrameCache.symmetric): a batch that holds such an item goes down the uncached path whole and counts as bypassed."""
        ds, cache = self.dataset, self.cache
        paths = [ds.frame_paths(i) for i in indices]
        need, hits = {}, 0
        for item in paths:
            size = None
            for path in item:
                if cache.lookup(path) is not None:
                    hits += 1
                elif path not in need:
                    size = size or _image_size(path)
                    need[path] = size
        if not all(cache.symmetric(w) for _, w in need.values()):
            cache.stats["bypassed"] += sum(len(item) for item in paths)
            return self._submit(indices, draws, alloc)
        cache.stats["hits"] += hits
        cache.stats["misses"] += sum(len(item) for item in paths) - hits
        cache.stats["decoded"] += len(need)
        frames, off = [], 0
        for path, (h, w) in need.items():
            frames.append((path, off, h, w))
            off += h * w * 3
        return dict(self._job(indices, draws, [(path, h, w) for path, _, h, w in frames], alloc), paths=paths, frames=frames)

    def decode_batch(self, indices, draws=None, out=None):
        """Host half of one batch: -> (packed uint8 buffer, sizes [(Hn, Wn)] per item, flips, jitters, extras).  The buffer
        holds the decoded frames back to back, frame-major (what GpuPreprocessor.ragged takes); extras: the stacked
        "depth_gt" (B, 1, H, W) / "stereo_T" (B, 4, 4) of datasets that have them.  draws: one (do_flip, jitter) per item
        (default: none).  out: a uint8 array to decode into (default: a new one)."""
        draws = draws if draws is not None else [(False, None)] * len(indices)

        def alloc(nbytes):
            if out is None:
                return np.empty(nbytes, np.uint8)
            if out.size < nbytes:
                raise ValueError("decode_batch: %d bytes do not fit the given buffer of %d" % (nbytes, out.size))
            return out
        job = self._submit(indices, draws, alloc, device_depth=False)
        extras = self._wait(job)
        return job["buf"], job["sizes"], job["flips"], job["jitters"], extras

    # ---------------------------------------------------------------------------------------------------------- device half
    def _upload(self, job, slot):
        """One host-to-device copy + the data step (`_device_half`) -> (batch dict, event that completes it)."""
        self._device_state(self.batch_size)
        if "paths" in job:
            return self._upload_cached(job, slot)
        return self._device_half(job, slot, self._wait(job), lambda dev: self._pre.ragged(
            dev[:job["frame_bytes"]], job["sizes"], job["flips"], job["jitters"]))

    def _upload_cached(self, job, slot):
        """`_upload` of a `_submit_cached` job: the decoded frames go up in one copy and into slots -- cache slots while
        there are free ones, else the arena's overflow slots, which only this batch reads; a frame that an earlier batch has
        inserted since this one was submitted just uses its slot -- and the batch is gathered from the slots
        (GpuPreprocessor.cached).  Slots are given out here, on the consuming thread, in batch order; everything runs in
        order on the loader's stream, so a slot is written before any batch reads it and the overflow slots are free again
        when the next batch builds."""
        extras, cache = self._wait(job), self.cache
        where, build, spilled = {}, [], 0
        for path, off, h, w in job["frames"]:
            where[path] = cache.lookup(path)
            if where[path] is None:
                where[path] = cache.insert(path)
                if where[path] is None:
                    where[path] = cache.overflow_slot(spilled)
                    spilled += 1
                build.append((off, h, w, where[path]))
        paths = job["paths"]
        slots = []
        for f in range(len(self.dataset.frame_idxs)):
            for item in paths:
                s = where.get(item[f])
                slots.append(s if s is not None else cache.lookup(item[f]))
        if any(s is None for s in slots):
            raise RuntimeError("a frame of this batch has left the cache since the batch was planned (FrameCache.clear during an epoch)")

        def data_step(dev):
            cache.build(self._pre, dev, build)
            return self._pre.cached(cache.arena, slots, job["flips"], job["jitters"])
        return self._device_half(job, slot, extras, data_step, copy=bool(build or job["scans"]))


class SequenceLoader(_StagedLoader):
    """One sequence item per step for the ConvGRU front-end (reference trainer_gru.py:206-240: DataLoader(batch_size=1) over
    KITTIDataset_v1).  dataset: datasets.KITTISequenceDataset.  `plan(epoch)` is a function of (seed, epoch) alone: the
    (shuffled) order of the items, then one `sample_sequence` per item in that order.  The n + 2 frames are decoded on the
    pool into a pinned buffer, the n centre scans -- when the dataset has them -- read behind them, one copy moves both, and
    the data step (GpuPreprocessor.sequence, then the projection through camera 2 with the mirror applied once) runs on the
    loader's own stream.  Every GPU call comes from the consuming thread.  No frame cache.
    items_per_step = S > 1 (beyond the reference): a step is S consecutive items of the same permutation with the same
    per-item draws, the last partial step dropped; their frames go up item-major in the one copy and come back stacked
    time-major (GpuPreprocessor.sequence_batch: frame j of item s is row j * S + s), "depth_gt" of the n * S centre scans in
    the same order from the one projection call."""

    def __init__(self, dataset, num_workers=12, device="cuda", seed=0, shuffle=True, prefetch=2, items_per_step=1):
        self.dataset, self.batch_size = dataset, 1
        self.items_per_step = int(items_per_step)
        if self.items_per_step < 1:
            raise ValueError("items_per_step must be >= 1, got %r" % (items_per_step,))
        self.is_train = bool(dataset.is_train)
        self._init_staging(num_workers, device, seed, shuffle, prefetch)

    def __len__(self):
        return len(self.dataset) // self.items_per_step

    def plan(self, epoch=None):
        """The epoch's items: [(index, (do_flip, jitters))]; with items_per_step = S > 1 the same list cut into runs of S:
        [((index, ...), ((do_flip, jitters), ...))]."""
        ds = self.dataset
        rng = epoch_rng(self.seed, self.epoch if epoch is None else epoch)
        order = list(range(len(ds)))
        if self.shuffle:
            rng.shuffle(order)
        items = [(i, sample_sequence(self.is_train, rng, ds.n, ds.num_scales)) for i in order]
        S = self.items_per_step
        if S == 1:
            return items
        return [tuple(zip(*items[k * S:(k + 1) * S])) for k in range(len(items) // S)]

    def _submit_step(self, indices, draws, alloc, device_depth=True):
        """`_submit` for a step of several items: every item's n + 2 frames back to back, item-major, each item at the size
        of its own first frame; the centre scans behind them time-major (scan j of item s is map j * S + s)."""
        ds = self.dataset
        paths = [ds.frame_paths(i) for i in indices]
        sizes = [_image_size(p[0]) for p in paths]
        frame_bytes = sum(len(p) * h * w * 3 for p, (h, w) in zip(paths, sizes))
        flips, jitters = [bool(d[0]) for d in draws], [d[1] for d in draws]
        scans = None
        if ds.load_depth and device_depth:
            per_item = [[(p, ds.calib_dir(i), 2) for p in ds.scan_paths(i)] for i in indices]
            scans = self._scan_job([item[j] for j in range(ds.n) for item in per_item], flips * ds.n, frame_bytes)
        total = scans["total"] if scans else frame_bytes
        buf = alloc(total)[:total]
        futures, off = [], 0
        for item, (h, w) in zip(paths, sizes):
            for path in item:
                futures.append(self._pool_().submit(_decode_into, path, buf[off:off + h * w * 3].reshape(h, w, 3)))
                off += h * w * 3
        if scans:
            futures += self._read_scans(scans, buf)
        return {"buf": buf, "frame_bytes": frame_bytes, "sizes": sizes, "flips": flips, "jitters": jitters, "futures": futures,
                "scans": scans}

    def _submit(self, index, draw, alloc, device_depth=True):
        """Start decoding a plan entry: one item, or the items of a step."""
        if self.items_per_step > 1:
            return self._submit_step(index, draw, alloc, device_depth)
        return self._submit_item(index, draw, alloc, device_depth)

    def _submit_item(self, index, draw, alloc, device_depth=True):
        """Start decoding an item: the size from the header of its first frame, one task per frame writing at its offset of
        `alloc(total bytes)`, the scans behind them (device_depth=False: frames only).  -> job dict with the futures."""
        ds = self.dataset
        paths = ds.frame_paths(index)
        h, w = _image_size(paths[0])
        frame_bytes = len(paths) * h * w * 3
        flip, jitters = bool(draw[0]), draw[1]
        scans = None
        if ds.load_depth and device_depth:
            scans = self._scan_job([(p, ds.calib_dir(index), 2) for p in ds.scan_paths(index)], [flip] * ds.n, frame_bytes)
        total = scans["total"] if scans else frame_bytes
        buf = alloc(total)[:total]
        futures = [self._pool_().submit(_decode_into, path, buf[k * h * w * 3:(k + 1) * h * w * 3].reshape(h, w, 3))
                   for k, path in enumerate(paths)]
        if scans:
            futures += self._read_scans(scans, buf)
        return {"buf": buf, "frame_bytes": frame_bytes, "shape": (len(paths), h, w, 3), "flip": flip, "jitters": jitters,
                "futures": futures, "scans": scans}

    def decode_item(self, index, draw=(False, None)):
        """Host half of one item -> (frames (n + 2, Hn, Wn, 3) uint8, flip, jitters); the scans are left to the device half."""
        job = self._submit_item(index, draw, lambda nbytes: np.empty(nbytes, np.uint8), device_depth=False)
        self._wait(job)
        return job["buf"].reshape(job["shape"]), job["flip"], job["jitters"]

    def _upload(self, job, slot):
        """One host-to-device copy + the data step (`_device_half`) -> (batch dict, event that completes it)."""
        self._device_state(self.dataset.n * self.items_per_step)
        if self.items_per_step > 1:
            return self._device_half(job, slot, self._wait(job), lambda dev: self._pre.sequence_batch(
                dev[:job["frame_bytes"]], job["sizes"], self.dataset.n, job["flips"], job["jitters"]))
        return self._device_half(job, slot, self._wait(job), lambda dev: self._pre.sequence(
            dev[:job["frame_bytes"]].view(job["shape"]), job["flip"], job["jitters"]))
