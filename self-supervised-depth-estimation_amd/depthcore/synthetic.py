"""Synthetic KITTI-shaped batches with the reference's dict schema
(datasets/mono_dataset.py:122-183, datasets/kitti_dataset.py:25-28), generated on the device."""
import numpy as np
import torch
import torch.nn.functional as F

KITTI_K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)


def synthetic_batch(batch, height, width, device, num_scales=4, frame_ids=(0, -1, 1), seed=0, smooth=True, packed=False):
    """U(0,1) images (optionally 5x5 box-smoothed so SSIM is not saturated), pyramid by 2x2 means,
    KITTI intrinsics scaled per pyramid level, inv_K = pinv(K).  `packed`: also what the device data step emits next to
    ("color", f, 0) -- ("color_packed", f, 0), the pixel-interleaved RGBx copy the photometric kernels gather from
    (depthcore.data.GpuPreprocessor, dc_data_to_rgbx) -- for the three frames of the loss."""
    g = torch.Generator(device=device).manual_seed(seed)
    inputs = {}
    for f in frame_ids:
        base = torch.rand(batch, 3, height, width, device=device, generator=g)
        if smooth:
            base = F.avg_pool2d(F.pad(base, (2, 2, 2, 2), mode="reflect"), 5, 1)
        for s in range(num_scales):
            img = base if s == 0 else F.avg_pool2d(base, 2 ** s)
            inputs[("color", f, s)] = img.contiguous()
            inputs[("color_aug", f, s)] = inputs[("color", f, s)]
        if packed and f in (0, -1, 1):
            from . import ops
            inputs[("color_packed", f, 0)] = ops.pack_rgbx(inputs[("color", f, 0)])
    for s in range(num_scales):
        K = KITTI_K.copy()
        K[0, :] *= width // (2 ** s)
        K[1, :] *= height // (2 ** s)
        inv_K = np.linalg.pinv(K)
        inputs[("K", s)] = torch.from_numpy(K).to(device).unsqueeze(0).repeat(batch, 1, 1).contiguous()
        inputs[("inv_K", s)] = torch.from_numpy(inv_K).to(device).unsqueeze(0).repeat(batch, 1, 1).contiguous()
    return inputs


def synthetic_sequence_batch(len_sequence, height, width, device, num_scales=4, frame_ids=(0, -1, 1), seed=0, items=None):
    """One sequence of `len_sequence` frames in the schema of datasets/kitti_dataset_seq.py:110-140 (batch size 1):
    ("color", f, s, j), ("K", s, j), ("inv_K", s, j).
    items = S: instead the ALREADY STACKED dict of a step of S sequences as the loader delivers it (("color", f, s),
    ("color_aug", f, s), ("color_packed", f, 0), ("K", s), ("inv_K", s) with len_sequence * S rows), time-major: frame j of
    item s is row j * S + s (depthcore.data.seq_rows)."""
    if items is not None:
        if int(items) < 1:
            raise ValueError("items must be >= 1, got %r" % (items,))
        return synthetic_batch(len_sequence * int(items), height, width, device, num_scales, frame_ids, seed, packed=True)
    flat = synthetic_batch(len_sequence, height, width, device, num_scales, frame_ids, seed)
    out = {}
    for k, v in flat.items():
        if k[0] == "color_aug":
            continue
        for j in range(len_sequence):
            out[k + (j,)] = v[j:j + 1].contiguous()
    return out


def synthetic_depth_gt(batch, device, seed, height=375, width=1242, density=0.05):
    """Sparse LiDAR-like ground truth ("depth_gt", (batch, 1, height, width) fp32, KITTI's raw size by default): a smooth
    road-like depth field (near at the bottom rows, far at the top) sampled at a `density` fraction of the pixels, quantised
    to 1/256 m as KITTI's uint16 depth maps are (so the values tie heavily), zero where there is no return.  About 1 % of the
    returns are below 1e-3 and 1 % above 80, so that both the trainer's (gt > 0) and the Eigen (1e-3 < gt < 80) masks have
    something to drop.  Drawn on a CPU generator from `seed` (same values on every device), then moved to `device`."""
    g = torch.Generator().manual_seed(int(seed))
    y = torch.linspace(0.0, 1.0, height).view(1, 1, height, 1)
    x = torch.linspace(-1.0, 1.0, width).view(1, 1, 1, width)
    base = 2.0 + 70.0 * (1.0 - y) ** 2 + 3.0 * x.abs()
    depth = base * (1.0 + 0.1 * torch.randn(batch, 1, height, width, generator=g))
    depth = torch.round(depth.clamp(min=0.5) * 256.0) / 256.0
    u = torch.rand(batch, 1, height, width, generator=g)
    ret = u < density
    low = u < density * 0.01
    high = (u >= density * 0.01) & (u < density * 0.02)
    depth = torch.where(low, torch.rand(batch, 1, height, width, generator=g) * 1e-3, depth)
    depth = torch.where(high, 80.0 + 40.0 * torch.rand(batch, 1, height, width, generator=g), depth)
    depth = torch.where(ret, depth, torch.zeros(()))
    return depth.to(torch.float32).contiguous().to(device)
