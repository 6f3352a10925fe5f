"""Drop-in for the reference's evaluate_depth_fusion_v3.py (lines 63-165 + the scoring it shares with evaluate_depth.py): scores
a Fusion_v3 model (encoder.pth / depth.pth / fusion.pth of `--fusion v3` training) on a KITTI test split with
evaluate_depth.py's options and prints the same table.

    python evaluate_depth_fusion_v3.py --load_weights_folder <weights_N> --eval_mono [--post_process] [--disable_attention]
                                       [--eval_split eigen] [--data_path kitti_data] [--splits_dir splits]

Every test file contributes frames [-2, -1, 0] of its drive; a neighbour whose file does not exist is replaced by frame 0
(datasets/mono_dataset.py).  A batch is stacked frame-major along the batch, as Trainer._depth_branch stacks it, and runs
encoder -> DepthDecoder -> Fusion_v3 (depthcore.evaluate.predict_disparities_fusion).

Where it differs from the reference, beyond evaluate_depth.py's own list:
  - --post_process runs the mirrored triplets as a fusion call of their own and blends the two results
    (ops.post_process_disparity).  The reference concatenates [x; flip(x)] before the networks; Fusion_v3 then cuts that
    batch of 6B into three chunks of 2B, which mixes frames with mirrored frames of other instants;
  - Fusion_v3(attention=not --disable_attention), as the trainer builds it (the reference always builds the attention form);
  - the loop over the first 100 dataset items that the reference runs before it predicts is not reproduced.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import evaluate_depth as ED  # noqa: E402
import networks  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from depthcore import ops  # noqa: E402
from depthcore.data import GpuPreprocessor  # noqa: E402
from depthcore.loader import decode_packed  # noqa: E402
from options import MonodepthOptions  # noqa: E402

FRAMES = (-2, -1, 0)                  # evaluate_depth_fusion_v3.py:98, :142


def triplet_paths(data_path, line, img_ext=".jpg"):
    """The files of frames [-2, -1, 0] of a split line "folder frame_index side"; a missing neighbour -> frame 0's file."""
    folder, frame_index, side = line.split()
    centre = ED.image_path(data_path, line, img_ext)
    paths = [ED.image_path(data_path, "{} {} {}".format(folder, int(frame_index) + i, side), img_ext) for i in FRAMES]
    return [p if os.path.exists(p) else centre for p in paths]


def triplet_batches(lines, data_path, img_ext, height, width, batch_size, device):
    """(3,B,3,h,w) batches of up to batch_size test files in file order: PIL decode, the frames packed frame-major, resized by
    GpuPreprocessor.ragged (an item's three frames share its native size; the items of a batch need not)."""
    prep = GpuPreprocessor(height, width, num_scales=1, frame_idxs=FRAMES, device=device)
    for i0 in range(0, len(lines), batch_size):
        items = [triplet_paths(data_path, line, img_ext) for line in lines[i0:i0 + batch_size]]
        packed, sizes = decode_packed([item[j] for j in range(3) for item in items])
        out = prep.ragged(torch.from_numpy(packed).to(device), sizes[:len(items)])
        stacked = ops.stack_frames([[out[("color", f, 0)] for f in FRAMES]])[0]
        yield stacked.view((3, len(items)) + tuple(stacked.shape[1:]))


def load_networks(opt, device):
    encoder, decoder, height, width = ED.load_networks(opt, device)
    fusion = networks.Fusion_v3(attention=not getattr(opt, "disable_attention", False))
    fusion.load_state_dict(torch.load(os.path.join(os.path.expanduser(opt.load_weights_folder), "fusion.pth"), map_location="cpu"))
    return encoder, decoder, fusion.to(device), height, width


def evaluate(opt):
    """evaluate_depth_fusion_v3.py:63-165 and the scoring behind it.  Returns depthcore.evaluate.evaluate_depth's result, or None
    when nothing is scored."""
    if opt.eval_split.startswith("odom"):
        raise ValueError("eval_split %r is pose evaluation: run evaluate_pose.py" % opt.eval_split)
    assert sum((opt.eval_mono, opt.eval_stereo)) == 1, \
        "Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo"
    device = torch.device("cuda", torch.cuda.current_device())
    if opt.ext_disp_to_eval is None:
        encoder, decoder, fusion, height, width = load_networks(opt, device)
        lines = ED.readlines(os.path.join(opt.splits_dir, opt.eval_split, "test_files.txt"))
        img_ext = ".png" if getattr(opt, "png", False) else ".jpg"
        print("-> Computing predictions with size {}x{}".format(width, height))
        pred_disps = E.predict_disparities_fusion(
            encoder, decoder, fusion, triplet_batches(lines, opt.data_path, img_ext, height, width, opt.batch_size, device),
            opt.min_depth, opt.max_depth, opt.post_process, opt.batch_size)
    else:
        pred_disps = ED.load_external_disparities(opt, device)
    return ED.finish(opt, pred_disps)


if __name__ == "__main__":
    evaluate(MonodepthOptions().parse())
