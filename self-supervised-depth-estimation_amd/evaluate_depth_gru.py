"""Drop-in for the reference's evaluate_depth_gru_fusion.py with `--gru_version v5` or `v8` (its `evaluate_v5_seq`, lines 504-554,
`evaluate_v8_seq`, lines 557-618, and `evaluate`, lines 622-853): scores a ConvGRU v5 or ConvLSTM v8 model (train_gru.py's
encoder.pth / gru.pth / depth.pth) on a KITTI test split with evaluate_depth.py's options and prints the same table.

    python evaluate_depth_gru.py --load_weights_folder <weights_N> --eval_mono [--eval_split eigen] [--batch_size 16]
                                 [--gru_version v8 [--n_prev_images 6]] [--gru_version v10 [--n_prev_images 10]]
                                 [--data_path kitti_data] [--splits_dir splits] [--eval_json results.json]

v5.  The model is recurrent.  The lines of test_files.txt are grouped by their drive (first field); the drives are taken in sorted
order and a drive's lines sorted as strings (`sorted(test_files[scene])`, so frame "100" comes before frame "20" -- kept);
the hidden state starts at the learned `h0_layer1` and is carried from one TEST FILE of a drive to the next (the frames between
them are skipped, as in the reference); every frame's decoder input is features + (h_cur + h_prev) / 2.  The drives are
independent of each other, so `--batch_size` of them advance in lockstep (depthcore.evaluate.predict_disparities_lockstep):
step t decodes frame t of every drive that still has one (PIL), packs the frames back to back -- their native sizes differ by
drive -- and resizes them in GpuPreprocessor.ragged's two launches.

Where it differs from the reference, beyond evaluate_depth.py's own list:
  - predictions are returned and saved in test_files.txt order, not in the order they were computed, so gt_depths.npz,
    --ext_disp_to_eval and --eval_eigen_to_benchmark mean what they mean for evaluate_depth.py.  `sequence_order(lines)` is
    the permutation; when only the reference's gt_depths_seq.npz (export_gt_depth_seq.py) exists it is read and un-permuted;
  - the split and data paths are the options', not "splits/eigen/test_files.txt" and a fixed kitti_data;
  - the networks' size is the one stored in encoder.pth (the reference resizes to 192 x 640 whatever the checkpoint says);
  - --post_process is refused: the reference's v5 and v8 paths have none, and a mirrored stream under a learned, non-symmetric
    h0 is a different model; gru versions other than v5, v8 and v10 are refused.

v8.  Every test file is a window of its own: the file's frame and up to `--n_prev_images` (6, the reference's
constant) frames before it in the same drive and side, `max(0, f - n_prev) .. f`; the window starts from the learned (h0, c0) of
the four cells, every frame goes through encoder -> decoder(pre_disp) -> the ConvLSTM, and the scale-0 disparity of the LAST
frame is the prediction.  The windows are independent of each other, so `--batch_size` of them advance in lockstep, right
aligned (depthcore.evaluate.predict_disparities_windows): the disparity heads, which the recurrence never reads, run once per
group instead of four times per frame.  Frames shared by the windows of neighbouring test files are computed once per window, as
in the reference.

v10 is the reference's evaluate_depth_gru_fusion_my_v.py (`evaluate_v9_v10_seq`, lines 641-701) for the coarse-to-fine
ConvGRU model: v8's protocol with `ConvGRUBlocks_v9(attention=False)`, windows that start from the learned h0 of the four cells,
and 10 previous frames where v8 has 6.  `--n_prev_images` keeps its default of 6 for every version: `--n_prev_images 10`
reproduces the reference's v10 protocol.  v9 (the attention variant) is not built.
"""
import collections
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import evaluate_depth as ED  # noqa: E402
import networks  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from depthcore import ops  # noqa: E402
from depthcore.data import GpuPreprocessor  # noqa: E402
from depthcore.loader import decode_packed  # noqa: E402
from options import MonodepthOptions  # noqa: E402


def scenes_of(lines):
    """evaluate_depth_gru_fusion.py:728-731 + :505, :514 -> [(scene, [indices into `lines`, in the order the state visits them])]."""
    by_scene = collections.defaultdict(list)
    for i, line in enumerate(lines):
        by_scene[line.split()[0]].append(i)
    return [(scene, sorted(by_scene[scene], key=lambda i: (lines[i], i))) for scene in sorted(by_scene)]


def sequence_order(lines):
    """The permutation from sequence order to file order: entry j is the index in `lines` (test_files.txt) of the j-th frame the
    reference's evaluate_v5_seq predicts.  pred_seq == pred_file[order], gt_file == gt_seq[np.argsort(order)]."""
    return np.array([i for _, ids in scenes_of(lines) for i in ids], np.int64)


N_PREV_IMAGES = 6            # evaluate_depth_gru_fusion.py:558


N_PREV_IMAGES_MY_V = 10      # evaluate_depth_gru_fusion_my_v.py:642 (v9 / v10): asked for with --n_prev_images 10


VERSIONS = {"v5": "ConvGRUBlocks_v5, evaluate_v5_seq", "v8": "ConvGRUBlocks_v8, evaluate_v8_seq"}     # evaluate_depth_gru_fusion.py's
MY_V_VERSIONS = {"v10": "ConvGRUBlocks_v9(attention=False), evaluate_v9_v10_seq"}                     # evaluate_depth_gru_fusion_my_v.py's
WINDOWED = ("v8", "v10")     # one window per test file (predict_windows); v5 carries its state along a drive


def check_options(opt, versions=("v5",)):
    """Refuses what the evaluation of the gru versions `versions` does not cover.  The one-argument form is the check of the
    v5 evaluation and stays what it was (callers and a test rely on it refusing every other version); `evaluate` passes
    both tables' versions, so the script takes v8 and v10 as well."""
    if opt.eval_split.startswith("odom"):
        raise ValueError("eval_split %r is pose evaluation: run evaluate_pose.py" % opt.eval_split)
    if getattr(opt, "gru_version", "v5") not in versions:
        raise NotImplementedError("gru_version %r: this evaluation covers %s" % (
            opt.gru_version, " and ".join("%s (%s)" % (v, {**VERSIONS, **MY_V_VERSIONS}[v]) for v in versions)))
    if opt.post_process:
        raise NotImplementedError("--post_process with the recurrent front-ends: the reference's v5, v8 and v10 evaluations have none, "
                                  "and a mirrored stream under a learned, non-symmetric initial state is a different model")
    if getattr(opt, "n_prev_images", N_PREV_IMAGES) < 0:
        raise ValueError("--n_prev_images must not be negative")
    assert sum((opt.eval_mono, opt.eval_stereo)) == 1, \
        "Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo"


def load_networks(opt, device):
    """evaluate_depth.load_networks' encoder and decoder + gru.pth into ConvGRUBlocks_v5, or with --gru_version v8 / v10 into
    ConvGRUBlocks_v8 / ConvGRUBlocks_v9 (num_ch_dec from the decoder), at the size stored in encoder.pth."""
    encoder, decoder, height, width = ED.load_networks(opt, device)
    version = getattr(opt, "gru_version", "v5")
    if version in WINDOWED:
        blocks = networks.ConvGRUBlocks_v8 if version == "v8" else networks.ConvGRUBlocks_v9
        gru = blocks(kernel_size=(3, 3), bias=True, device="cpu", attention=False, height=height, width=width,
                     num_ch_dec=tuple(int(c) for c in decoder.num_ch_dec[:4]))
    else:
        gru = networks.ConvGRUBlocks_v5(kernel_size=(3, 3), bias=True, device="cpu", height=height, width=width,
                                        num_ch_enc=tuple(int(c) for c in encoder.num_ch_enc))
    gru.load_state_dict(torch.load(os.path.join(os.path.expanduser(opt.load_weights_folder), "gru.pth"), map_location="cpu"))
    return encoder, gru.to(device), decoder, height, width


def frame_batch(prep, paths, device):
    """One lockstep step's frames: PIL decode, packed back to back, GpuPreprocessor.ragged (no flip, no jitter) -> (B,3,h,w)."""
    packed, sizes = decode_packed(paths)
    return prep.ragged(torch.from_numpy(packed).to(device), sizes)[("color", 0, 0)]


def window_paths(data_path, line, img_ext=".jpg", n_prev=N_PREV_IMAGES):
    """evaluate_depth_gru_fusion.py:580-586: the image paths of a test line's window, frames max(0, f - n_prev) .. f of its
    drive and side, in order (the line's own frame last)."""
    folder, frame, side = line.split()
    frame = int(frame)
    return [ED.image_path(data_path, "%s %d %s" % (folder, k, side), img_ext) for k in range(max(0, frame - n_prev), frame + 1)]


def predict_windows(opt, device):
    """v8 / v10 -> (N,1,h,w) scaled disparities in test_files.txt order: one window per test file, --batch_size windows in
    lockstep."""
    encoder, lstm, decoder, height, width = load_networks(opt, device)
    lines = ED.readlines(os.path.join(opt.splits_dir, opt.eval_split, "test_files.txt"))
    img_ext = ".png" if getattr(opt, "png", False) else ".jpg"
    windows = [window_paths(opt.data_path, line, img_ext, getattr(opt, "n_prev_images", N_PREV_IMAGES)) for line in lines]
    prep = GpuPreprocessor(height, width, num_scales=1, frame_idxs=(0,), device=device)
    print("-> Computing predictions with size {}x{}: {} windows of up to {} frames, {} in lockstep".format(
        width, height, len(windows), max(len(w) for w in windows), opt.batch_size))

    def batch(j, ids, frame_of):
        return frame_batch(prep, [windows[c][t] for c, t in zip(ids, frame_of)], device)
    return E.predict_disparities_windows(encoder, decoder, lstm, [len(w) for w in windows], batch, opt.min_depth, opt.max_depth,
                                         opt.batch_size)


def predict(opt, device):
    """-> (N,1,h,w) scaled disparities in test_files.txt order."""
    if getattr(opt, "gru_version", "v5") in WINDOWED:
        return predict_windows(opt, device)
    encoder, gru, decoder, height, width = load_networks(opt, device)
    lines = ED.readlines(os.path.join(opt.splits_dir, opt.eval_split, "test_files.txt"))
    img_ext = ".png" if getattr(opt, "png", False) else ".jpg"
    scenes = scenes_of(lines)
    prep = GpuPreprocessor(height, width, num_scales=1, frame_idxs=(0,), device=device)
    print("-> Computing predictions with size {}x{}: {} scenes, {} in lockstep".format(width, height, len(scenes), opt.batch_size))

    def batch(t, ids):
        return frame_batch(prep, [ED.image_path(opt.data_path, lines[scenes[c][1][t]], img_ext) for c in ids], device)
    per_scene = E.predict_disparities_lockstep(encoder, gru, decoder, [len(ids) for _, ids in scenes], batch,
                                               opt.min_depth, opt.max_depth, opt.batch_size)
    row = {i: per_scene[c][t:t + 1] for c, (_, ids) in enumerate(scenes) for t, i in enumerate(ids)}
    return ops.stack_frames([[row[i] for i in range(len(lines))]])[0]


def load_gt_depths(opt):
    """gt_depths.npz (file order), or the reference's gt_depths_seq.npz (sequence order) put back into file order."""
    split_dir = os.path.join(opt.splits_dir, opt.eval_split)
    if os.path.exists(os.path.join(split_dir, "gt_depths.npz")):
        return ED.load_gt_depths(opt)
    seq = np.load(os.path.join(split_dir, "gt_depths_seq.npz"), fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    order = sequence_order(ED.readlines(os.path.join(split_dir, "test_files.txt")))
    if len(seq) != len(order):
        raise ValueError("gt_depths_seq.npz holds %d maps for %d test files" % (len(seq), len(order)))
    return seq[np.argsort(order)]


def evaluate(opt):
    """evaluate_depth_gru_fusion.py:622-853 for gru_version v5 / v8 and evaluate_depth_gru_fusion_my_v.py for v10.  Returns depthcore.evaluate.evaluate_depth's result, or None when
    nothing is scored."""
    check_options(opt, tuple(VERSIONS) + tuple(MY_V_VERSIONS))
    device = torch.device("cuda", torch.cuda.current_device())
    pred_disps = predict(opt, device) if opt.ext_disp_to_eval is None else ED.load_external_disparities(opt, device)
    return ED.finish(opt, pred_disps, load_gt_depths)


if __name__ == "__main__":
    evaluate(MonodepthOptions().parse())
