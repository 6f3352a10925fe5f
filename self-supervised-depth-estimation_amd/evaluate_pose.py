"""Drop-in for the reference's evaluate_pose.py: evaluates a trained pose network on KITTI odometry sequence 09 or 10 with the
same options (options.py) and prints the same line.

    python evaluate_pose.py --load_weights_folder <weights_N> --eval_split odom_9 --data_path kitti_odom
                            [--splits_dir splits] [--png] [--eval_json results.json]

Prediction and scoring run on depthcore's kernels (depthcore.evaluate.predict_poses / evaluate_pose); the host decodes the
images (PIL), reads the split list and the ground-truth poses and writes the outputs.  Where it differs from the reference
(DESIGN 4k):
  - the split list is <splits_dir>/odom/test_files_{09,10}.txt (the project ships no splits) and must name consecutive frames
    of one sequence and one side, as the reference's lists do: every frame is then decoded and resized once, not twice;
  - the encoder is loaded with the keys it has (a checkpoint with extra entries loads);
  - only `--pose_model_type separate_resnet` is evaluated -- the reference's script builds nothing else either.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import networks  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from evaluate_depth import SIDE_MAP, image_batches, readlines  # noqa: E402
from options import MonodepthOptions  # noqa: E402

TRACK_LENGTH = 5                                                # evaluate_pose.py:118


def sequence_id(eval_split):
    assert eval_split == "odom_9" or eval_split == "odom_10", \
        "eval_split should be either odom_9 or odom_10"
    return int(eval_split.split("_")[1])


def split_file(splits_dir, eval_split):
    return os.path.join(splits_dir, "odom", "test_files_{:02d}.txt".format(sequence_id(eval_split)))


def image_path(data_path, folder, frame_index, side, img_ext=".jpg"):
    """kitti_dataset.py:95-102 (KITTIOdomDataset.get_image_path)."""
    return os.path.join(data_path, "sequences/{:02d}".format(int(folder)), "image_{}".format(SIDE_MAP[side]),
                        "{:06d}{}".format(frame_index, img_ext))


def poses_path(data_path, eval_split):
    return os.path.join(data_path, "poses", "{:02d}.txt".format(sequence_id(eval_split)))


def parse_split(lines):
    """Lines "sequence frame_index side" -> (sequence, side, first, last).  Line i stands for the pair (frame_index,
    frame_index + 1) (frame_idxs [0, 1] of evaluate_pose.py:64-65), so scoring a trajectory needs consecutive frames of one
    sequence seen from one side."""
    if not lines:
        raise ValueError("the split list is empty")
    rows = []
    for n, line in enumerate(lines):
        parts = line.split()
        if len(parts) != 3 or parts[2] not in SIDE_MAP:
            raise ValueError("line %d of the split list is not 'sequence frame_index side': %r" % (n + 1, line))
        rows.append((int(parts[0]), int(parts[1]), SIDE_MAP[parts[2]]))
    seq, first, side = rows[0]
    for n, (s, f, sd) in enumerate(rows):
        if s != seq or sd != side or f != first + n:
            raise ValueError("the split list must name consecutive frames of one sequence and one side: line %d is %r, "
                             "expected sequence %d frame %d" % (n + 1, lines[n], seq, first + n))
    return seq, lines[0].split()[2], first, first + len(rows) - 1


def check_pose_model_type(opt):
    if opt.pose_model_type != "separate_resnet":
        raise NotImplementedError("--pose_model_type %s: pose evaluation covers separate_resnet only (the reference's "
                                  "evaluate_pose.py builds ResnetEncoder(num_layers, False, 2) + PoseDecoder(num_ch_enc, 1, 2))"
                                  % opt.pose_model_type)


def load_networks(opt, device):
    check_pose_model_type(opt)
    folder = os.path.expanduser(opt.load_weights_folder)
    pose_encoder = networks.ResnetEncoder(opt.num_layers, False, 2)
    loaded = torch.load(os.path.join(folder, "pose_encoder.pth"), map_location="cpu")
    model_dict = pose_encoder.state_dict()
    pose_encoder.load_state_dict({k: v for k, v in loaded.items() if k in model_dict})
    pose_decoder = networks.PoseDecoder(pose_encoder.num_ch_enc, 1, 2)
    pose_decoder.load_state_dict(torch.load(os.path.join(folder, "pose.pth"), map_location="cpu"))
    return pose_encoder.to(device), pose_decoder.to(device)


def evaluate(opt):
    """evaluate_pose.py:49-129.  Returns (the result of depthcore.evaluate.evaluate_pose, the (N,4,4) predictions)."""
    assert opt.load_weights_folder is not None and os.path.isdir(os.path.expanduser(opt.load_weights_folder)), \
        "Cannot find a folder at {}".format(opt.load_weights_folder)
    seq_id = sequence_id(opt.eval_split)
    check_pose_model_type(opt)
    lines = readlines(split_file(opt.splits_dir, opt.eval_split))
    seq, side, first, last = parse_split(lines)
    img_ext = ".png" if getattr(opt, "png", False) else ".jpg"
    paths = [image_path(opt.data_path, seq, i, side, img_ext) for i in range(first, last + 2)]
    device = torch.device("cuda", torch.cuda.current_device())
    pose_encoder, pose_decoder = load_networks(opt, device)

    print("-> Computing pose predictions")
    frames = image_batches(paths, opt.height, opt.width, opt.batch_size, device)
    pred_poses = E.predict_poses(pose_encoder, pose_decoder, frames, opt.batch_size)

    gt_global_poses = np.loadtxt(poses_path(opt.data_path, opt.eval_split)).reshape(-1, 3, 4)
    res = E.evaluate_pose(pred_poses, gt_global_poses, TRACK_LENGTH)
    print("\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(res["mean"], res["std"]))

    save_path = os.path.join(opt.load_weights_folder, "poses.npy")
    host = pred_poses.cpu().numpy()
    np.save(save_path, host)
    print("-> Predictions saved to", save_path)
    if opt.eval_json:
        out = {"split": opt.eval_split, "sequence": seq_id, "frames": len(paths), "track_length": TRACK_LENGTH,
               "mean": res["mean"], "std": res["std"]}
        with open(opt.eval_json, "w") as f:
            json.dump(out, f, indent=1)
    return res, host


if __name__ == "__main__":
    options = MonodepthOptions()
    evaluate(options.parse())
