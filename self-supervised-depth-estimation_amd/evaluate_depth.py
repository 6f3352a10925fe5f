"""Drop-in for the reference's evaluate_depth.py: evaluates a trained depth model on a KITTI test split with the same options
(options.py, "EVALUATION") and prints the same table.

    python evaluate_depth.py --load_weights_folder <weights_N> --eval_mono [--post_process] [--eval_split eigen]
                             [--data_path kitti_data] [--splits_dir splits] [--eval_json results.json]

Prediction and scoring run on depthcore's kernels (depthcore.evaluate); the host decodes the images (PIL), reads the splits
and writes the outputs.  Where it differs from the reference:
  - the disparities are resized to the ground truth's size by F.interpolate(bilinear, align_corners=False)'s expression --
    the half-pixel sampling of cv2.resize(INTER_LINEAR) when upsampling, not its bits (cv2 is not a dependency);
  - saved disparities (--save_pred_disps) are fp32 also with --post_process (the reference saves fp64 there);
  - gt_depths.npz is read only when something is scored, so --no_eval and the benchmark split need none;
  - the encoder is ResnetEncoder(--num_layers) (the reference builds a resnet18 whatever the option says), or
    ResnetEncoderAttention(--num_layers) with --model rn_encoder_with_attention / rn_fusion (trainer_dpt.py:78-92); weights
    saved from the other class are refused.  load_networks() without a `model` option (test_simple.py) takes the class the
    checkpoint was saved from;
  - the Fusion_v3 and ConvGRU front-ends are refused here (NotImplementedError), as in the reference, where they have scripts
    of their own: evaluate_depth_fusion_v3.py and evaluate_depth_gru.py next to this file.
"""
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import networks  # noqa: E402
from depthcore import evaluate as E  # noqa: E402
from depthcore import ops  # noqa: E402
from depthcore.data import GpuPreprocessor  # noqa: E402
from depthcore.loader import decode_packed  # noqa: E402
from options import MonodepthOptions  # noqa: E402

STEREO_SCALE_FACTOR = ops.STEREO_SCALE_FACTOR
SIDE_MAP = {"2": 2, "3": 3, "l": 2, "r": 3}          # kitti_dataset.py:31


def readlines(filename):
    with open(filename, "r") as f:
        return f.read().splitlines()


def image_path(data_path, line, img_ext=".jpg"):
    """kitti_dataset.py:65-69 with mono_dataset.py:145-156's parsing of a split line "folder [frame_index side]"."""
    parts = line.split()
    folder = parts[0]
    frame_index = int(parts[1]) if len(parts) == 3 else 0
    side = parts[2] if len(parts) == 3 else None
    return os.path.join(data_path, folder, "image_0{}/data".format(SIDE_MAP[side]), "{:010d}{}".format(frame_index, img_ext))


def image_batches(paths, height, width, batch_size, device):
    """The eval-mode ("color", 0, 0) inputs of KITTIRAWDataset(is_train=False): PIL decode, then GpuPreprocessor's Lanczos
    resize (no flip, no colour augmentation) -- batches of up to batch_size images of one native size, in file order."""
    prep = GpuPreprocessor(height, width, num_scales=1, frame_idxs=(0,), device=device)
    pending = []

    def flush():
        native = torch.from_numpy(np.stack(pending)[None]).to(device)
        pending.clear()
        return prep(native)[("color", 0, 0)]

    for p in paths:
        flat, [(h, w)] = decode_packed([p])
        img = flat.reshape(h, w, 3)
        if pending and (img.shape != pending[0].shape or len(pending) == batch_size):
            yield flush()
        pending.append(img)
    if pending:
        yield flush()


def load_networks(opt, device):
    folder = os.path.expanduser(opt.load_weights_folder)
    if not os.path.isdir(folder):
        raise FileNotFoundError("Cannot find a folder at {}".format(folder))
    print("-> Loading weights from {}".format(folder))
    encoder_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location="cpu")
    # the encoder class: what --model names (as trainer.py builds it); a caller without that option (test_simple.py) gets the
    # class the checkpoint was saved from.  A checkpoint of the other class is an error, never a silently dropped layer.
    saved_cls = networks.ResnetEncoderAttention if any(k.startswith("atten") for k in encoder_dict) else networks.ResnetEncoder
    cls = networks.depth_encoder_class(opt.model) if hasattr(opt, "model") else saved_cls
    if cls is not saved_cls:
        raise ValueError("--model {!r} builds {} but {} holds a {} (its keys {} atten1..4.*): pass the --model the weights were "
                         "trained with".format(opt.model, cls.__name__, os.path.join(folder, "encoder.pth"), saved_cls.__name__,
                                               "include" if saved_cls is networks.ResnetEncoderAttention else "lack"))
    encoder = cls(opt.num_layers, False)
    decoder = networks.DepthDecoder(encoder.num_ch_enc)
    model_dict = encoder.state_dict()
    encoder.load_state_dict({k: v for k, v in encoder_dict.items() if k in model_dict})
    decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location="cpu"))
    return encoder.to(device), decoder.to(device), int(encoder_dict["height"]), int(encoder_dict["width"])


def evaluate(opt):
    """evaluate_depth.py:59-236.  Returns the result of depthcore.evaluate.evaluate_depth, or None when nothing is scored."""
    if opt.eval_split.startswith("odom"):
        raise ValueError("eval_split %r is pose evaluation: run evaluate_pose.py" % opt.eval_split)
    if getattr(opt, "fusion", None) or getattr(opt, "gru", None):
        raise NotImplementedError("evaluating the %s front-end: run %s (this script scores the plain encoder + decoder)"
                                  % (("Fusion_v3", "evaluate_depth_fusion_v3.py") if opt.fusion else ("ConvGRU", "evaluate_depth_gru.py")))
    assert sum((opt.eval_mono, opt.eval_stereo)) == 1, \
        "Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo"
    device = torch.device("cuda", torch.cuda.current_device())
    split_dir = os.path.join(opt.splits_dir, opt.eval_split)

    if opt.ext_disp_to_eval is None:
        encoder, decoder, height, width = load_networks(opt, device)
        filenames = readlines(os.path.join(split_dir, "test_files.txt"))
        img_ext = ".png" if getattr(opt, "png", False) else ".jpg"
        paths = [image_path(opt.data_path, line, img_ext) for line in filenames]
        print("-> Computing predictions with size {}x{}".format(width, height))
        pred_disps = E.predict_disparities(encoder, decoder, image_batches(paths, height, width, opt.batch_size, device),
                                           opt.min_depth, opt.max_depth, opt.post_process, opt.batch_size)
    else:
        pred_disps = load_external_disparities(opt, device)

    return finish(opt, pred_disps)


def load_external_disparities(opt, device):
    """--ext_disp_to_eval (evaluate_depth.py:138-147): saved disparities, in test_files.txt order, onto the device."""
    print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
    host = np.load(opt.ext_disp_to_eval)
    if opt.eval_eigen_to_benchmark:
        host = host[np.load(os.path.join(opt.splits_dir, "benchmark", "eigen_to_benchmark_ids.npy"))]
    host = np.ascontiguousarray(host, np.float32)
    return torch.from_numpy(host.reshape(host.shape[0], 1, host.shape[-2], host.shape[-1])).to(device)


def load_gt_depths(opt):
    split_dir = os.path.join(opt.splits_dir, opt.eval_split)
    return np.load(os.path.join(split_dir, "gt_depths.npz"), fix_imports=True, encoding="latin1", allow_pickle=True)["data"]


def finish(opt, pred_disps, load_gt=load_gt_depths):
    """evaluate_depth.py:149-236 from the predictions on: --save_pred_disps, --no_eval, the benchmark export, scoring, the table
    and --eval_json.  pred_disps (N,1,h,w) on the device in test_files.txt order; load_gt(opt) -> the ground truths in that
    order, called only when something is scored.  Shared by evaluate_depth_gru.py and evaluate_depth_fusion_v3.py."""
    if opt.save_pred_disps:
        output_path = os.path.join(opt.load_weights_folder, "disps_{}_split.npy".format(opt.eval_split))
        print("-> Saving predicted disparities to ", output_path)
        np.save(output_path, pred_disps[:, 0].cpu().numpy())          # (N, h, w) as the reference's, fp32

    if opt.no_eval:
        print("-> Evaluation disabled. Done.")
        return None

    if opt.eval_split == "benchmark":
        save_dir = os.path.join(opt.load_weights_folder, "benchmark_predictions")
        print("-> Saving out benchmark predictions to {}".format(save_dir))
        os.makedirs(save_dir, exist_ok=True)
        depth = ops.depth_png16(pred_disps, ops.BENCHMARK_SIZE, STEREO_SCALE_FACTOR)
        depth = depth.view(torch.int16).cpu().numpy().view(np.uint16)
        for idx in range(depth.shape[0]):
            Image.fromarray(depth[idx]).save(os.path.join(save_dir, "{:010d}.png".format(idx)))
        print("-> No ground truth is available for the KITTI benchmark, so not evaluating. Done.")
        return None

    gt_depths = load_gt(opt)
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by {}".format(STEREO_SCALE_FACTOR))
        opt.disable_median_scaling = True
        opt.pred_depth_scale_factor = STEREO_SCALE_FACTOR
    else:
        print("   Mono evaluation - using median scaling")
    res = E.evaluate_depth(pred_disps, gt_depths, opt.eval_split, not opt.disable_median_scaling, opt.pred_depth_scale_factor)
    if not opt.disable_median_scaling:
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(res["ratio_median"], res["ratio_std"]))
    mean_errors = res["mean_errors"]
    print("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    print(("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\")
    if opt.eval_json:
        out = {"split": opt.eval_split, "images": int(res["errors"].shape[0]), "post_process": bool(opt.post_process),
               "median_scaling": not opt.disable_median_scaling, "scale_factor": float(opt.pred_depth_scale_factor),
               "mean_errors": {k: float(v) for k, v in zip(res["names"], mean_errors)},
               "ratio_median": res["ratio_median"], "ratio_std": res["ratio_std"]}
        with open(opt.eval_json, "w") as f:
            json.dump(out, f, indent=1)
    print("\n-> Done!")
    return res


if __name__ == "__main__":
    options = MonodepthOptions()
    evaluate(options.parse())
