"""Drop-in for the reference's test_simple.py: a trained depth model and an image or a folder of images in, for every image
`<name>_disp.npy` (the scaled disparity at network resolution, (1,1,h,w) float32) and `<name>_disp.jpeg` (the magma rendering of
the disparity at the photo's own size) out.

    python test_simple.py --image_path <file or folder> --load_weights_folder <weights_N> [--ext jpg] [--num_layers 18]
                          [--batch_size 16]

Prediction and rendering run on depthcore's kernels (depthcore.evaluate: predict_disparities, render_disparities); the host
decodes the photos and encodes the JPEGs (PIL) and receives Ho x Wo x 3 bytes and two floats per image.  matplotlib, cv2 and
torchvision are not imported.  Where it differs from the reference:
  - weights are NEVER downloaded: --load_weights_folder names a checkpoint folder (encoder.pth, depth.pth -- what
    evaluate_depth.py loads); --model_name NAME means models/NAME if that folder exists and is an error otherwise;
  - --no_cuda is refused: there is no CPU path;
  - the images of a folder are taken in sorted order and run in batches of one native size (--batch_size);
  - the picture is rendered from the scaled disparity that is saved (an affine map of the sigmoid output, so the same picture up
    to rounding), its 95th percentile formed with numpy 1.x's fp64 virtual index;
  - the encoder is ResnetEncoder(--num_layers) (the reference builds a resnet18).
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MIN_DEPTH, MAX_DEPTH = 0.1, 100.0                   # test_simple.py:133


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Single-image inference: disparity .npy and magma .jpeg for an image or a folder.")
    parser.add_argument("--image_path", type=str, required=True, help="path to a test image or folder of images")
    parser.add_argument("--load_weights_folder", type=str, default=None, help="checkpoint folder holding encoder.pth and depth.pth")
    parser.add_argument("--model_name", type=str, default=None,
                        help="name of a model folder under models/ (used when --load_weights_folder is not given; never downloaded)")
    parser.add_argument("--ext", type=str, default="jpg", help="image extension to search for in folder")
    parser.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152], help="number of resnet layers")
    parser.add_argument("--batch_size", type=int, default=16, help="images of one native size per network batch")
    parser.add_argument("--no_cuda", action="store_true", help="refused: there is no CPU path")
    return parser.parse_args(argv)


def weights_folder(args):
    """The checkpoint folder the options name.  Nothing is ever fetched: a model that is not on disk is an error."""
    if args.load_weights_folder:
        return os.path.expanduser(args.load_weights_folder)
    if not args.model_name:
        raise ValueError("You must specify --load_weights_folder (or --model_name of a folder under models/)")
    folder = os.path.join("models", args.model_name)
    if not os.path.isdir(folder):
        raise FileNotFoundError("--model_name {}: there is no folder {}, and weights are never downloaded -- put the model there "
                                "or pass --load_weights_folder".format(args.model_name, folder))
    return folder


def find_images(image_path, ext):
    """test_simple.py:93-103 -> (paths, output directory); a folder's images in sorted order."""
    if os.path.isfile(image_path):
        return [image_path], os.path.dirname(image_path)
    if os.path.isdir(image_path):
        return sorted(glob.glob(os.path.join(image_path, "*.{}".format(ext)))), image_path
    raise FileNotFoundError("Can not find args.image_path: {}".format(image_path))


def predict_folder(args, keep_rgb=False):
    """test_simple.py:53-150.  -> one dict per processed image: image, npy, jpeg (paths), size (Ho, Wo), range (vmin, vmax) and,
    with keep_rgb, rgb -- the (Ho, Wo, 3) uint8 array handed to PIL."""
    if args.no_cuda:
        raise ValueError("--no_cuda: there is no CPU path, the networks and the rendering run on HIP kernels only")
    if args.batch_size <= 0:
        raise ValueError("--batch_size must be positive")
    folder = weights_folder(args)
    paths, output_directory = find_images(args.image_path, args.ext)

    import evaluate_depth as ED
    from depthcore import evaluate as E

    device = torch.device("cuda", torch.cuda.current_device())
    opt = argparse.Namespace(load_weights_folder=folder, num_layers=args.num_layers)
    encoder, decoder, feed_height, feed_width = ED.load_networks(opt, device)

    print("-> Predicting on {:d} test images".format(len(paths)))
    # don't try to predict disparity for a disparity image!
    todo = [(idx, p) for idx, p in enumerate(paths) if not p.endswith("_disp.jpg")]
    records = []
    done = 0
    for x in ED.image_batches([p for _, p in todo], feed_height, feed_width, args.batch_size, device):
        batch = todo[done:done + x.shape[0]]                     # image_batches keeps file order; one native size per batch
        done += x.shape[0]
        with Image.open(batch[0][1]) as im:
            original_width, original_height = im.size
        # the training flags of every submodule are restored when this returns
        disps = E.predict_disparities(encoder, decoder, x, MIN_DEPTH, MAX_DEPTH, False, args.batch_size)
        images, ranges = E.render_disparities(disps, (original_height, original_width))
        scaled = disps.cpu().numpy()
        for k, (idx, image_path) in enumerate(batch):
            output_name = os.path.splitext(os.path.basename(image_path))[0]
            name_dest_npy = os.path.join(output_directory, "{}_disp.npy".format(output_name))
            np.save(name_dest_npy, scaled[k:k + 1])
            name_dest_im = os.path.join(output_directory, "{}_disp.jpeg".format(output_name))
            Image.fromarray(images[k]).save(name_dest_im)
            rec = {"image": image_path, "npy": name_dest_npy, "jpeg": name_dest_im, "size": (original_height, original_width),
                   "range": (float(ranges[k, 0]), float(ranges[k, 1]))}
            if keep_rgb:
                rec["rgb"] = images[k]
            records.append(rec)
            print("   Processed {:d} of {:d} images - saved prediction to {}".format(idx + 1, len(paths), name_dest_im))
    print("-> Done!")
    return records


if __name__ == "__main__":
    predict_folder(parse_args())
