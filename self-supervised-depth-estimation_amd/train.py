"""Train a model (reference train.py): `python train.py --data_path <kitti_data> --splits_dir <dir> --split <name>`.

MonodepthOptions -> Trainer -> train(): a single process on one GPU.  The split files are read from
`<splits_dir>/<split>/{train,val}_files.txt` (none ship with the project), `--dataset` picks the dataset class and `--png`
the image extension."""
import sys

from options import MonodepthOptions


def main(argv=None):
    opts = MonodepthOptions().parse(argv)
    if opts.use_stereo:
        sys.exit("train.py: --use_stereo is not supported: the trainer has no stereo loss (frame_ids with 's' are never "
                 "supervised); train on the monocular frames [0, -1, 1]")
    from trainer import Trainer
    trainer = Trainer(opts)
    trainer.train()
    trainer.close()


if __name__ == "__main__":
    main()
