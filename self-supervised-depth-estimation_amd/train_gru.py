"""Train the ConvGRU front-end on KITTI sequences (reference train_gru.py):
`python train_gru.py --data_path <kitti_data> --splits_dir <dir> --split <name> --len_sequence 10`.

MonodepthOptions -> Trainer -> train_sequences(): a single process on one GPU.  The drive lists are read from
`<splits_dir>/<split>/{train,val}_sequences.txt` ("date/drive" per line; none ship with the project); `--len_sequence`,
`--train_n_tuples`, `--test_n_tuples` and `--h_s_epoch` are the reference's.  One sequence item is one step: the batch size is 1."""
import sys

from options import MonodepthOptions


def main(argv=None):
    opts = MonodepthOptions().parse(argv)
    if opts.use_stereo:
        sys.exit("train_gru.py: --use_stereo is not supported: the trainer has no stereo loss (frame_ids with 's' are never "
                 "supervised); train on the monocular frames [0, -1, 1]")
    if not opts.gru:
        opts.gru = "v5"
    opts.batch_size = 1                     # trainer_gru.py:206-240: DataLoader(batch_size=1), one sequence per step
    from trainer import Trainer
    trainer = Trainer(opts)
    trainer.train_sequences()
    trainer.close()


if __name__ == "__main__":
    main()
