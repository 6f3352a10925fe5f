"""Train the ConvGRU front-end on KITTI sequences (reference train_gru.py):
`python train_gru.py --data_path <kitti_data> --splits_dir <dir> --split <name> --len_sequence 10`.

MonodepthOptions -> Trainer -> train_sequences(): a single process on one GPU.  The drive lists are read from
`<splits_dir>/<split>/{train,val}_sequences.txt` ("date/drive" per line; none ship with the project); `--len_sequence`,
`--train_n_tuples`, `--test_n_tuples` and `--h_s_epoch` are the reference's.  One sequence item is one step: the batch size is 1.
`--gru_version` picks the front-end: `v5` (ConvGRU inside the skip connections, the default) `v8` (ConvLSTM behind the decoder)
or `v10` (ConvGRU cells in v8's coarse-to-fine arrangement).
`--seq_batch S` (beyond the reference, default 1) trains S sequence items per step in lockstep: the loss and the BatchNorm
statistics run over the S * len_sequence frames, every parameter is shared, the learning rate is not rescaled."""
import sys

from options import MonodepthOptions


def main(argv=None):
    opts = MonodepthOptions().parse(argv)
    if opts.use_stereo:
        sys.exit("train_gru.py: --use_stereo is not supported: the trainer has no stereo loss (frame_ids with 's' are never "
                 "supervised); train on the monocular frames [0, -1, 1]")
    if not opts.gru:
        opts.gru = opts.gru_version         # trainer_gru.py:128-144: "v5" (the default), "v8" or "v10"; the Trainer refuses the others
    opts.batch_size = 1                     # trainer_gru.py:206-240: DataLoader(batch_size=1), one sequence per step
    # (opts.seq_batch sequences per step is its own option: batch_size keeps the reference's meaning and value)
    from trainer import Trainer
    trainer = Trainer(opts)
    trainer.train_sequences()
    trainer.close()


if __name__ == "__main__":
    main()
