"""evaluate_depth_gru.py --gru_version v8 end to end on a tiny KITTI-shaped tree (two drives, two native sizes, nine frames each)
against the composition that existed before it: per test file, the window's frames through encoder -> decoder(pre_disp=True)
-> ConvGRUBlocks_v8.run_sequence at batch 1, the last frame's scale-0 disparity, ops.disp_to_depth."""
import os
import sys

import numpy as np
import pytest
import torch

import kitti_tree as KT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-supervised-depth-estimation_amd")
HN, WN = 64, 128
A, B = sorted(KT.DRIVES)
# shuffled; drive A at frames 0 (a window of one frame), 1 (two), 8 and 7 (seven each), drive B at frame 3 (four)
LINES = ["%s 3 l" % B, "%s 1 l" % A, "%s 8 l" % A, "%s 0 l" % A, "%s 7 l" % A]
TOL = dict(rtol=1e-3, atol=1e-3)                        # the bound test_eval_seq_gpu.py::test_gru_script uses


def _save_gt(splits, name, gts):
    arr = np.empty(len(gts), dtype=object)
    for i, g in enumerate(gts):
        arr[i] = g
    np.savez(os.path.join(splits, "eigen", name), data=arr)


def test_v8_script(tmp_path):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluate_depth_gru as EG
    import trainer as T
    from depthcore import evaluate as E
    from depthcore import ops
    from depthcore.data import GpuPreprocessor
    from depthcore.synthetic import synthetic_depth_gt
    from options import MonodepthOptions
    root = str(tmp_path)
    data, splits = os.path.join(root, "kitti"), os.path.join(root, "splits")
    KT.write_raw_tree(data, frames=9)
    os.makedirs(os.path.join(splits, "eigen"))
    with open(os.path.join(splits, "eigen", "test_files.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    gts = [synthetic_depth_gt(1, "cpu", seed=i, height=60 + 4 * (i % 2), width=200, density=0.3)[0, 0].numpy() for i in range(len(LINES))]
    torch.manual_seed(3)
    tr = T.Trainer(T.default_options(height=HN, width=WN, batch_size=1, gru="v8", len_sequence=3), device=DEV)
    with torch.no_grad():
        for p in tr.models["gru"].parameters():                   # the learned (h0, c0) start at zero: make them count
            p.normal_(0, 0.05)
    weights = tr.save_model(os.path.join(root, "weights"))
    _save_gt(splits, "gt_depths.npz", gts)
    common = ["--load_weights_folder", weights, "--data_path", data, "--splits_dir", splits, "--png", "--eval_mono", "--gru_version", "v8"]
    res = EG.evaluate(MonodepthOptions().parse(common + ["--batch_size", "2", "--save_pred_disps"]))
    saved = np.load(os.path.join(weights, "disps_eigen_split.npy"))
    assert saved.shape == (len(LINES), HN, WN) and saved.dtype == np.float32

    # file by file, batch 1, through the training-time sequence forward
    enc, lstm, dec, h, w = EG.load_networks(MonodepthOptions().parse(common), DEV)
    assert (h, w) == (HN, WN) and type(lstm).__name__ == "ConvGRUBlocks_v8"
    for k, v in tr.models["gru"].state_dict().items():
        assert torch.equal(lstm.state_dict()[k], v), k
    prep = GpuPreprocessor(h, w, num_scales=1, frame_idxs=(0,), device=DEV)
    for net in (enc, lstm, dec):
        net.eval()

    def composition(n_prev):
        want = torch.empty(len(LINES), 1, h, w, device=DEV)
        with torch.no_grad():
            for i, line in enumerate(LINES):
                paths = EG.window_paths(data, line, ".png", n_prev)
                frames = torch.cat([EG.frame_batch(prep, [p], DEV) for p in paths])
                maps = dec(enc(frames), True)
                disp = lstm.run_sequence({("disp", s): maps[("disp", s)] for s in range(4)})[("disp", 0)][-1:]
                want[i] = ops.disp_to_depth(disp, 0.1, 100.0)[0][0]
        return want
    assert [len(EG.window_paths(data, line, ".png")) for line in LINES] == [4, 2, 7, 1, 7]
    want = composition(6)
    err = float(np.abs(saved - want[:, 0].cpu().numpy()).max())
    print("max |script - composition| = %.3e" % err)
    np.testing.assert_allclose(saved, want[:, 0].cpu().numpy(), **TOL)                              # file order
    ref = E.evaluate_depth(want, gts, "eigen")
    np.testing.assert_allclose(res["errors"], ref["errors"], **TOL)
    np.testing.assert_allclose(res["mean_errors"], ref["mean_errors"], **TOL)
    np.testing.assert_allclose(res["ratio_median"], ref["ratio_median"], rtol=1e-3)
    # the windows matter: the prediction of a test file differs from that of its frame alone
    alone = float(np.abs(saved[2] - composition(0)[2, 0].cpu().numpy()).max())
    print("max |window of 7 - frame alone| = %.3e" % alone)
    assert alone > 0

    # another lockstep width, and shorter windows, are what the composition gives for those settings
    res1 = EG.evaluate(MonodepthOptions().parse(common + ["--batch_size", "1"]))
    np.testing.assert_allclose(res1["errors"], ref["errors"], **TOL)
    res2 = EG.evaluate(MonodepthOptions().parse(common + ["--batch_size", "2", "--n_prev_images", "2"]))
    ref2 = E.evaluate_depth(composition(2), gts, "eigen")
    np.testing.assert_allclose(res2["errors"], ref2["errors"], **TOL)
    np.testing.assert_allclose(res2["ratio_median"], ref2["ratio_median"], rtol=1e-3)

    # only the reference's gt_depths_seq.npz: read and un-permuted -- the same result from the same (saved) predictions
    ext = ["--ext_disp_to_eval", os.path.join(weights, "disps_eigen_split.npy")]
    a = EG.evaluate(MonodepthOptions().parse(common + ext))
    assert np.array_equal(a["errors"], res["errors"])
    os.remove(os.path.join(splits, "eigen", "gt_depths.npz"))
    _save_gt(splits, "gt_depths_seq.npz", [gts[i] for i in EG.sequence_order(LINES)])
    b = EG.evaluate(MonodepthOptions().parse(common + ext))
    assert np.array_equal(b["errors"], res["errors"]) and b["ratio_median"] == res["ratio_median"]
    tr.close()
