"""depthcore.loader.BatchLoader, device half: prefetched batches equal synchronous ones, a held batch is never
overwritten by later ones (staging buffers, side stream), keys and shapes are the same every step."""
import pytest
import torch

from kitti_tree import DRIVES, write_raw_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import datasets
    root = str(tmp_path_factory.mktemp("kitti"))
    write_raw_tree(root, frames=6)
    lines = ["%s %d l" % (drive, i) for drive in sorted(DRIVES) for i in range(6)]          # frames 0 and 5: a neighbour is missing
    return datasets.KITTIRAWDataset(root, lines, 32, 64, [0, -1, 1], 4, is_train=True, img_ext=".png")


def _six(dataset, prefetch):
    from depthcore.loader import BatchLoader
    ld = BatchLoader(dataset, 2, num_workers=4, device=DEV, seed=3, prefetch=prefetch)
    assert len(ld) == 6
    batches = list(ld)
    torch.cuda.synchronize()
    ld.close()
    return ld, batches


def test_prefetched_batches_equal_synchronous_ones(dataset):
    ld, want = _six(dataset, 0)
    _, got = _six(dataset, 2)
    assert len(want) == len(got) == 6
    for a, b in zip(want, got):
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # the epoch mixes both drives' sizes inside a batch and draws flips and jitters
    plan = ld.plan()
    sizes = [{DRIVES[dataset.filenames[i].split()[0]] for i in idx} for idx, _ in plan]
    assert any(len(s) == 2 for s in sizes)
    assert any(d[0] for _, draws in plan for d in draws) and any(d[1] is not None for _, draws in plan for d in draws)
    assert any(not torch.equal(b[("color", 0, 0)], b[("color_aug", 0, 0)]) for b in want)


def test_held_batch_survives_further_fetches(dataset):
    from depthcore.loader import BatchLoader
    ld = BatchLoader(dataset, 2, num_workers=4, device=DEV, seed=3, prefetch=2)
    it = iter(ld)
    held = next(it)
    torch.cuda.synchronize()
    copy = {k: v.clone() for k, v in held.items()}
    next(it), next(it)
    torch.cuda.synchronize()
    for k in held:
        assert torch.equal(held[k], copy[k]), k
    it.close()
    ld.close()


def test_keys_and_shapes_are_constant_and_all_tensors(dataset):
    _, batches = _six(dataset, 2)
    B, frames = 2, (0, -1, 1)
    want = {(n, f, s): (B, 3, 32 >> s, 64 >> s) for n in ("color", "color_aug") for f in frames for s in range(4)}
    want.update({("color_packed", f, 0): (B, 32, 64, 4) for f in frames})
    want.update({(n, s): (B, 4, 4) for n in ("K", "inv_K") for s in range(4)})
    for b in batches:
        assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 for v in b.values())
        assert {k: tuple(v.shape) for k, v in b.items()} == want
    K = batches[0][("K", 1)][1].cpu()
    assert torch.allclose(K, torch.tensor([[0.58 * 32, 0, 16, 0], [0, 1.92 * 16, 8, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
