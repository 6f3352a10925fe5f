"""ops.bn_eval (eval-mode BatchNorm2d on dc_bn_eval_coef + dc_bn_apply / dc_bn_eval_bwd) against CPU fp64
F.batch_norm(training=False), forward and every gradient; running statistics untouched; the encoders in eval mode against the
fp64 oracle."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    bn.num_batches_tracked.fill_(7)
    return bn.eval()


@pytest.mark.parametrize("N,C,H,W", [(2, 8, 16, 20), (3, 5, 7, 9), (1, 64, 3, 5), (4, 16, 6, 20), (2, 3, 1, 1)])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (True, False), (False, False)])
def test_bn_eval_forward_and_gradients_vs_fp64(N, C, H, W, res, relu):
    from depthcore import ops
    bn = _bn(C, N * 100 + C)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, C, H, W, generator=g)
    r = torch.randn(N, C, H, W, generator=g) if res else None
    cot = torch.randn(N, C, H, W, generator=g)
    bnd = bn.to(DEV)
    before = {k: v.clone() for k, v in bnd.state_dict().items()}
    xd = x.to(DEV).requires_grad_()
    rd = r.to(DEV).requires_grad_() if res else None
    y = ops.bn_eval(xd, bnd, rd, relu)
    grads = torch.autograd.grad((y * cot.to(DEV)).sum(), [xd, bnd.weight, bnd.bias] + ([rd] if res else []))
    for k, v in bnd.state_dict().items():                    # running statistics and num_batches_tracked: bitwise untouched
        assert torch.equal(v, before[k]), k
    # fp64 oracle
    x64 = x.double().requires_grad_()
    r64 = r.double().requires_grad_() if res else None
    w64 = bn.weight.detach().cpu().double().requires_grad_()
    b64 = bn.bias.detach().cpu().double().requires_grad_()
    y64 = F.batch_norm(x64, bn.running_mean.cpu().double(), bn.running_var.cpu().double(), w64, b64, False, 0.1, bn.eps)
    if res:
        y64 = y64 + r64
    if relu:
        y64 = F.relu(y64)
    want = torch.autograd.grad((y64 * cot.double()).sum(), [x64, w64, b64] + ([r64] if res else []))
    assert rel_l2(y, y64) < 2e-6
    for gg, ww in zip(grads, want):
        assert rel_l2(gg, ww) < 1e-5, (rel_l2(gg, ww))


def test_bn_eval_refuses_batch_statistics():
    from depthcore import ops
    from depthcore._lib import DepthcoreError
    bn = nn.BatchNorm2d(4, track_running_stats=False).to(DEV).eval()
    with pytest.raises(DepthcoreError):
        ops.bn_eval(torch.randn(2, 4, 4, 4, device=DEV), bn)


@pytest.mark.parametrize("num_layers,B,H,W", [(18, 2, 64, 128), (50, 2, 64, 96), (18, 1, 70, 102)])
def test_encoder_eval_forward_vs_fp64_oracle(num_layers, B, H, W):
    import networks
    from oracle.resnet_ref import resnet_encoder_forward
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(num_layers, False).to(DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, nn.BatchNorm2d):
                C = m.num_features
                m.weight.copy_((0.5 + torch.rand(C, generator=g)).to(DEV))
                m.bias.copy_((0.1 * torch.randn(C, generator=g)).to(DEV))
                m.running_mean.copy_((0.1 * torch.randn(C, generator=g)).to(DEV))
                m.running_var.copy_((0.5 + torch.rand(C, generator=g)).to(DEV))
    enc.eval()
    state = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    x = torch.rand(B, 3, H, W, generator=g)
    with torch.no_grad():
        got = enc(x.to(DEV))
    assert all(torch.equal(v, state[k].to(DEV)) for k, v in enc.state_dict().items())
    st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    st32 = {k: (v.float() if v.is_floating_point() else v) for k, v in state.items()}
    f64 = resnet_encoder_forward(st64, x.double(), num_layers, training=False)
    f32 = resnet_encoder_forward(st32, x, num_layers, training=False)
    for i in range(5):
        e, e32 = rel_l2(got[i], f64[i]), rel_l2(f32[i], f64[i])
        assert e <= max(2.0 * e32, 2.5e-5), (i, e, e32)
