"""CPU checks of the residual-join plumbing: the staged forward that threads
a block-output pair through each stage, and the aliased-pair autograd
pattern the fused join relies on."""
import os

import pytest
import torch

from dwt_amd.models import Bottleneck, ResNetDWT

GOLDEN_KEYS = os.path.join(os.path.dirname(__file__), "golden",
                           "resnet_dwt_state_keys_2111.txt")


def _model():
    torch.manual_seed(0)
    return ResNetDWT(Bottleneck, [2, 1, 1, 1], None, num_classes=5) \
        .double().train()


def _block_forward_unfused(blk, x):
    """The bottleneck as it was before the join: norm3 without ReLU, then the
    downsample branch, then add_relu(out, identity)."""
    from dwt_amd.models.sites import norm_site
    from dwt_amd.ops.functional import add_relu
    tr = blk.training
    identity = x
    out = blk.conv1(x)
    out = norm_site(out, [blk.bns1, blk.bnt1, blk.bnt1_aug],
                    blk.gamma1, blk.beta1, training=tr, relu=True)
    out = blk.conv2(out)
    out = norm_site(out, [blk.bns2, blk.bnt2, blk.bnt2_aug],
                    blk.gamma2, blk.beta2, training=tr, relu=True)
    out = blk.conv3(out)
    out = norm_site(out, [blk.bns3, blk.bnt3, blk.bnt3_aug],
                    blk.gamma3, blk.beta3, training=tr, relu=False)
    if blk.downsample is not None:
        identity = blk.downsample(x)
        identity = norm_site(
            identity,
            [blk.downsample_bns, blk.downsample_bnt, blk.downsample_bnt_aug],
            blk.downsample_gamma, blk.downsample_beta, training=tr, relu=False)
    return add_relu(out, identity)


def _plain_forward(model, x, block_forward):
    """The model with each block run tensor -> tensor in sequence."""
    from dwt_amd.models.sites import norm_site
    from dwt_amd.ops.pooling import global_avg_pool
    x = model.conv1(x)
    x = norm_site(x, [model.bns1, model.bnt1, model.bnt1_aug], model.gamma1,
                  model.beta1, training=model.training, relu=True)
    x = model.maxpool(x)
    for stage in (model.layer1, model.layer2, model.layer3, model.layer4):
        for i in range(len(stage)):
            x = block_forward(stage[i], x)
    return model.fc_out(global_avg_pool(x))


@pytest.mark.parametrize("block_forward", [
    lambda blk, x: blk.forward(x),   # each block's plain forward
    _block_forward_unfused,          # the composition from before the join
], ids=["block_forward", "unfused_composition"])
def test_staged_forward_matches_blockwise(block_forward):
    torch.manual_seed(1)
    x = torch.randn(6, 3, 32, 32, dtype=torch.float64)
    w = torch.randn(6, 5, dtype=torch.float64)

    m1, m2 = _model(), _model()
    out1 = m1(x)
    (out1 * w).sum().backward()
    out2 = _plain_forward(m2, x, block_forward)
    (out2 * w).sum().backward()

    assert torch.allclose(out1, out2, rtol=1e-9, atol=0)
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert n1 == n2
        assert p1.grad is not None, n1
        assert torch.allclose(p1.grad, p2.grad, rtol=1e-9, atol=0), n1
    for (n1, b1), (n2, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.allclose(b1, b2, rtol=1e-9, atol=0), n1


def test_state_dict_keys_unchanged():
    with open(GOLDEN_KEYS) as f:
        want = f.read().split()
    assert list(_model().state_dict().keys()) == want


def test_stage_indexing():
    m = _model()
    assert isinstance(m.layer1[1], Bottleneck)
    assert len(m.layer1) == 2 and len(m.layer4) == 1


def test_bottleneck_forward_is_pair_element():
    torch.manual_seed(2)
    blk = _model().layer1[1]
    x = torch.randn(6, 256, 4, 4, dtype=torch.float64)
    y = blk(x)
    ya, yb = blk.forward_pair(x, x)
    assert isinstance(y, torch.Tensor)
    assert torch.equal(ya, yb)
    assert torch.allclose(y, ya, rtol=1e-12)


def test_unused_alias_gets_none_grad():
    """Two outputs aliasing one buffer with set_materialize_grads(False):
    backward sees the consumers' gradients un-summed, None for an unused one."""
    seen = []

    class Pair(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            ctx.set_materialize_grads(False)
            y = a * 2
            return y, y.view_as(y)

        @staticmethod
        def backward(ctx, g1, g2):
            seen.append((g1, g2))
            g = g1 if g2 is None else g2 if g1 is None else g1 + g2
            return g * 2

    a = torch.randn(4, dtype=torch.float64, requires_grad=True)
    p, q = Pair.apply(a)
    assert p.data_ptr() == q.data_ptr()
    (q * 3).sum().backward()
    assert seen[-1][0] is None and torch.equal(seen[-1][1], torch.full((4,), 3.0, dtype=torch.float64))
    assert torch.equal(a.grad, torch.full((4,), 6.0, dtype=torch.float64))

    a.grad = None
    p, q = Pair.apply(a)
    (p.sum() + (q * 3).sum()).backward()
    g1, g2 = seen[-1]
    assert torch.equal(g1, torch.ones(4, dtype=torch.float64))
    assert torch.equal(g2, torch.full((4,), 3.0, dtype=torch.float64))
    assert torch.equal(a.grad, torch.full((4,), 8.0, dtype=torch.float64))
