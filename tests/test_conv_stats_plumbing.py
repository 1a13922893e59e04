"""CPU checks of the conv-epilogue statistics plumbing: the switch changes
nothing where the kernel cannot run, the accumulator layout reference matches
the statistics ops/functional.py computes, and sites ignore an accumulator
they cannot use."""
import pytest
import torch

from dwt_amd.models import Bottleneck, ResNetDWT
from dwt_amd.models.sites import norm_site
from dwt_amd.ops import oracle
from dwt_amd.ops.batch_norm import DomainBatchNorm2d
from dwt_amd.ops.mfma import (conv1x1_routed, conv1x1_stats, conv_stats_route,
                              stats_acc_numel)
from dwt_amd.ops.oracle import stats_acc_reference
from dwt_amd.ops.whitening import WhiteningScaleShift

PARTS = 3
G = 4


def _model_step(on, monkeypatch):
    monkeypatch.setenv("DWT_AMD_FUSED_CONV_STATS", "1" if on else "0")
    torch.manual_seed(3)
    model = ResNetDWT(Bottleneck, [1, 1, 1, 1], None, num_classes=5).train()
    data = torch.randn(6, 3, 32, 32)
    out = model(data)
    out.square().sum().backward()
    grads = [p.grad.clone() for p in model.parameters()]
    return out.detach(), grads


def test_switch_is_inert_on_cpu(monkeypatch):
    out_on, g_on = _model_step(True, monkeypatch)
    out_off, g_off = _model_step(False, monkeypatch)
    assert torch.equal(out_on, out_off)
    assert len(g_on) == len(g_off)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)


def test_route_and_wrapper_fall_back_on_cpu():
    conv = torch.nn.Conv2d(64, 64, 1, bias=False)
    x = torch.randn(PARTS * 2, 64, 8, 8).contiguous(
        memory_format=torch.channels_last)
    branches = [DomainBatchNorm2d(64, affine=False) for _ in range(PARTS)]
    assert conv_stats_route(conv, x, branches, True) is None
    out, acc = conv1x1_routed(conv, x, branches, True)
    assert acc is None
    assert torch.equal(out, conv(x))
    # the module's own forward: no routing Function on the graph
    assert "Conv1x1Fn" not in type(out.grad_fn).__name__
    out, acc = conv1x1_stats(x, conv.weight, "bn", G, PARTS)
    assert acc is None
    assert torch.equal(out, conv(x))


def test_routing_predicate_matches_committed_table():
    """conv_stats_shape_ok routes exactly the rows of
    profiles/conv_stats_bench_b1536.md that gain more than 5%."""
    import os
    from dwt_amd.ops.mfma import conv_stats_shape_ok
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "conv_stats_bench_b1536.md")
    rows = 0
    with open(path) as f:
        for line in f:
            cells = [c.strip() for c in line.strip().strip("|").split("|")]
            if len(cells) != 10 or "x" not in cells[1] \
                    or not cells[1][0].isdigit():
                continue
            m, cout, cin = (int(v) for v in cells[1].split("x"))
            gain = float(cells[7].rstrip("x"))
            routed = conv_stats_shape_ok(m, cin, cout)
            assert routed == (gain > 1.05), (cells[0], gain, routed)
            assert cells[9] == ("yes" if routed else "no"), cells[0]
            rows += 1
    assert rows == 12


def _x(c, b=4, h=5, w=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(PARTS * b, c, h, w, generator=gen, dtype=torch.float64)
    x[b:2 * b] += 1.5
    x[2 * b:] *= 3.0
    return x, b


def test_acc_reference_matches_bn_statistics():
    c = 16
    x, b = _x(c)
    acc = stats_acc_reference(x, "bn", PARTS)
    assert acc.numel() == stats_acc_numel("bn", c, PARTS)
    acc = acc.reshape(PARTS, 2, c)
    n = b * x.shape[2] * x.shape[3]
    for p in range(PARTS):
        xp = x[p * b:(p + 1) * b]
        mean = acc[p, 0] / n
        var = acc[p, 1] / n - mean * mean
        assert torch.allclose(mean, xp.mean(dim=(0, 2, 3)), atol=1e-12)
        assert torch.allclose(var, xp.var(dim=(0, 2, 3), unbiased=False),
                              atol=1e-10)


def test_acc_reference_matches_whitening_statistics():
    c = 16
    ng = c // G
    x, b = _x(c, seed=1)
    acc = stats_acc_reference(x, "whiten", PARTS, G)
    assert acc.numel() == stats_acc_numel("whiten", c, PARTS, G)
    acc = acc.reshape(PARTS, ng, G + G * G)
    n = b * x.shape[2] * x.shape[3]
    for p in range(PARTS):
        xp = x[p * b:(p + 1) * b]
        m = xp.mean(dim=(0, 2, 3))
        cov = oracle.grouped_cov(xp - m.view(1, c, 1, 1), ng)
        mean = acc[p, :, :G] / n
        low = acc[p, :, G:].reshape(ng, G, G)
        # only j <= i is stored; the finalize kernel mirrors it
        assert torch.equal(low, torch.tril(low))
        full = low + torch.tril(low, -1).transpose(1, 2)
        got = full / n - mean.unsqueeze(2) * mean.unsqueeze(1)
        assert torch.allclose(mean.reshape(-1), m, atol=1e-12)
        assert torch.allclose(got, cov, atol=1e-10)


@pytest.mark.parametrize("kind", ["bn", "whiten"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_norm_site_ignores_acc_it_cannot_use(kind, training):
    """Eval mode never reads batch statistics; the CPU path has no use for
    the accumulator in training either.  Garbage must change nothing."""
    c = 16
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(PARTS * 2, c, 4, 4, generator=gen)
    gamma = torch.randn(c, 1, 1, generator=gen)
    beta = torch.randn(c, 1, 1, generator=gen)

    def run(acc):
        torch.manual_seed(0)
        if kind == "bn":
            br = [DomainBatchNorm2d(c, affine=False) for _ in range(PARTS)]
        else:
            br = [WhiteningScaleShift(c, G, affine=False) for _ in range(PARTS)]
        return norm_site(x, br, gamma, beta, training=training, relu=True,
                         stats_acc=acc)

    garbage = torch.full((stats_acc_numel(kind, c, PARTS),), float("nan"))
    assert torch.equal(run(garbage), run(None))
