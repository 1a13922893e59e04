"""GPU numerics of the 1x1 conv forward that accumulates the next norm site's
raw statistics in its epilogue (dwt_amd.ops.mfma.conv1x1_stats), and of the
norm sites consuming that accumulator.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PARTS = 3
G = 4
# (Cin, Cout, b, h, w) per branch:
#   one tile per branch, Cout below the 128 tile / two M-tiles per branch and
#   two N-tiles / K = 256, the pipelined instantiation / unaligned (fallback)
ALIGNED = [(64, 64, 2, 8, 8), (64, 256, 4, 8, 8), (256, 128, 2, 8, 8)]
# the two instantiations the layer-2 block below (and the flagship's layer 2)
# runs: K = 128, two k-steps of the non-pipelined loop with four N-tiles, and
# K = 512, eight k-steps of the pipelined one
LAYER2 = [(128, 512, 2, 8, 8), (512, 128, 2, 8, 8)]
UNALIGNED = (64, 64, 2, 3, 3)
KINDS = ["bn", "whiten"]
# 1 workgroup crosses both branch boundaries (and, with two N-tiles, walks
# both); 2 splits the M-tiles in runs that cross one boundary each
MAX_WGS = [0, 1, 2]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dwt_amd.kernels import dispatch
    assert dispatch.available(), "HIP extension must be built+loaded on a GPU box"
    return torch.device("cuda:0")


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() /
            b.float().abs().max().clamp_min(1e-6)).item()


def _maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    """(x, weight, F.conv2d reference), built once per shape.  Each branch's
    input has its own offset and scale, so rows credited to the wrong branch
    show up in the sums."""
    cin, cout, b, h, w = shape
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(100 + cin + cout + h)
    x = torch.randn(PARTS * b, cin, h, w, generator=gen)
    x[b:2 * b] += 1.5
    x[2 * b:] *= 3.0
    x = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 1, 1, generator=gen) * cin ** -0.5) \
        .to(dev).to(torch.bfloat16)
    ref = F.conv2d(x, wt)
    return x, wt, ref


@functools.lru_cache(maxsize=None)
def _fused(shape, kind, max_wg):
    from dwt_amd.ops.mfma import conv1x1_stats
    x, wt, _ = _conv_case(shape)
    out, acc = conv1x1_stats(x, wt, kind, G, PARTS, max_workgroups=max_wg)
    torch.cuda.synchronize()
    return out, acc


@pytest.mark.parametrize("max_wg", MAX_WGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALIGNED + LAYER2, ids=str)
def test_conv_out_and_acc(dev, shape, kind, max_wg):
    from dwt_amd.ops.mfma import stats_acc_numel
    from dwt_amd.ops.oracle import stats_acc_reference
    cin, cout, b, h, w = shape
    _, _, ref = _conv_case(shape)
    out, acc = _fused(shape, kind, max_wg)
    assert acc is not None and not acc.requires_grad
    assert out.is_contiguous(memory_format=torch.channels_last)
    err = _rel_err(out, ref)
    print(f"{shape} {kind} wg={max_wg}: out rel err {err:.3g}")
    assert err < 0.05, err
    # the GEMM does not depend on how the tiles are dealt to workgroups
    assert torch.equal(out, _fused(shape, kind, 0)[0])

    # statistics of the STORED bf16 values, fp64 reference; bound: fp32
    # summation of n terms, (n-1) * 2^-24 * sum|terms|, doubled for the
    # two-level (lane partial -> workgroup -> global) reduction
    assert acc.numel() == stats_acc_numel(kind, cout, PARTS, G)
    want = stats_acc_reference(out, kind, PARTS, G)
    mag = stats_acc_reference(out.abs(), kind, PARTS, G)
    n = b * h * w
    bound = 2.0 * (n - 1) * 2.0 ** -24 * mag
    diff = (acc.double() - want).abs()
    worst = (diff - bound).max().item()
    print(f"  acc: max diff {diff.max().item():.3g}, "
          f"max diff/bound {(diff / bound.clamp_min(1e-300)).max().item():.3g}")
    assert worst <= 0.0, (diff.max().item(), worst)


@pytest.mark.parametrize("kind", KINDS)
def test_unaligned_falls_back(dev, kind):
    """b*h*w = 18 rows per branch: no multiple of the 128-row tile."""
    from dwt_amd.ops.mfma import _Conv1x1Fn, conv1x1_stats
    x, wt, ref = _conv_case(UNALIGNED)
    before = _Conv1x1Fn.stats_calls
    out, acc = conv1x1_stats(x, wt, kind, G, PARTS)
    assert _Conv1x1Fn.stats_calls == before
    assert acc is None
    assert _rel_err(out, ref) < 0.05
    # the site behind it computes its own statistics
    cout = UNALIGNED[1]
    gamma, beta = _affine(cout, dev, torch.bfloat16)
    y = _site(kind, out, _branches(kind, cout, dev), gamma, beta, acc)
    y_ref = _site(kind, ref, _branches(kind, cout, dev), gamma, beta, None)
    assert torch.allclose(y.float(), y_ref.float(), atol=0.1, rtol=0.05)


# ---------------------------------------------------------------------------
# norm sites fed with the accumulator
# ---------------------------------------------------------------------------

def _branches(kind, c, dev):
    from dwt_amd.ops.batch_norm import DomainBatchNorm2d
    from dwt_amd.ops.whitening import WhiteningScaleShift
    if kind == "bn":
        mods = [DomainBatchNorm2d(c, affine=False) for _ in range(PARTS)]
    else:
        mods = [WhiteningScaleShift(c, G, affine=False, mode="zca")
                for _ in range(PARTS)]
    return [m.to(dev) for m in mods]


def _affine(c, dev, dtype, seed=7):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    gamma = (torch.randn(c, 1, 1, generator=gen) * 0.5 + 1.0).to(dev).to(dtype)
    beta = (torch.randn(c, 1, 1, generator=gen) * 0.5).to(dev).to(dtype)
    return gamma, beta


def _site(kind, x, branches, gamma, beta, acc, residual=None):
    from dwt_amd.models.sites import norm_site
    return norm_site(x, branches, gamma, beta, training=True, relu=True,
                     residual=residual, stats_acc=acc)


def _buffers_of(kind, branches):
    if kind == "bn":
        return [b.running_mean for b in branches] + \
            [b.running_var for b in branches]
    return [b.wh.running_mean for b in branches] + \
        [b.wh.running_variance for b in branches]


def _run_site(kind, x, acc, join, dev, seed):
    c = x.shape[1]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    wa = torch.randn(x.shape, generator=gen).to(dev)
    wb = torch.randn(x.shape, generator=gen).to(dev)
    idn = torch.randn(x.shape, generator=gen).to(dev).to(x.dtype) \
        .contiguous(memory_format=torch.channels_last)
    gamma, beta = _affine(c, dev, x.dtype)
    x, idn, gamma, beta = (t.clone().requires_grad_(True)
                           for t in (x, idn, gamma, beta))
    branches = _branches(kind, c, dev)
    if join:
        ya, yb = _site(kind, x, branches, gamma, beta, acc, residual=idn)
    else:
        ya = yb = _site(kind, x, branches, gamma, beta, acc)
    loss = (ya.float() * wa).sum() + 0.5 * (yb.float() ** 2 * wb).sum()
    loss.backward()
    res = dict(y=ya.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    if join:
        res["did"] = idn.grad
    return res, _buffers_of(kind, branches)


# tests/test_gpu_join.py, fused against unfused: the fp32 tolerances of
# test_join_parity_fp32 (out, dx / d_identity, dgamma / dbeta) and the bf16
# ones of test_join_bf16_no_worse_than_unfused ((atol, rtol) for y, grads)
FP32_TOLS = {"bn": (1e-4, 1e-3, 1e-2), "whiten": (3e-4, 2e-3, 3e-2)}
BF16_TOLS = ((0.1, 0.05), (0.2, 0.1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("join", [False, True], ids=["plain", "join"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALIGNED, ids=str)
def test_norm_site_with_acc(dev, shape, kind, join, dtype):
    """norm_site(conv_out, stats_acc=acc) against norm_site(conv_out) on the
    same conv_out.  bf16 is the path the model runs; the fp32 copy of the same
    conv_out isolates the statistics (no output rounding) at the fp32
    tolerances."""
    out, acc = _fused(shape, kind, 0)
    x = out.to(dtype).contiguous(memory_format=torch.channels_last)
    got, bufs_g = _run_site(kind, x, acc.clone(), join, dev, seed=11)
    want, bufs_w = _run_site(kind, x, None, join, dev, seed=11)
    for k in got:
        print(f"{shape} {kind} join={join} {dtype} {k}: "
              f"{_maxerr(got[k], want[k]):.3g}")
    if dtype == torch.float32:
        t_out, t_dx, t_p = FP32_TOLS[kind]
        tol = dict(y=t_out, dx=t_dx, did=t_dx, dgamma=t_p, dbeta=t_p)
        for k in got:
            assert torch.allclose(got[k], want[k], atol=tol[k]), \
                (k, _maxerr(got[k], want[k]))
    else:
        for k in got:
            atol, rtol = BF16_TOLS[0] if k == "y" else BF16_TOLS[1]
            assert torch.allclose(got[k].float(), want[k].float(), atol=atol,
                                  rtol=rtol), (k, _maxerr(got[k], want[k]))
    for a, b in zip(bufs_g, bufs_w):
        assert torch.allclose(a, b, atol=1e-4), _maxerr(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_norm_site_consumes_acc(dev, kind):
    """A deliberately wrong accumulator changes the result: the site really
    reads it instead of recomputing."""
    shape = ALIGNED[0]
    out, acc = _fused(shape, kind, 0)
    c = shape[1]
    gamma, beta = _affine(c, dev, torch.bfloat16)
    y = _site(kind, out, _branches(kind, c, dev), gamma, beta, acc.clone())
    y_bad = _site(kind, out, _branches(kind, c, dev), gamma, beta,
                  acc * 4.0 + 1.0)
    assert not torch.allclose(y.float(), y_bad.float(), atol=0.1, rtol=0.05)


# ---------------------------------------------------------------------------
# bottleneck blocks, switch on / off
# ---------------------------------------------------------------------------

def _block(style, dev):
    from dwt_amd.models.resnet_dwt import Bottleneck, conv1x1
    torch.manual_seed(5)
    if style == "layer1":
        ds = nn.Sequential(conv1x1(64, 256))
        blk = Bottleneck(64, 64, 1, 0, None, G, 1, ds, whiten_mode="zca")
        cin = 64
    else:
        blk = Bottleneck(512, 128, 2, 1, None, G)
        cin = 512
    blk = blk.to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).train()
    gen = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(PARTS * 2, cin, 8, 8, generator=gen).to(dev) \
        .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wl = torch.randn(PARTS * 2, blk.conv3.out_channels, 8, 8,
                     generator=gen).to(dev)
    return blk, x, wl


def _block_step(blk, x, wl, on, monkeypatch):
    """One forward and backward of L = sum(wl * y^2) / 2.

    The loss is quadratic on purpose.  The block ends in a ReLU, and its
    output gradient reaches dx undiluted through the identity.  Two correct
    runs differ in the last bits (atomic order of the statistics, the conv's
    accumulation order), which now and then moves an exit pre-activation
    across zero.  With a linear loss that element's gradient jumps from wl to
    0, a change of the size of max|dx| itself: measured over 12 seeds, the
    switch-off path compared with ITSELF reached 0.29 in dx and on against
    off 0.42 (dx) and 0.15 (conv3.weight), always together with flipped exit
    masks, so the max-norm criterion measured the ReLU and not the code.
    dL/dy = wl * y vanishes where y does, so a flipped exit mask changes the
    gradients continuously and the criterion sees the code again: with this
    loss, 60 repeated steps on this test's own data (30 off, 30 on, each
    against the first off step) stayed within 0.0058 in every compared
    quantity for both blocks, and dx within 0.012 over 24 other seeds with up
    to 15 flipped exit masks.  The two inner ReLUs cannot be treated the same
    way from outside the block: in that sweep a flipped inner mask moved
    conv2.weight by 0.045 and 0.073 in 2 of the 24 layer-2 seeds (on against
    off; none on this test's data)."""
    monkeypatch.setenv("DWT_AMD_FUSED_CONV_STATS", "1" if on else "0")
    blk.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True)
    y = blk(xin)
    (0.5 * y.float() ** 2 * wl).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    return y.detach(), xin.grad, grads


@pytest.mark.parametrize("style", ["layer1", "layer2"])
def test_bottleneck_switch(dev, style, monkeypatch):
    from dwt_amd.ops import mfma
    blk, x, wl = _block(style, dev)
    # the shape table (measured at N = 1536) keeps layer 1's shapes on the
    # old path; this test is about the wiring, so every eligible conv routes:
    # conv1, conv3 and, in the layer-1 block, the stride-1 downsample conv
    monkeypatch.setattr(mfma, "conv_stats_shape_ok", lambda m, cin, cout: True)
    expect = 3 if style == "layer1" else 2

    before = mfma._Conv1x1Fn.stats_calls
    y_off, dx_off, g_off = _block_step(blk, x, wl, False, monkeypatch)
    assert mfma._Conv1x1Fn.stats_calls == before
    y_on, dx_on, g_on = _block_step(blk, x, wl, True, monkeypatch)
    assert mfma._Conv1x1Fn.stats_calls == before + expect  # no silent fallback

    print(f"{style}: y {_rel_err(y_on, y_off):.3g} dx {_rel_err(dx_on, dx_off):.3g}")
    assert _rel_err(y_on, y_off) < 0.05
    assert _rel_err(dx_on, dx_off) < 0.05
    assert set(g_on) == set(g_off)
    for name in g_off:
        err = _rel_err(g_on[name], g_off[name])
        print(f"  {name}: {err:.3g}")
        assert err < 0.05, (name, err)
