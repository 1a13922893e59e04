"""The direct-to-LDS main loop of the dense MFMA kernels (conv1x1_stats, the
1x1 dgrad / forward and mfma_gemm) against the register-staged loop it
replaces: the MFMA sequence per accumulator is the same, so the outputs must
be EQUAL bit for bit, and the loop's staging must not race (a race shows as a
rare wrong tile, hence the repeated launches).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PARTS = 3
G = 4
# (Cin, Cout, b, h, w) per branch:
#   one k-step (the prologue is the whole loop) / two k-steps, two N-tiles /
#   three k-steps (odd: the buffer parity flips from tile to tile), three
#   M-tiles per branch / eight k-steps
STATS_SHAPES = [(64, 128, 2, 8, 8), (128, 256, 2, 8, 8), (192, 128, 6, 8, 8),
                (512, 256, 4, 8, 8)]
KINDS = ["bn", "whiten"]
# 1: one workgroup walks every tile of every N-tile, so each cross-tile and
# cross-N-tile prefetch is exercised; 2: two runs or two N lanes
MAX_WGS = [0, 1, 2]
REPEATS = 10

# dense GEMM: M = 245 (5x7x7, a partial last tile), one and a half / three
# tiles; K of one, three, eight k-steps; N below one tile, one tile, a
# partial third
GEMM_M = [(5, 7, 7), (4, 8, 8), (6, 8, 8)]      # (n, h, w): 245, 256, 384
GEMM_K = [64, 192, 512]
GEMM_N = [64, 128, 320]
SENTINEL = -7.0
PAD_ROWS = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dwt_amd.kernels import dispatch
    assert dispatch.available(), "HIP extension must be built+loaded on a GPU box"
    return torch.device("cuda:0")


@pytest.fixture()
def ext(dev):
    """The extension, with the loop switch restored afterwards."""
    from dwt_amd.kernels import dispatch
    e = dispatch.ext()
    was = e.dense_glds_selected()
    yield e
    e.set_dense_glds(was)


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() /
            b.float().abs().max().clamp_min(1e-6)).item()


@functools.lru_cache(maxsize=None)
def _stats_case(shape):
    cin, cout, b, h, w = shape
    gen = torch.Generator(device="cpu").manual_seed(300 + cin + cout + b)
    x = torch.randn(PARTS * b, cin, h, w, generator=gen)
    x[b:2 * b] += 1.5
    x[2 * b:] *= 3.0
    x = x.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, 1, 1, generator=gen) * cin ** -0.5) \
        .cuda().to(torch.bfloat16)
    return x, wt


@functools.lru_cache(maxsize=None)
def _stats_old(shape, kind):
    """Output of the register-staged loop (max_workgroups = 0), once."""
    from dwt_amd.kernels import dispatch
    from dwt_amd.ops.mfma import conv1x1_stats
    e = dispatch.ext()
    was = e.dense_glds_selected()
    e.set_dense_glds(False)
    try:
        x, wt = _stats_case(shape)
        n0 = e.dense_glds_launches()
        out, _ = conv1x1_stats(x, wt, kind, G, PARTS)
        assert e.dense_glds_launches() == n0, "the switch did not select the old loop"
        torch.cuda.synchronize()
    finally:
        e.set_dense_glds(was)
    return out


@pytest.mark.parametrize("max_wg", MAX_WGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", STATS_SHAPES, ids=str)
def test_stats_new_loop_equals_old(ext, shape, kind, max_wg):
    from dwt_amd.ops.mfma import conv1x1_stats
    from dwt_amd.ops.oracle import stats_acc_reference
    cin, cout, b, h, w = shape
    x, wt = _stats_case(shape)
    old = _stats_old(shape, kind)
    ext.set_dense_glds(True)
    n0 = ext.dense_glds_launches()
    runs = [conv1x1_stats(x, wt, kind, G, PARTS, max_workgroups=max_wg)
            for _ in range(REPEATS)]
    torch.cuda.synchronize()
    assert ext.dense_glds_launches() == n0 + REPEATS, "new loop not taken"
    bad = [i for i, (out, _) in enumerate(runs) if not torch.equal(out, old)]
    assert not bad, f"launches {bad} of {REPEATS} differ from the old loop"

    # the accumulator: the bound of test_gpu_conv_stats.test_conv_out_and_acc
    # (fp32 summation of n terms, doubled for the two-level reduction)
    want = stats_acc_reference(old, kind, PARTS, G)
    mag = stats_acc_reference(old.abs(), kind, PARTS, G)
    n = b * h * w
    bound = 2.0 * (n - 1) * 2.0 ** -24 * mag
    for _, acc in runs:
        diff = (acc.double() - want).abs()
        worst = (diff - bound).max().item()
        assert worst <= 0.0, (diff.max().item(), worst)


@functools.lru_cache(maxsize=None)
def _gemm_case(nhw, k, n):
    """dy (nb, k, h, w) channels_last = A[M, k]; weight (k, n, 1, 1) of the
    conv whose dgrad is A @ W, i.e. Bt = W^T (n, k)."""
    nb, h, w = nhw
    gen = torch.Generator(device="cpu").manual_seed(500 + nb * h * w + k + n)
    dy = torch.randn(nb, k, h, w, generator=gen).cuda().to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(k, n, 1, 1, generator=gen) * k ** -0.5) \
        .cuda().to(torch.bfloat16)
    return dy, wt


def _sentinel_out(m, n):
    buf = torch.full((m + 2 * PAD_ROWS, n), SENTINEL, device="cuda",
                     dtype=torch.bfloat16)
    return buf, buf[PAD_ROWS:PAD_ROWS + m]


def _check_sentinels(buf, m):
    assert (buf[:PAD_ROWS] == SENTINEL).all(), "rows before the output written"
    assert (buf[PAD_ROWS + m:] == SENTINEL).all(), "rows after the output written"


@pytest.mark.parametrize("n", GEMM_N)
@pytest.mark.parametrize("k", GEMM_K)
@pytest.mark.parametrize("nhw", GEMM_M, ids=str)
def test_dense_gemm_and_dgrad(ext, nhw, k, n):
    nb, h, w = nhw
    m = nb * h * w
    dy, wt = _gemm_case(nhw, k, n)
    a = dy.permute(0, 2, 3, 1).reshape(m, k)           # the NHWC storage
    bt = wt.reshape(k, n).t().contiguous()             # (n, k)
    empty = torch.empty(0, device="cuda")
    assert (PAD_ROWS * n * 2) % 16 == 0                # the view stays 16-B aligned

    res = {}
    for glds in (False, True):
        ext.set_dense_glds(glds)
        n0 = ext.dense_glds_launches()
        gbuf, gout = _sentinel_out(m, n)
        ext.mfma_gemm(a, bt, empty, gout, False, False)
        dbuf, dout = _sentinel_out(m, n)
        ext.mfma_conv2d_dgrad(dy, bt, dout, nb, h, w, n, h, w, k, 1, 1, 1, 0)
        torch.cuda.synchronize()
        assert ext.dense_glds_launches() - n0 == (2 if glds else 0)
        _check_sentinels(gbuf, m)
        _check_sentinels(dbuf, m)
        res[glds] = (gout.clone(), dout.clone())
    assert torch.equal(res[True][0], res[False][0]), "mfma_gemm: new != old loop"
    assert torch.equal(res[True][1], res[False][1]), "dgrad: new != old loop"
    assert torch.equal(res[True][0], res[True][1])

    ref = (a.float() @ bt.float().t()).to(torch.bfloat16)
    assert _rel_err(res[True][0], ref) < 0.05
    x = torch.empty(nb, n, h, w, device="cuda", dtype=torch.bfloat16,
                    memory_format=torch.channels_last)
    dx_ref, _, _ = torch.ops.aten.convolution_backward(
        dy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
        [True, False, False])
    dx = res[True][1].reshape(nb, h, w, n).permute(0, 3, 1, 2)
    assert _rel_err(dx, dx_ref) < 0.05


def test_dense_gemm_bias_relu_equal(ext):
    """The 16-byte-store epilogue keeps the optional bias and ReLU."""
    from dwt_amd.ops.mfma import mfma_gemm
    gen = torch.Generator(device="cpu").manual_seed(9)
    a = torch.randn(200, 128, generator=gen).cuda().to(torch.bfloat16)
    bt = torch.randn(72, 128, generator=gen).cuda().to(torch.bfloat16)
    bias = torch.randn(72, generator=gen).cuda()
    ext.set_dense_glds(False)
    old = mfma_gemm(a, bt, bias=bias, relu=True)
    ext.set_dense_glds(True)
    n0 = ext.dense_glds_launches()
    new = mfma_gemm(a, bt, bias=bias, relu=True)
    assert ext.dense_glds_launches() == n0 + 1
    assert torch.equal(new, old)
    ref = torch.relu(a.float() @ bt.float().t() + bias).to(torch.bfloat16)
    assert _rel_err(new, ref) < 0.05


def test_k72_takes_old_loop(ext):
    """K = 72 is no whole number of 64-deep k-steps and an LDS-DMA load cannot
    zero-fill, so the register-staged loop runs whatever the switch says."""
    from dwt_amd.ops.mfma import conv1x1_stats, mfma_gemm
    ext.set_dense_glds(True)
    gen = torch.Generator(device="cpu").manual_seed(10)
    a = torch.randn(245, 72, generator=gen).cuda().to(torch.bfloat16)
    bt = torch.randn(128, 72, generator=gen).cuda().to(torch.bfloat16)
    n0 = ext.dense_glds_launches()
    out = mfma_gemm(a, bt)
    x = torch.randn(PARTS * 2, 72, 8, 8, generator=gen).cuda().to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(128, 72, 1, 1, generator=gen) * 72 ** -0.5) \
        .cuda().to(torch.bfloat16)
    y, acc = conv1x1_stats(x, wt, "bn", G, PARTS)
    torch.cuda.synchronize()
    assert ext.dense_glds_launches() == n0
    assert acc is not None
    assert _rel_err(out, (a.float() @ bt.float().t()).to(torch.bfloat16)) < 0.05
    assert _rel_err(y, F.conv2d(x, wt)) < 0.05


# ---------------------------------------------------------------------------
# routing: bottleneck blocks with every eligible pass on the dense kernel
# ---------------------------------------------------------------------------

def _block(style):
    import torch.nn as nn
    from dwt_amd.models.resnet_dwt import Bottleneck, conv1x1
    torch.manual_seed(5)
    if style == "layer1":
        ds = nn.Sequential(conv1x1(64, 256))
        blk = Bottleneck(64, 64, 1, 0, None, G, 1, ds, whiten_mode="zca")
        cin = 64
    else:
        blk = Bottleneck(512, 128, 2, 1, None, G)
        cin = 512
    blk = blk.cuda().to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).train()
    gen = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(PARTS * 2, cin, 8, 8, generator=gen).cuda() \
        .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wl = torch.randn(PARTS * 2, blk.conv3.out_channels, 8, 8,
                     generator=gen).cuda()
    return blk, x, wl


def _block_step(blk, x, wl, on, monkeypatch):
    """One forward and backward of L = sum(wl * y^2) / 2: the quadratic loss of
    tests/test_gpu_conv_stats.py::test_bottleneck_switch, whose docstring says
    why (a flipped exit ReLU mask then moves the gradients continuously)."""
    monkeypatch.setenv("DWT_AMD_DENSE_ROUTE", "1" if on else "0")
    blk.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True)
    y = blk(xin)
    (0.5 * y.float() ** 2 * wl).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    return y.detach(), xin.grad, grads


def _counters(mfma):
    """(dense forwards, stats forwards, dense data gradients)"""
    fn = mfma._Conv1x1Fn
    return (fn.dense_fwd_calls, fn.stats_calls, fn.dense_dgrad_calls)


@pytest.mark.parametrize("style", ["layer1", "layer2"])
def test_bottleneck_dense_route(ext, style, monkeypatch):
    from dwt_amd.ops import mfma
    blk, x, wl = _block(style)
    # this test is about the wiring: every eligible pass routes, whatever the
    # measured table says about the shape
    monkeypatch.setattr(mfma, "dense_route_ok", lambda which, cin, cout: True)
    ext.set_dense_glds(True)

    c0 = _counters(mfma)
    g0 = ext.dense_glds_launches()
    y_off, dx_off, g_off = _block_step(blk, x, wl, False, monkeypatch)
    c1 = _counters(mfma)
    g1 = ext.dense_glds_launches()
    assert (c1[0], c1[2]) == (c0[0], c0[2]), "switch off still routed"
    y_on, dx_on, g_on = _block_step(blk, x, wl, True, monkeypatch)
    c2 = _counters(mfma)
    g2 = ext.dense_glds_launches()
    d = tuple(b - a for a, b in zip(c1, c2))
    if style == "layer1":
        # conv1, conv3 and the stride-1 downsample: the table of the stats
        # route keeps all three on the plain forward, so they are dense
        assert d == (3, 0, 3), d
        assert g1 - g0 == 0 and g2 - g1 == 6      # no silent fallback
    else:
        # conv1 and conv3 run the fused stats forward; their dgrads route
        assert d == (0, 2, 2), d
        assert g1 - g0 == 2 and g2 - g1 == 4

    print(f"{style}: y {_rel_err(y_on, y_off):.3g} dx {_rel_err(dx_on, dx_off):.3g}")
    assert _rel_err(y_on, y_off) < 0.05
    assert _rel_err(dx_on, dx_off) < 0.05
    assert set(g_on) == set(g_off)
    for name in g_off:
        err = _rel_err(g_on[name], g_off[name])
        print(f"  {name}: {err:.3g}")
        assert err < 0.05, (name, err)


def test_whole_model_routes_by_the_tables(dev, monkeypatch):
    """The committed tables, unpatched, on a whole model: one forward and
    backward of ResNetDWT [1, 1, 1, 1] on 96x3x64x64 (32 images per branch).
    Rows per branch are 8192, 2048, 512 and 128 in layers 1-4, the smallest
    sizes at which every stage still meets the stats kernel's 128-row tile.

    Layer 1's conv1, conv3 and stride-1 downsample take the dense forward
    (3); conv1 and conv3 of layers 2-4 the stats forward (6); all nine take
    the dense data gradient.  The stride-2 downsamples are the module's."""
    from dwt_amd.models import Bottleneck, ResNetDWT
    from dwt_amd.ops import mfma
    monkeypatch.delenv("DWT_AMD_DENSE_ROUTE", raising=False)
    monkeypatch.delenv("DWT_AMD_FUSED_CONV_STATS", raising=False)
    torch.manual_seed(7)
    model = ResNetDWT(Bottleneck, [1, 1, 1, 1], None, num_classes=5)
    model = model.to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(PARTS * 32, 3, 64, 64, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    c0 = _counters(mfma)
    out = model(x)
    out.float().square().sum().backward()
    torch.cuda.synchronize()
    d = tuple(b - a for a, b in zip(c0, _counters(mfma)))
    assert d == (3, 6, 9), d
    assert torch.isfinite(out).all()
