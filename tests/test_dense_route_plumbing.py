"""CPU checks of the routing of the 1x1 convs: the planner's decisions for
every 1x1 stride-1 conv of ResNet50, and without the extension the autograd
Function and the model's entry point are the library's conv and its backward;
the table is well formed."""
import pytest
import torch
import torch.nn.functional as F

from dwt_amd.ops import mfma


def _case(cin=64, cout=64, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(6, cin, 8, 8, generator=gen).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(cout, cin, 1, 1, generator=gen) * cin ** -0.5
    dy = torch.randn(6, cout, 8, 8, generator=gen)
    return x, w, dy


def _reference(x, w, dy):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = F.conv2d(x, w)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


def _counters():
    fn = mfma._Conv1x1Fn
    return (fn.dense_fwd_calls, fn.stats_calls, fn.dense_dgrad_calls)


def test_conv1x1_fn_is_the_library_on_cpu():
    x, w, dy = _case()
    assert mfma.dense_route_ok("fwd", 64, 64) and mfma.dense_route_ok("dgrad", 64, 64)
    plan = mfma.plan_conv1x1(6, 64, 8, 8, 64, "whiten", 4, 3)
    assert (plan.fwd, plan.dgrad) == ("dense", "dense")
    before = _counters()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, acc = mfma._Conv1x1Fn.apply(xr, wr, plan)
    assert acc is None
    y.backward(dy)
    assert _counters() == before
    y_ref, dx_ref, dw_ref = _reference(x, w, dy)
    assert torch.equal(y.detach(), y_ref)
    assert torch.equal(xr.grad, dx_ref)
    assert torch.equal(wr.grad, dw_ref)


def test_stats_fn_backward_is_the_library_on_cpu():
    """The stats forward needs the GPU; the backward of a plan with a dense
    data gradient must be aten's conv backward where the kernel cannot run."""
    x, w, dy = _case(seed=1)
    plan = mfma.Conv1x1Plan("library", "dense", "bn", 0, 3)
    _, dx_ref, dw_ref = _reference(x, w, dy)
    before = _counters()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, acc = mfma._Conv1x1Fn.apply(xr, wr, plan)
    assert acc is None
    dx, dw = torch.autograd.grad(y, (xr, wr), dy)
    assert _counters() == before
    assert torch.equal(dx, dx_ref) and torch.equal(dw, dw_ref)

    # without an input gradient: dx is None at the Function's backward itself
    wr = w.clone().requires_grad_(True)
    y, _ = mfma._Conv1x1Fn.apply(x, wr, plan)
    got = {}
    node = y.grad_fn
    node.register_hook(lambda gin, gout: got.update(gin=gin))
    (dw,) = torch.autograd.grad(y, (wr,), dy)
    assert got["gin"][0] is None and torch.equal(dw, dw_ref)
    assert _counters() == before


def test_wrapper_is_the_module_on_cpu(monkeypatch):
    x, w, _ = _case(seed=2)
    conv = torch.nn.Conv2d(64, 64, 1, bias=False)
    branches = [torch.nn.Identity()] * 3
    for env in ("1", "0"):
        monkeypatch.setenv("DWT_AMD_DENSE_ROUTE", env)
        for training in (True, False):
            out, acc = mfma.conv1x1_routed(conv, x, branches, training)
            assert acc is None and torch.equal(out, conv(x))


def test_table_is_well_formed():
    assert mfma._DENSE_ROUTE, "empty table"
    for (which, cin, cout), ratio in mfma._DENSE_ROUTE.items():
        assert which in ("fwd", "dgrad")
        # the direct-to-LDS loop takes whole 64-deep k-steps and 8-wide stores
        k, n = (cin, cout) if which == "fwd" else (cout, cin)
        assert k % 64 == 0 and n % 8 == 0, (which, cin, cout)
        assert ratio > 1.05, (which, cin, cout, ratio)   # the routing rule
    assert not mfma.dense_route_ok("fwd", 72, 64)


# ---------------------------------------------------------------------------
# the planner on every 1x1 stride-1 conv of ResNet50 [3, 4, 6, 3]
# ---------------------------------------------------------------------------

# (Cin, Cout) in model order: conv1, conv3, the stride-1 downsample of block 0,
# then conv1, conv3 of blocks 1 and 2; whitening sites with g = 4
LAYER1 = [(64, 64), (64, 256), (64, 256),
          (256, 64), (64, 256), (256, 64), (64, 256)]
# conv1, conv3 of each block (the downsamples have stride 2); BN sites
LAYER234 = [(256, 128), (128, 512)] + [(512, 128), (128, 512)] * 3 \
    + [(512, 256), (256, 1024)] + [(1024, 256), (256, 1024)] * 5 \
    + [(1024, 512), (512, 2048)] + [(2048, 512), (512, 2048)] * 2
PARTS = 3


def _plans(shapes, kind, g, hw):
    """(fwd, dgrad) per conv; 2 images per branch of hw x hw."""
    got = []
    for cin, cout in shapes:
        plan = mfma.plan_conv1x1(PARTS * 2, cin, hw, hw, cout, kind, g, PARTS)
        assert (plan.kind, plan.g, plan.parts) == (kind, g, PARTS)
        got.append((plan.fwd, plan.dgrad))
    return got


# (DWT_AMD_DENSE_ROUTE, DWT_AMD_FUSED_CONV_STATS, rows per branch) ->
# the plan of every layer-1 conv, the plan of every layer-2/3/4 conv
PLAN_CASES = [
    (None, None, 128, ("dense", "dense"), ("stats", "dense")),
    ("1", "1", 128, ("dense", "dense"), ("stats", "dense")),
    (None, None, 98, ("dense", "dense"), ("library", "dense")),
    ("0", None, 128, ("library", "library"), ("stats", "library")),
    (None, "0", 128, ("dense", "dense"), ("library", "dense")),
    ("0", "0", 128, ("library", "library"), ("library", "library")),
]


@pytest.mark.parametrize("dense,stats,rows,want1,want234", PLAN_CASES)
def test_planner_on_resnet50(monkeypatch, dense, stats, rows, want1, want234):
    assert len(LAYER1) == 7 and len(LAYER234) == 26
    for name, val in (("DWT_AMD_DENSE_ROUTE", dense),
                      ("DWT_AMD_FUSED_CONV_STATS", stats)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    hw = {128: 8, 98: 7}[rows]
    assert 2 * hw * hw == rows
    assert _plans(LAYER1, "whiten", 4, hw) == [want1] * 7
    assert _plans(LAYER234, "bn", 0, hw) == [want234] * 26


def test_planner_g2_whitening_never_plans_stats(monkeypatch):
    monkeypatch.delenv("DWT_AMD_DENSE_ROUTE", raising=False)
    monkeypatch.delenv("DWT_AMD_FUSED_CONV_STATS", raising=False)
    # the same convs behind a g = 4 whitening site do plan it where the NHWC
    # whitening kernels serve Cout (up to 256, or a multiple of 256)
    g4 = _plans(LAYER234, "whiten", 4, 8)
    assert g4 == [("stats", "dense")] * 26
    for shapes in (LAYER1, LAYER234):
        assert all(fwd != "stats" for fwd, _ in _plans(shapes, "whiten", 2, 8))
    assert _plans(LAYER234, "whiten", 2, 8) == [("library", "dense")] * 26
    # nor does a site of a kind the stats kernel does not know
    assert _plans(LAYER234, None, 0, 8) == [("library", "dense")] * 26
