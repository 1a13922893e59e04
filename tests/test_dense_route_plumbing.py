"""CPU checks of the dense-kernel routing of the 1x1 convs: without the
extension both autograd Functions and the wrapper are the library's conv and
its backward, and the table is well formed."""
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


def test_conv1x1_fn_is_the_library_on_cpu():
    x, w, dy = _case()
    assert mfma.dense_route_ok("fwd", 64, 64) and mfma.dense_route_ok("dgrad", 64, 64)
    before = (mfma._Conv1x1Fn.fwd_calls, mfma._Conv1x1Fn.dgrad_calls)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = mfma._Conv1x1Fn.apply(xr, wr)
    y.backward(dy)
    assert (mfma._Conv1x1Fn.fwd_calls, mfma._Conv1x1Fn.dgrad_calls) == before
    y_ref, dx_ref, dw_ref = _reference(x, w, dy)
    assert torch.equal(y.detach(), y_ref)
    assert torch.equal(xr.grad, dx_ref)
    assert torch.equal(wr.grad, dw_ref)


def test_stats_fn_backward_is_the_library_on_cpu():
    """_Conv1x1StatsFn's forward needs the GPU; its backward is the shared
    helper, which must be aten's conv backward where the kernel cannot run."""
    x, w, dy = _case(seed=1)
    before = mfma._Conv1x1StatsFn.dgrad_calls
    dx, dw = mfma._conv1x1_backward(mfma._Conv1x1StatsFn, dy, x, w, True)
    assert mfma._Conv1x1StatsFn.dgrad_calls == before
    _, dx_ref, dw_ref = _reference(x, w, dy)
    assert torch.equal(dx, dx_ref) and torch.equal(dw, dw_ref)
    dx, dw = mfma._conv1x1_backward(mfma._Conv1x1StatsFn, dy, x, w, False)
    assert dx is None and torch.equal(dw, dw_ref)


def test_wrapper_is_the_module_on_cpu(monkeypatch):
    x, w, _ = _case(seed=2)
    conv = torch.nn.Conv2d(64, 64, 1, bias=False)
    for env in ("1", "0"):
        monkeypatch.setenv("DWT_AMD_DENSE_ROUTE", env)
        for training in (True, False):
            assert torch.equal(mfma.conv1x1_dense(conv, x, training), conv(x))


def test_table_is_well_formed():
    assert mfma._DENSE_ROUTE, "empty table"
    for (which, cin, cout), ratio in mfma._DENSE_ROUTE.items():
        assert which in ("fwd", "dgrad")
        # the direct-to-LDS loop takes whole 64-deep k-steps and 8-wide stores
        k, n = (cin, cout) if which == "fwd" else (cout, cin)
        assert k % 64 == 0 and n % 8 == 0, (which, cin, cout)
        assert ratio > 1.05, (which, cin, cout, ratio)   # the routing rule
    assert not mfma.dense_route_ok("fwd", 72, 64)
