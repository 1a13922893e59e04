"""Integer-valued conv cases whose fp32 reference is exact, shared by the
bit-exact GPU tests (test_gpu_folded.py, test_gpu_mfma_exact.py)."""
import torch
import torch.nn.functional as F

_EXACT = {}


def out_hw(shape):
    n, cin, h, w, cout, k, s, p = shape
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def exact_case(shape, seed):
    """Integer-valued inputs (exact in bf16, every partial sum an exact fp32
    integer whatever the accumulation order) and the fp32 conv of them, drawn
    once per (shape, seed) on the CPU and left unchanged.

    shape is (N, Cin, H, W, Cout, k, stride, pad): activations in [0, 4),
    weights in [-2, 2], bias and residual in quarter steps."""
    key = (shape, seed)
    if key in _EXACT:
        return _EXACT[key]
    n, cin, h, w, cout, k, s, p = shape
    gen = torch.Generator().manual_seed(seed)
    ph, pw = out_hw(shape)
    x = torch.randint(0, 4, (n, cin, h, w), generator=gen).float()
    wt = torch.randint(-2, 3, (cout, cin, k, k), generator=gen).float()
    bias = torch.randint(-8, 9, (cout,), generator=gen).float() * 0.25
    res = torch.randint(-16, 17, (n, cout, ph, pw), generator=gen).float() * 0.25
    conv = F.conv2d(x, wt, None, s, p)
    conv64 = F.conv2d(x.double(), wt.double(), None, s, p)
    assert torch.equal(conv.double(), conv64), "fp32 reference is not exact"
    case = dict(x=x, w=wt, bias=bias, res=res, conv=conv)
    _EXACT[key] = case
    return case


def same_bits(got, want):
    """bf16 tensors equal bit for bit (so -0.0 != 0.0 and NaNs compare)."""
    return torch.equal(got.view(torch.int16), want.view(torch.int16))
