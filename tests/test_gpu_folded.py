"""Folded inference on the GPU: the conv forward with the bias / residual /
ReLU epilogue (bit-exact single rounding, bounds, preconditions) and the
folded bf16 model against the fp32 oracle."""
import types

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from exact_cases import exact_case as _shared_exact_case, out_hw

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# (N, Cin, H, W, Cout, k, stride, pad); every one has a ragged last M-tile
SHAPES = [
    (2, 64, 9, 9, 64, 3, 1, 1),       # M=162, half an N-tile, gather
    (2, 64, 9, 9, 192, 1, 1, 0),      # ragged second N-tile, dense, one k-step
    (2, 256, 9, 9, 64, 1, 1, 0),      # dense PIPE path
    (2, 256, 9, 9, 1024, 1, 1, 0),    # PIPE + SWZ: 8 N-tiles x 2 M-tiles
    (2, 64, 9, 9, 128, 3, 2, 1),      # strided 3x3, M=50
    (2, 128, 9, 9, 256, 1, 2, 0),     # the stride-2 downsample
    (2, 3, 20, 20, 64, 7, 2, 3),      # stem
]
IDS = ["gather3x3", "dense_ragged_n", "dense_pipe", "dense_pipe_swz",
       "strided3x3", "downsample_s2", "stem"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from dwt_amd.kernels import dispatch
    assert dispatch.available()
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _out_hw(shape):
    return out_hw(shape)


def exact_case(shape):
    """The shared integer-valued case of this shape (tests/exact_cases.py),
    one fixed seed per shape."""
    return _shared_exact_case(shape, 1234 + SHAPES.index(shape))


def expected(case, relu, with_res):
    v = case["conv"] + case["bias"].view(1, -1, 1, 1)
    if with_res:
        v = v + case["res"]
    if relu:
        v = torch.relu(v)
    return v.to(BF16)


def double_rounded(case, relu):
    v = (case["conv"] + case["bias"].view(1, -1, 1, 1)).to(BF16).float()
    v = v + case["res"]
    if relu:
        v = torch.relu(v)
    return v.to(BF16)


def run_kernel(dev, case, shape, relu, with_res, out=None):
    from dwt_amd.ops.mfma import conv2d_fused_fwd
    n, cin, h, w, cout, k, s, p = shape
    x = _cl(case["x"].to(BF16)).to(dev)
    wt = _cl(case["w"].to(BF16)).to(dev)
    res = _cl(case["res"].to(BF16)).to(dev) if with_res else None
    return conv2d_fused_fwd(x, wt, case["bias"].to(dev), stride=s, padding=p,
                            relu=relu, residual=res, out=out, route=False)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]],
                         ids=[IDS[0], IDS[2]])
def test_inputs_tell_single_from_double_rounding(shape):
    """CPU-only property of the test inputs: rounding conv + bias to bf16
    before the residual add gives another tensor, so bit equality below
    proves the single rounding."""
    case = exact_case(shape)
    for relu in (False, True):
        want = expected(case, relu, True)
        twice = double_rounded(case, relu)
        ndiff = (want.view(torch.int16) != twice.view(torch.int16)).sum().item()
        print(f"{shape} relu={relu}: {ndiff} elements differ")
        assert ndiff >= 1


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_epilogue_bit_exact(dev, shape, relu, with_res):
    case = exact_case(shape)
    want = expected(case, relu, with_res)
    got = run_kernel(dev, case, shape, relu, with_res)
    assert got.shape == want.shape and got.dtype == BF16
    assert got.is_contiguous(memory_format=torch.channels_last)
    got = got.cpu()
    nbad = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
    assert nbad == 0, f"{nbad} of {want.numel()} elements differ"


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_parity(dev, shape, with_res):
    from dwt_amd.ops.mfma import conv2d_fused_fwd
    n, cin, h, w, cout, k, s, p = shape
    torch.manual_seed(7)
    ph, pw = _out_hw(shape)
    x = _cl(torch.randn(n, cin, h, w, device=dev).to(BF16))
    wt = _cl((torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5).to(BF16))
    bias = torch.randn(cout, device=dev)
    res = _cl(torch.randn(n, cout, ph, pw, device=dev).to(BF16)) if with_res else None
    got = conv2d_fused_fwd(x, wt, bias, stride=s, padding=p, relu=True,
                           residual=res, route=False)
    ref = F.conv2d(x.float(), wt.float(), bias, s, p)
    if with_res:
        ref = ref + res.float()
    ref = torch.relu(ref)
    err = ((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    print(f"{shape} res={with_res}: rel max err {err:.3e}")
    assert err < 0.05, err
    # the routed default computes the same thing, whichever side it picks
    routed = conv2d_fused_fwd(x, wt, bias, stride=s, padding=p, relu=True,
                              residual=res)
    err_r = ((routed.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    assert err_r < 0.05, err_r


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[5]],
                         ids=[IDS[0], IDS[1], IDS[4], IDS[5]])
def test_nothing_written_outside_out(dev, shape):
    """out= is a channels_last view inside a larger sentinel-filled buffer:
    the bytes before and after it stay untouched (M=162 and M=50 ragged
    tiles; Cout = 64, 192, 128, 256)."""
    n, cin, h, w, cout, k, s, p = shape
    ph, pw = _out_hw(shape)
    numel = n * cout * ph * pw
    pre, post = 64, 128 * 256            # pre keeps out 16-byte aligned
    sentinel = 0x7B5A
    buf = torch.full((pre + numel + post,), sentinel, dtype=torch.int16,
                     device=dev)
    out = buf[pre:pre + numel].view(BF16).view(n, ph, pw, cout).permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 == 0
    case = exact_case(shape)
    got = run_kernel(dev, case, shape, True, True, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert (buf[:pre] == sentinel).all().item()
    assert (buf[pre + numel:] == sentinel).all().item()
    want = expected(case, True, True)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_preconditions_raise_before_launch(dev):
    from dwt_amd.ops.mfma import conv2d_fused_fwd
    x = _cl(torch.randn(2, 64, 9, 9, device=dev).to(BF16))
    w = _cl(torch.randn(64, 64, 1, 1, device=dev).to(BF16))
    b = torch.zeros(64, device=dev)
    # Cout % 8 != 0
    w12 = _cl(torch.randn(12, 64, 1, 1, device=dev).to(BF16))
    with pytest.raises(ValueError, match="Cout % 8"):
        conv2d_fused_fwd(x, w12, torch.zeros(12, device=dev))
    # misaligned residual: a dense NHWC view one element into a buffer
    numel = 2 * 64 * 9 * 9
    flat = torch.zeros(numel + 8, device=dev, dtype=BF16)
    res_mis = flat[1:1 + numel].view(2, 9, 9, 64).permute(0, 3, 1, 2)
    assert res_mis.data_ptr() % 16 != 0
    with pytest.raises(ValueError, match="16-byte aligned"):
        conv2d_fused_fwd(x, w, b, residual=res_mis)
    # NCHW residual
    with pytest.raises(ValueError, match="channels_last"):
        conv2d_fused_fwd(x, w, b, residual=torch.zeros(2, 64, 9, 9, device=dev, dtype=BF16))
    # wrong residual shape
    with pytest.raises(ValueError, match="shape"):
        conv2d_fused_fwd(x, w, b, residual=_cl(torch.zeros(2, 64, 8, 9, device=dev, dtype=BF16)))
    # out aliases the residual / the input
    res = _cl(torch.zeros(2, 64, 9, 9, device=dev, dtype=BF16))
    with pytest.raises(ValueError, match="aliases residual"):
        conv2d_fused_fwd(x, w, b, residual=res, out=res)
    with pytest.raises(ValueError, match="aliases x"):
        conv2d_fused_fwd(x, w, b, out=x)


# ---------------------------------------------------------------------------
# the folded model
# ---------------------------------------------------------------------------

def _small_model():
    from test_folded import make_model
    return make_model([2, 1, 2, 1], mode="zca", dtype=torch.float32, seed=3)


def test_model_parity_bf16(dev):
    """e_fold <= 2 e_eval: max-abs error over max|oracle| of the folded bf16
    model and of the existing bf16 channels_last eval, both against the fp32
    model's eval output.  The two paths round at different places with the
    same number format; a factor of 2 covers that and nothing more."""
    from dwt_amd.models import fold_resnet
    from dwt_amd.ops import mfma
    model = _small_model()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 64, 64, generator=gen)
    with torch.no_grad():
        oracle = model(x)
    m16 = model.to(dev).to(BF16).to(memory_format=torch.channels_last).eval()
    x16 = x.to(dev).to(BF16)
    x16_cl = _cl(x16)
    calls = []
    real = mfma.conv2d_fused_fwd
    with torch.no_grad():
        y_eval = m16(x16_cl).float().cpu()
        folded = fold_resnet(m16)
        mfma.conv2d_fused_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            y_fold = folded(x16_cl).float().cpu()
            y_fold_nchw = folded(x16).float().cpu()
            folded.route = False        # every conv on the kernel
            y_kern = folded(x16_cl).float().cpu()
            y_kern_nchw = folded(x16).float().cpu()
        finally:
            mfma.conv2d_fused_fwd = real
    # one call per conv of the network, per forward
    nconv = 1 + sum(3 * b for b in folded.layers) + 4
    assert len(calls) == 4 * nconv
    scale = oracle.abs().max()
    e_eval = ((y_eval - oracle).abs().max() / scale).item()
    e_fold = ((y_fold - oracle).abs().max() / scale).item()
    e_kern = ((y_kern - oracle).abs().max() / scale).item()
    print(f"model parity: e_eval = {e_eval:.4e}, e_fold = {e_fold:.4e} "
          f"(routed), {e_kern:.4e} (every conv on the kernel)")
    assert e_fold <= 2 * e_eval, (e_fold, e_eval)
    assert e_kern <= 2 * e_eval, (e_kern, e_eval)
    # NCHW or channels_last input: the same output, bit for bit, where every
    # conv runs on the project's kernel.  The routed model cannot be held to
    # that: the library conv it routes some shapes to is not bit-reproducible
    # (measured: `F.conv2d` in bf16 with a bias, called three times on one
    # input, returned differing tensors for 12 of this model's 17 conv
    # shapes, and six forwards of the routed model on one input differed by
    # up to 0.25 at logits of magnitude 70).  So there the two outputs, each
    # a bf16 evaluation of the same network, are held to the bound each is
    # held to against the oracle.
    assert torch.equal(y_kern, y_kern_nchw)
    d_routed = ((y_fold - y_fold_nchw).abs().max() / scale).item()
    print(f"routed, NCHW vs channels_last input: {d_routed:.3e}")
    assert d_routed <= 2 * e_eval, (d_routed, e_eval)


def test_folded_engine_test_gpu(dev, capsys):
    """engine.test on the synthetic uint8 loader with the DeviceBatcher eval
    path prints the unchanged line for the folded model."""
    from dwt_amd.data import SyntheticOfficeHome
    from dwt_amd.data.device_pipeline import DeviceBatcher
    from dwt_amd.engine import officehome as engine
    from dwt_amd.models import fold_resnet
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    model = _small_model().to(dev).to(BF16).to(memory_format=torch.channels_last)
    # frame size == crop size: the eval crop has one position, so two passes
    # see the same batches
    ds = SyntheticOfficeHome(16, num_classes=7, img_size=64, seed=2, uint8=True)
    loader = DataLoader(ds, batch_size=8)
    batcher = DeviceBatcher(64, mean, std, BF16, dev, seed=0)
    args = types.SimpleNamespace(folded_eval=True)
    acc = engine.test(args, model, dev, loader, batcher=batcher)
    out = capsys.readouterr().out
    assert 0.0 <= acc <= 100.0
    assert "\nTest set: Average loss: " in out and "Accuracy: " in out
    assert out.count("Test set") == 1
    acc2 = engine.test(types.SimpleNamespace(), fold_resnet(model), dev, loader,
                       batcher=batcher)
    assert acc2 == acc
