"""Bit-exact pins of the MFMA conv / GEMM paths that the rest of the suite
holds only to a relative bound: the generic and the class-decomposed dgrad,
the forward gather with the narrow (bias + ReLU, 2-byte store) epilogue, and
the dense register-staged loop.

Inputs are small integers (tests/exact_cases.py): activations in [0, 4),
weights in [-2, 2], bias in quarter steps.  Every partial sum is then an
exact fp32 value far below 2^24 (K <= 256 here, |sum| <= K * 3 * 2), so the
result does not depend on the accumulation order; each test asserts that the
fp32 CPU reference equals the fp64 one.  The expected output is that
reference rounded once to bf16, compared bit for bit.
"""
import functools

import pytest
import torch

from exact_cases import exact_case, same_bits

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dwt_amd.kernels import dispatch
    assert dispatch.available(), "HIP extension must be built+loaded on a GPU box"
    return torch.device("cuda:0")


@pytest.fixture()
def staged(dev):
    """The extension with the dense kernels on the register-staged loop; the
    switch is restored afterwards."""
    from dwt_amd.kernels import dispatch
    e = dispatch.ext()
    was = e.dense_glds_selected()
    e.set_dense_glds(False)
    yield e
    e.set_dense_glds(was)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------
# dgrad.  (N, Cin, H, W, Cdy, k, stride, pad): dx is (N, Cin, H, W)
# ---------------------------------------------------------------------------
DGRAD = {
    # generic gather (A_DGRAD): M = 162 (ragged second M-tile), K = 144
    # (ragged third k-step), Cin = 24 (ragged N-tile)
    "gather_s1": (2, 24, 9, 9, 16, 3, 1, 1),
    # stride 2 stays on the generic path when Cdy is no power of two
    "gather_s2_cdy24": (2, 24, 9, 9, 24, 3, 2, 1),
    # (Cdy % 8 != 0, the per-element gather, is not pinned: it drops the
    # elements of a chunk that lie in the next tap, see docs/ROADMAP.md)
    # class-decomposed: odd extent (the four classes differ in Hc / Wc) ...
    "classes_odd": (2, 40, 9, 9, 16, 3, 2, 1),
    # ... and even extent
    "classes_even": (2, 40, 8, 8, 16, 3, 2, 1),
}


@functools.lru_cache(maxsize=None)
def _dgrad_case(name):
    n, cin, h, w, cdy, k, s, p = DGRAD[name]
    ph, pw = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    gen = torch.Generator().manual_seed(4321 + sorted(DGRAD).index(name))
    dy = torch.randint(0, 4, (n, cdy, ph, pw), generator=gen).float()
    wt = torch.randint(-2, 3, (cdy, cin, k, k), generator=gen).float()
    dx = torch.nn.grad.conv2d_input((n, cin, h, w), wt, dy, s, p)
    dx64 = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(),
                                      s, p)
    assert torch.equal(dx.double(), dx64), "fp32 reference is not exact"
    return dy, wt, dx.to(BF16)


@pytest.mark.parametrize("name", list(DGRAD))
def test_dgrad_bit_exact(dev, name):
    from dwt_amd.ops.mfma import conv2d_dgrad
    n, cin, h, w, cdy, k, s, p = DGRAD[name]
    dy, wt, want = _dgrad_case(name)
    got = conv2d_dgrad(_cl(dy.to(BF16)).to(dev), _cl(wt.to(BF16)).to(dev),
                       (n, cin, h, w), stride=s, padding=p)
    assert got.shape == want.shape and got.dtype == BF16
    got = got.cpu()
    nbad = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
    print(f"{name}: {nbad} of {want.numel()} elements differ")
    assert same_bits(got, want)


# ---------------------------------------------------------------------------
# forward gather, narrow epilogue with bias + ReLU
# (N, Cin, H, W, Cout, k, stride, pad)
# ---------------------------------------------------------------------------
FWD_GATHER = {
    "chunks8_cin8": (2, 8, 9, 9, 40, 3, 2, 1),     # 8-channel chunks
    "scalar_cin12": (2, 12, 9, 9, 40, 3, 2, 1),    # per-element gather
    "stem": (2, 3, 16, 16, 64, 7, 2, 3),           # Cin = 3 padded to 4
}
# dense register-staged loop, 1x1 forward
FWD_DENSE = {
    # single-buffered, ragged K (72 = 64 + 8), M = 162, ragged N
    "k72": (2, 72, 9, 9, 40, 1, 1, 0),
    # PIPE (K = 256 = 4 k-steps) and SWZ (8 N-tiles x 2 M-tiles)
    "pipe_swz": (4, 256, 8, 8, 1024, 1, 1, 0),
}


def _fwd_seed(name):
    return 5000 + sorted(list(FWD_GATHER) + list(FWD_DENSE)).index(name)


def _run_fwd(dev, shape, seed, bias, relu):
    from dwt_amd.ops.mfma import conv2d_fwd
    n, cin, h, w, cout, k, s, p = shape
    case = exact_case(shape, seed)
    want = case["conv"]
    if bias:
        want = want + case["bias"].view(1, -1, 1, 1)
    if relu:
        want = torch.relu(want)
    want = want.to(BF16)
    got = conv2d_fwd(_cl(case["x"].to(BF16)).to(dev),
                     _cl(case["w"].to(BF16)).to(dev),
                     bias=case["bias"].to(dev) if bias else None,
                     stride=s, padding=p, relu=relu)
    assert got.shape == want.shape and got.dtype == BF16
    got = got.cpu()
    nbad = (got.view(torch.int16) != want.view(torch.int16)).sum().item()
    print(f"{shape}: {nbad} of {want.numel()} elements differ")
    assert same_bits(got, want)


@pytest.mark.parametrize("name", list(FWD_GATHER))
def test_fwd_gather_bias_relu_bit_exact(dev, name):
    _run_fwd(dev, FWD_GATHER[name], _fwd_seed(name), bias=True, relu=True)


@pytest.mark.parametrize("name", list(FWD_DENSE))
def test_fwd_dense_staged_bit_exact(staged, dev, name):
    n0 = staged.dense_glds_launches()
    _run_fwd(dev, FWD_DENSE[name], _fwd_seed(name), bias=False, relu=False)
    assert staged.dense_glds_launches() == n0, "the direct-to-LDS loop ran"


def test_gemm_staged_bias_relu_bit_exact(staged, dev):
    """mfma_gemm's epilogue on the register-staged loop: M = 162, K = 72 and
    N = 40 are all ragged."""
    from dwt_amd.ops.mfma import mfma_gemm
    gen = torch.Generator().manual_seed(77)
    a = torch.randint(0, 4, (162, 72), generator=gen).float()
    bt = torch.randint(-2, 3, (40, 72), generator=gen).float()
    bias = torch.randint(-8, 9, (40,), generator=gen).float() * 0.25
    ref = a @ bt.t()
    assert torch.equal(ref.double(), a.double() @ bt.double().t()), \
        "fp32 reference is not exact"
    want = torch.relu(ref + bias).to(BF16)
    n0 = staged.dense_glds_launches()
    got = mfma_gemm(a.to(BF16).to(dev), bt.to(BF16).to(dev),
                    bias=bias.to(dev), relu=True)
    assert staged.dense_glds_launches() == n0, "the direct-to-LDS loop ran"
    assert got.shape == want.shape and got.dtype == BF16
    assert same_bits(got.cpu(), want)
