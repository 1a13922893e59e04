"""Python layer over the hand-written MFMA GEMM / implicit-GEMM conv kernels.

``mfma_gemm``: C[M,N] = A[M,K] @ B[N,K]^T (+bias/+ReLU), bf16 in, fp32
accumulate, bf16 out — the v_mfma_f32_16x16x32_bf16 tile kernel.

``MFMALinear``: nn.Linear whose forward AND backward run on mfma_gemm
(dgrad/wgrad are plain GEMMs with small host-side transposes).

``conv2d_fwd``: NHWC implicit-GEMM convolution forward on the same kernel
(1x1 degenerates to the dense-GEMM fast path; KxK gathers patches on the
fly; the channels_last conv weight is consumed as stored).

``conv2d_fused_fwd``: the same conv with the folded-inference epilogue,
``bf16(relu(conv + bias + residual))`` in one launch (fp32 adds, one
rounding, 16-byte stores), routed per shape by a measured table.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


def _ext():
    from ..kernels import dispatch
    return dispatch.ext()


def _pad_k(t: torch.Tensor) -> torch.Tensor:
    k = t.shape[1]
    if k % 8 == 0:
        return t
    return F.pad(t, (0, 8 - k % 8))


def mfma_gemm(a: torch.Tensor, bt: torch.Tensor,
              bias: Optional[torch.Tensor] = None, relu: bool = False):
    """a (M,K) bf16, bt (N,K) bf16 -> (M,N) bf16 = a @ bt.T."""
    assert a.dtype == torch.bfloat16 and bt.dtype == torch.bfloat16
    a = _pad_k(a.contiguous())
    bt = _pad_k(bt.contiguous())
    m, n = a.shape[0], bt.shape[0]
    out = torch.empty(m, n, device=a.device, dtype=torch.bfloat16)
    has_bias = bias is not None
    b32 = bias.detach().float().contiguous() if has_bias else torch.empty(0, device=a.device)
    _ext().mfma_gemm(a, bt, b32, out, relu, has_bias)
    return out


class _MFMALinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x2 = x.reshape(-1, x.shape[-1])
        out = mfma_gemm(x2, weight, bias=bias, relu=False)
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        ctx.in_shape = x.shape
        return out.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dout):
        x2, weight = ctx.saved_tensors
        dout2 = dout.reshape(-1, dout.shape[-1]).contiguous()
        # dx = dy @ W          : A = dy (M,N), Bt = W^T (K,N)
        dx = mfma_gemm(dout2, weight.t().contiguous())
        # dW = dy^T @ x        : A = dy^T (N,M), Bt = x^T (K,M)
        dw = mfma_gemm(dout2.t().contiguous(), x2.t().contiguous())
        db = dout2.sum(0).to(dout.dtype) if ctx.has_bias else None
        return dx.reshape(ctx.in_shape), dw, db


class MFMALinear(nn.Linear):
    """nn.Linear running fwd/dgrad/wgrad on the hand-written MFMA GEMM when
    on GPU in bf16; falls back to F.linear otherwise."""

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and self.weight.dtype == torch.bfloat16:
            from ..kernels import dispatch
            if dispatch.available():
                return _MFMALinearFn.apply(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)


def _pad_stem_channels(t: torch.Tensor) -> torch.Tensor:
    """The stem's 3-channel input or weight zero-padded to 4 channels,
    channels_last, so the kernel's paired-pixel 16-B path applies (NHWC C=4
    chunks)."""
    n, _, h, w = t.shape
    t4 = torch.empty(n, 4, h, w, device=t.device, dtype=t.dtype,
                     memory_format=torch.channels_last)
    t4[:, 3] = 0
    t4[:, :3] = t
    return t4


def conv2d_fwd(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None, stride: int = 1,
               padding: int = 0, relu: bool = False) -> torch.Tensor:
    """NHWC implicit-GEMM conv forward (inference path).

    x: (N, C, H, W) channels_last bf16; weight: (Cout, Cin, KH, KW)
    channels_last bf16; returns (N, Cout, P, Q) channels_last bf16.
    """
    assert x.dtype == torch.bfloat16
    assert x.is_contiguous(memory_format=torch.channels_last) or x.shape[1] == 1
    n, cin, h, w = x.shape
    cout, _, kh, kw = weight.shape
    if cin == 3:  # stem; weight padded to match
        x, weight, cin = _pad_stem_channels(x), \
            _pad_stem_channels(weight.detach()), 4
    p = (h + 2 * padding - kh) // stride + 1
    q = (w + 2 * padding - kw) // stride + 1
    out = torch.empty(n, cout, p, q, device=x.device, dtype=torch.bfloat16,
                      memory_format=torch.channels_last)
    wgt = weight
    if not wgt.is_contiguous(memory_format=torch.channels_last):
        wgt = wgt.contiguous(memory_format=torch.channels_last)
    has_bias = bias is not None
    b32 = bias.detach().float().contiguous() if has_bias else torch.empty(0, device=x.device)
    _ext().mfma_conv2d_fwd(x, wgt, b32, out, n, h, w, cin, p, q, cout,
                           kh, kw, stride, padding, relu, has_bias)
    return out


# ----------------------------------------------------------------------------
# Conv forward with the bias / residual / ReLU epilogue (folded inference)
# ----------------------------------------------------------------------------

# Conv shapes ``(cin, cout, k, stride, has_residual)`` where the library conv
# with bias plus its elementwise op (in-place relu, or add_relu) measured
# faster than the fused kernel in the same sitting
# (profiles/inference_folded.md: N = 256 at 224x224, medians of alternated
# runs).  `conv2d_fused_fwd(route=True)` sends these to that composition;
# every other shape stays on the kernel.  The losers are the gather main loop
# (stem, every 3x3) and three 1x1 shapes with few M-tiles; every other 1x1,
# every residual join among them, wins by 1.06-2.8x.
_FUSED_FWD_LIBRARY_SHAPES = frozenset({
    (3, 64, 7, 2, False),          # stem            0.82 vs 0.74 ms
    (64, 64, 3, 1, False),         # l1 conv2        0.259 vs 0.231
    (128, 128, 3, 2, False),       # l2.0 conv2      0.219 vs 0.170
    (128, 128, 3, 1, False),       # l2 conv2        0.189 vs 0.165
    (256, 256, 3, 2, False),       # l3.0 conv2      0.289 vs 0.160
    (256, 256, 3, 1, False),       # l3 conv2        0.274 vs 0.158
    (512, 512, 3, 2, False),       # l4.0 conv2      0.294 vs 0.201
    (512, 512, 3, 1, False),       # l4 conv2        0.280 vs 0.195
    (512, 1024, 1, 2, False),      # l3.0 downsample 0.185 vs 0.165
    (1024, 512, 1, 1, False),      # l4.0 conv1      0.186 vs 0.159
    (1024, 2048, 1, 2, False),     # l4.0 downsample 0.207 vs 0.139
})


def fused_fwd_on_kernel(cin: int, cout: int, k: int, stride: int,
                        has_residual: bool) -> bool:
    """Whether the routing table keeps this conv shape on the fused kernel."""
    return (cin, cout, k, stride, bool(has_residual)) \
        not in _FUSED_FWD_LIBRARY_SHAPES


def _storage_range(t: torch.Tensor):
    lo = t.data_ptr()
    span = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return lo, lo + span * t.element_size()


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, a1 = _storage_range(a)
    b0, b1 = _storage_range(b)
    return a0 < b1 and b0 < a1


def _is_nhwc(t: torch.Tensor) -> bool:
    """Dense NHWC storage (size-1 dims make the torch query ambiguous, so the
    strides are compared directly)."""
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(s == 1 or st == ws for s, st, ws in zip(t.shape, t.stride(), want))


def conv2d_fused_fwd(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                     stride: int = 1, padding: int = 0, relu: bool = False,
                     residual: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None,
                     route: bool = True) -> torch.Tensor:
    """NHWC conv forward with the folded-inference epilogue, one launch:

        out = bf16( [relu]( conv(x, weight) + bias [+ residual] ) )

    with the adds in fp32 in that order and one rounding.  x (N, Cin, H, W)
    and weight (Cout, Cin, KH, KW) channels_last bf16, bias fp32 (Cout,),
    residual / out (N, Cout, P, Q) channels_last bf16, 16-byte aligned;
    Cout % 8 == 0; ``out`` (optional, preallocated) aliases neither ``x`` nor
    ``residual``.  A 3-channel ``x`` is zero-padded to 4 channels here; the
    weight may come with 3 or (padded once by the caller) 4.

    ``route=True`` (default) sends the shapes of the measured table above to
    the library conv + elementwise op instead; ``route=False`` and ``out=``
    always run the kernel.
    """
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError("conv2d_fused_fwd: x and weight must be 4-D")
    if x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise TypeError("conv2d_fused_fwd: x and weight must be bfloat16")
    n, cin, h, w = x.shape
    cout, wcin, kh, kw = weight.shape
    if cout % 8 != 0:
        raise ValueError(f"conv2d_fused_fwd: Cout % 8 != 0 (Cout = {cout}); "
                         "the epilogue stores 8 channels per lane")
    if bias is None or bias.numel() != cout:
        raise ValueError("conv2d_fused_fwd: bias of Cout elements is required")
    if wcin not in (cin, 4 if cin == 3 else cin):
        raise ValueError(f"conv2d_fused_fwd: weight Cin {wcin} vs x Cin {cin}")
    p = (h + 2 * padding - kh) // stride + 1
    q = (w + 2 * padding - kw) // stride + 1
    oshape = (n, cout, p, q)
    for name, t in (("residual", residual), ("out", out)):
        if t is None:
            continue
        if tuple(t.shape) != oshape:
            raise ValueError(f"conv2d_fused_fwd: {name}.shape {tuple(t.shape)} "
                             f"!= output shape {oshape}")
        if t.dtype != torch.bfloat16 or t.device != x.device:
            raise TypeError(f"conv2d_fused_fwd: {name} must be bfloat16 on x's device")
        if not _is_nhwc(t):
            raise ValueError(f"conv2d_fused_fwd: {name} must be channels_last")
        if t.data_ptr() % 16 != 0:
            raise ValueError(f"conv2d_fused_fwd: {name} must be 16-byte aligned")
    if out is not None:
        if _overlaps(out, x):
            raise ValueError("conv2d_fused_fwd: out aliases x")
        if residual is not None and _overlaps(out, residual):
            raise ValueError("conv2d_fused_fwd: out aliases residual")
    if not _is_nhwc(x):
        x = x.contiguous(memory_format=torch.channels_last)
    if x.data_ptr() % 16 != 0:      # the A-operand loads are 16 bytes wide
        x = x.clone(memory_format=torch.preserve_format)
    b32 = bias.detach()
    if b32.dtype != torch.float32 or not b32.is_contiguous():
        b32 = b32.float().contiguous()

    if route and out is None and not fused_fwd_on_kernel(
            cin, cout, kh, stride, residual is not None):
        from . import functional as Fdwt
        wl = weight[:, :cin] if wcin != cin else weight
        y = F.conv2d(x, wl, b32.to(torch.bfloat16), stride, padding)
        if residual is not None:
            return Fdwt.add_relu(y, residual) if relu else y + residual
        return y.relu_() if relu else y

    if cin == 3:  # stem; a weight the caller padded already stays as it is
        x, cin = _pad_stem_channels(x), 4
        if wcin == 3:
            weight = _pad_stem_channels(weight.detach())
    wgt = weight.detach()
    if not _is_nhwc(wgt):
        wgt = wgt.contiguous(memory_format=torch.channels_last)
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=torch.bfloat16,
                          memory_format=torch.channels_last)
    has_res = residual is not None
    _ext().mfma_conv2d_fwd_fused(x, wgt, b32, residual if has_res else out, out,
                                 n, h, w, cin, p, q, cout, kh, kw, stride,
                                 padding, relu, has_res)
    return out


# ----------------------------------------------------------------------------
# 1x1 conv forward with the following norm site's statistics in its epilogue
# ----------------------------------------------------------------------------

STATS_TILE_M = 128     # the kernel's M tile: rows per branch must divide by it
_STATS_KINDS = {"bn": 0, "whiten": 1}


def fused_conv_stats_enabled() -> bool:
    """``DWT_AMD_FUSED_CONV_STATS=0`` sends every 1x1 conv back to the library
    forward + stand-alone stats kernel.  Read on every call."""
    return os.environ.get("DWT_AMD_FUSED_CONV_STATS", "1") != "0"


def stats_acc_numel(kind: str, c: int, parts: int, g: int = 4) -> int:
    """Size of the raw-sums accumulator the finalize kernels read: BN
    ``[parts][2][C]``; whitening ``[parts*C/g][g + g*g]``."""
    if kind == "bn":
        return parts * 2 * c
    return parts * (c // g) * (g + g * g)


def conv_stats_shape_ok(m: int, cin: int, cout: int) -> bool:
    """Shapes where the fused conv beats library forward + stats kernel by
    more than 5% at N = 1536 (profiles/conv_stats_bench_b1536.md).

    Every shape with K = Cin >= 128 and Cout >= 128 wins by 1.33-1.66x, at
    each M measured (75 K to 4.8 M rows), so M does not enter.  The three
    layer-1 shapes (Cin or Cout = 64) lose, 0.48-0.67x: one k-step and a
    64-wide output leave nothing for the epilogue to hide under."""
    del m
    return cin >= _ROUTE_MIN_C and cout >= _ROUTE_MIN_C


_ROUTE_MIN_C = 128


# ----------------------------------------------------------------------------
# Routing of the 1x1 stride-1 convs in training: stats-epilogue, dense or
# library forward; dense or library data gradient
# ----------------------------------------------------------------------------

# ``(pass, Cin, Cout)`` of the conv, pass in {"fwd", "dgrad"}: the shapes where
# the dense kernel (for dgrad: including the per-call weight transpose) beat the
# library by more than 5% in the same sitting at N = 1536
# (profiles/conv_bench_b1536.md, direct-to-LDS loop).  The forward entries are
# the three layer-1 shapes the stats route leaves on the plain forward; every
# other 1x1 stride-1 forward runs as conv1x1_stats.
_DENSE_ROUTE = {
    ("fwd", 64, 64): 1.26, ("fwd", 256, 64): 1.15, ("fwd", 64, 256): 1.63,
    ("dgrad", 64, 64): 1.31, ("dgrad", 256, 64): 1.61,
    ("dgrad", 64, 256): 1.11,
    ("dgrad", 256, 128): 1.43, ("dgrad", 512, 128): 1.36,
    ("dgrad", 128, 512): 1.45,
    ("dgrad", 512, 256): 1.24, ("dgrad", 1024, 256): 1.40,
    ("dgrad", 256, 1024): 1.38,
    ("dgrad", 1024, 512): 1.23, ("dgrad", 2048, 512): 1.35,
    ("dgrad", 512, 2048): 1.36,
}


def dense_route_enabled() -> bool:
    """``DWT_AMD_DENSE_ROUTE=0`` keeps every 1x1 dgrad and the layer-1 1x1
    forwards on the library.  Read when a conv is planned, in its forward;
    the backward follows the plan made then."""
    return os.environ.get("DWT_AMD_DENSE_ROUTE", "1") != "0"


def dense_route_ok(which: str, cin: int, cout: int) -> bool:
    """Whether the measured table sends this pass of a 1x1 stride-1 conv to
    the dense MFMA kernel."""
    return (which, cin, cout) in _DENSE_ROUTE


def mfma_1x1_usable(x: torch.Tensor, weight: torch.Tensor, conv=None) -> bool:
    """Whether the MFMA 1x1 kernels (stats-epilogue and dense forward, dense
    data gradient) can run this conv on this input: a 1x1 bf16 ``weight``,
    where given the plain stride-1 bias-free ``nn.Conv2d`` it belongs to
    (``MFMAConv2d`` has its own path), on CUDA bf16 channels_last ``x``, both
    channel counts a multiple of 8, and the extension loaded."""
    if conv is not None and (
            type(conv) is not nn.Conv2d or conv.bias is not None
            or conv.kernel_size != (1, 1) or conv.stride != (1, 1)
            or conv.padding != (0, 0) or conv.dilation != (1, 1)
            or conv.groups != 1):
        return False
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and weight.dim() == 4
            and tuple(weight.shape[1:]) == (x.shape[1], 1, 1)
            and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    n, cin, h, w = x.shape
    # H*W == 1: channels_last is ambiguous there; keep the library path
    if h * w == 1 or cin % 8 or weight.shape[0] % 8:
        return False
    from ..kernels import dispatch
    return dispatch.available()


class Conv1x1Plan(NamedTuple):
    """Which kernels one 1x1 stride-1 conv of a training step runs on."""
    fwd: str                # "stats", "dense" or "library"
    dgrad: str              # "dense" or "library"
    kind: Optional[str]     # of the norm site behind the conv: "bn", "whiten"
    g: int                  # that site's whitening group size (0 for BN)
    parts: int              # its domain branches


def _stats_rows_ok(n: int, h: int, w: int, parts: int) -> bool:
    """Each branch's rows are a whole number of the stats kernel's M tiles."""
    return parts >= 1 and n % parts == 0 \
        and (n // parts * h * w) % STATS_TILE_M == 0


def plan_conv1x1(n: int, cin: int, h: int, w: int, cout: int,
                 kind: Optional[str], g: int, parts: int) -> Conv1x1Plan:
    """The plan for a conv :func:`mfma_1x1_usable` accepts, from its sizes,
    the norm site behind it (``kind`` None: a site the stats kernel does not
    serve) and the two switches.  No tensors, no device: the measured tables
    and the NHWC norm kernels' channel ranges decide."""
    from ..kernels import hip_ops
    dense = dense_route_enabled()
    site_ok = (kind == "whiten" and g == 4
               and hip_ops.whiten_cl_supported(cout, g)) \
        or (kind == "bn" and hip_ops.bn_cl_supported(cout))
    if fused_conv_stats_enabled() and site_ok \
            and _stats_rows_ok(n, h, w, parts) \
            and conv_stats_shape_ok(n * h * w, cin, cout):
        fwd = "stats"
    elif dense and dense_route_ok("fwd", cin, cout):
        fwd = "dense"
    else:
        fwd = "library"
    dgrad = "dense" if dense and dense_route_ok("dgrad", cin, cout) \
        else "library"
    return Conv1x1Plan(fwd, dgrad, kind, g, parts)


def _site_kind(branches, cout: int):
    """``(kind, g)`` of the norm site ``branches`` for :func:`plan_conv1x1`."""
    from .whitening import WhiteningScaleShift, WTransform2d
    from .batch_norm import _DomainBatchNorm
    first = branches[0]
    if isinstance(first, (WhiteningScaleShift, WTransform2d)):
        wh = first.wh if isinstance(first, WhiteningScaleShift) else first
        return "whiten", cout // wh.num_groups
    if isinstance(first, _DomainBatchNorm):
        return "bn", 0
    return None, 0


class _Conv1x1Fn(torch.autograd.Function):
    """A 1x1 stride-1 bias-free conv run as its :class:`Conv1x1Plan` says.
    Forward: the persistent MFMA GEMM with the stats epilogue (then ``acc`` is
    the raw-sums accumulator, else None), the dense MFMA kernel, or the
    library.  Backward: dx on the dense kernel (dy @ W, with a per-call
    transposed copy of W) and dw from the library alone, or both from the
    library.  The plan is fixed here in the forward; the backward re-reads no
    switch.  On CPU tensors every plan runs as library/library: the kernels
    need the device."""

    stats_calls = 0         # forwards on the stats-epilogue kernel
    dense_fwd_calls = 0     # forwards on the dense kernel
    dense_dgrad_calls = 0   # data gradients on the dense kernel

    @staticmethod
    def forward(ctx, x, weight, plan, max_workgroups=0):
        if not x.is_cuda:
            # a hand-made plan on CPU tensors (the plumbing tests): the
            # kernels need the device, so both passes are the library's
            plan = plan._replace(fwd="library", dgrad="library")
        acc = None
        if plan.fwd == "stats":
            n, cin, h, w = x.shape
            cout = weight.shape[0]
            out = torch.empty(n, cout, h, w, device=x.device,
                              dtype=torch.bfloat16,
                              memory_format=torch.channels_last)
            acc = torch.zeros(stats_acc_numel(plan.kind, cout, plan.parts),
                              device=x.device, dtype=torch.float32)
            wgt = weight.detach().reshape(cout, cin).contiguous()
            _ext().conv1x1_stats(x, wgt, out, acc, _STATS_KINDS[plan.kind],
                                 plan.g, plan.parts, max_workgroups)
            _Conv1x1Fn.stats_calls += 1
            ctx.mark_non_differentiable(acc)
        elif plan.fwd == "dense":
            out = conv2d_fwd(x, weight.detach())
            _Conv1x1Fn.dense_fwd_calls += 1
        else:
            out = F.conv2d(x, weight)
        ctx.save_for_backward(x, weight)
        ctx.dense_dgrad = plan.dgrad == "dense"
        return out, acc

    @staticmethod
    def backward(ctx, dout, _dacc):
        x, weight = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        dense = ctx.dense_dgrad and need_dx
        if dense:
            dout = dout.contiguous(memory_format=torch.channels_last)
            dense_dx = conv2d_dgrad(dout, weight.detach(), x.shape)
            _Conv1x1Fn.dense_dgrad_calls += 1
        dx, dw, _ = torch.ops.aten.convolution_backward(
            dout, x, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [need_dx and not dense, True, False])
        return dense_dx if dense else dx, dw, None, None


def _plan_of(conv, x: torch.Tensor, branches, training: bool):
    """The plan of ``conv`` on ``x`` in front of the norm site ``branches``,
    or None where the MFMA 1x1 kernels cannot run it (or not training)."""
    if not training or not mfma_1x1_usable(x, conv.weight, conv):
        return None
    n, cin, h, w = x.shape
    cout = conv.out_channels
    return plan_conv1x1(n, cin, h, w, cout, *_site_kind(branches, cout),
                        len(branches))


def conv1x1_routed(conv, x: torch.Tensor, branches, training: bool):
    """``(conv(x), stats_acc)`` for a conv feeding the norm site ``branches``:
    the model's one entry to the routing.  In training, a conv the MFMA 1x1
    kernels can run goes through :class:`_Conv1x1Fn` with its plan, and
    ``stats_acc`` (not None after a stats-epilogue forward) goes to
    ``norm_site``.  Everything else, an all-library plan included, is the
    module's own forward and ``None``."""
    plan = _plan_of(conv, x, branches, training)
    if plan is None or (plan.fwd == "library" and plan.dgrad == "library"):
        return conv(x), None
    return _Conv1x1Fn.apply(x, conv.weight, plan)


def conv_stats_route(conv, x: torch.Tensor, branches, training: bool):
    """``(kind, g, parts)`` when :func:`conv1x1_routed` would run ``conv`` on
    the stats-epilogue forward, else ``None``: the question without the conv,
    answered by the same plan."""
    plan = _plan_of(conv, x, branches, training)
    if plan is None or plan.fwd != "stats":
        return None
    return plan.kind, plan.g, plan.parts


def conv1x1_stats(x: torch.Tensor, weight: torch.Tensor, kind: str,
                  g: int = 4, parts: int = 3, max_workgroups: int = 0):
    """1x1 stride-1 bias-free conv of channels_last bf16 ``x`` that also
    returns the raw statistics accumulator of the norm site that follows
    (``kind`` "bn" or "whiten" with g = 4; ``parts`` equal batch ranges, each
    a multiple of 128 positions).  Hand ``acc`` to ``norm_site(stats_acc=)``.

    Where the kernel does not apply (another device, dtype, layout or group
    size, rows per branch no multiple of 128) this is ``(F.conv2d(x, weight),
    None)``: the norm site then takes its own statistics.
    """
    assert kind in _STATS_KINDS, kind
    if (kind == "whiten" and g != 4) or not mfma_1x1_usable(x, weight):
        return F.conv2d(x, weight), None
    n, cin, h, w = x.shape
    if not _stats_rows_ok(n, h, w, parts):
        return F.conv2d(x, weight), None
    # the stats forward whatever its switch and shape table say; the data
    # gradient as planned
    plan = plan_conv1x1(n, cin, h, w, weight.shape[0], kind, g, parts)
    return _Conv1x1Fn.apply(x, weight, plan._replace(fwd="stats"),
                            max_workgroups)


def conv2d_dgrad(dy: torch.Tensor, weight: torch.Tensor, in_shape,
                 stride: int = 1, padding: int = 0) -> torch.Tensor:
    """dx for an NHWC conv: implicit GEMM over dy with the weight permuted to
    [ci][r][s][co] (tiny host-side permute per call)."""
    n, cin, h, w = in_shape
    cout, _, kh, kw = weight.shape
    p, q = dy.shape[2], dy.shape[3]
    dyc = dy.contiguous(memory_format=torch.channels_last)
    # CL storage of weight is [co][kh][kw][ci]; build [ci][kh][kw][co]
    wv = weight.permute(0, 2, 3, 1)              # (Cout, KH, KW, Cin), contig view of CL
    wd = wv.permute(3, 1, 2, 0).contiguous()     # (Cin, KH, KW, Cout)
    dx = torch.empty(n, cin, h, w, device=dy.device, dtype=torch.bfloat16,
                     memory_format=torch.channels_last)
    _ext().mfma_conv2d_dgrad(dyc, wd, dx, n, h, w, cin, p, q, cout,
                             kh, kw, stride, padding)
    return dx


class _MFMAConv2dFn(torch.autograd.Function):
    """Training conv on the hand-written MFMA kernels: implicit-GEMM fwd,
    dgrad (skipped when the input needs no grad, e.g. the stem) and wgrad.
    DWT_AMD_WGRAD=aten routes wgrad through the library as an escape hatch."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding):
        out = conv2d_fwd(x, weight, bias=bias, stride=stride, padding=padding)
        ctx.save_for_backward(x, weight)
        ctx.meta = (stride, padding, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        stride, padding, has_bias = ctx.meta
        dout = dout.contiguous(memory_format=torch.channels_last)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dout, weight, x.shape, stride=stride,
                              padding=padding)
        if os.environ.get("DWT_AMD_WGRAD") == "aten":
            _, dw, db = torch.ops.aten.convolution_backward(
                dout, x, weight, [weight.shape[0]] if has_bias else None,
                [stride, stride], [padding, padding], [1, 1], False, [0, 0], 1,
                [False, True, has_bias])
        else:
            dw = conv2d_wgrad(dout, x, tuple(weight.shape), stride=stride,
                              padding=padding)
            db = dout.sum(dim=(0, 2, 3)).to(dout.dtype) if has_bias else None
        return dx, dw, db, None, None


class MFMAConv2d(nn.Conv2d):
    """Conv2d on the hand-written MFMA kernels (fwd + dgrad) when running
    bf16 channels_last on GPU; F.conv2d otherwise.  Enable in the models with
    DWT_AMD_CONV=hip."""

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and (x.shape[1] >= 8 or x.shape[1] == 3) \
                and x.is_contiguous(memory_format=torch.channels_last) \
                and self.stride[0] == self.stride[1] \
                and self.padding[0] == self.padding[1]:
            from ..kernels import dispatch
            if dispatch.available():
                return _MFMAConv2dFn.apply(x, self.weight, self.bias,
                                           self.stride[0], self.padding[0])
        return super().forward(x)


def _wgrad_patches_reference(x_nhwc, shape, stride, padding, npq_pad=None,
                             dtype=torch.float64):
    """CPU/torch reference of the kernel's wgrad B-operand gather: returns
    Bt [(r,s,ci), k=npq] built with EXACTLY the kernel's index decode
    (mfma_conv.hip::load_b_wgrad) — used by the index-math test."""
    n, h, w, cin = x_nhwc.shape
    cout, _, kh, kw = shape
    p = (h + 2 * padding - kh) // stride + 1
    q = (w + 2 * padding - kw) // stride + 1
    npq = n * p * q
    k_tot = npq_pad or npq
    cols = torch.zeros(kh * kw * cin, k_tot, dtype=dtype)
    ks = torch.arange(npq)
    qq = ks % q
    pp = (ks // q) % p
    nn = ks // (q * p)
    for r in range(kh):
        for s in range(kw):
            hh = pp * stride - padding + r
            ww = qq * stride - padding + s
            ok = (hh >= 0) & (hh < h) & (ww >= 0) & (ww < w)
            vals = torch.zeros(npq, cin, dtype=dtype)
            vals[ok] = x_nhwc[nn[ok], hh[ok].clamp(0), ww[ok].clamp(0)].to(dtype)
            for ci in range(cin):
                cols[(r * kw + s) * cin + ci, :npq] = vals[:, ci]
    return cols


def conv2d_wgrad(dy: torch.Tensor, x: torch.Tensor, weight_shape,
                 stride: int = 1, padding: int = 0) -> torch.Tensor:
    """dw for an NHWC conv on the split-K MFMA wgrad kernel: both operands
    consumed K-major straight from their NHWC storage (LDS-transposed in
    kernel), K = N*P*Q split across the grid into an fp32 workspace;
    output IS the channels_last weight storage [co][r][s][ci]."""
    cout, cin, kh, kw = weight_shape
    n, _, p, q = dy.shape
    assert cout % 8 == 0, "wgrad kernel needs Cout % 8 == 0"
    dyc = dy.contiguous(memory_format=torch.channels_last)
    dw = torch.empty(weight_shape, device=dy.device, dtype=torch.bfloat16,
                     memory_format=torch.channels_last)
    ws = torch.zeros(cout * kh * kw * cin, device=dy.device,
                     dtype=torch.float32)
    xc = x.contiguous(memory_format=torch.channels_last)
    _ext().mfma_conv2d_wgrad(dyc, xc, dw, ws, n, x.shape[2], x.shape[3], cin,
                             p, q, cout, kh, kw, stride, padding)
    return dw
