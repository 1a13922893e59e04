"""Folded target-domain inference for the DWT-ResNet.

At eval every norm site is an affine map with fixed coefficients: whitening
is ``gamma * W (x - m) + beta`` with a block-diagonal ``W`` computed from the
running covariance, domain BN is the diagonal case.  Each site sits directly
behind a bias-free conv, so it folds exactly into that conv's weight plus a
bias, and the whole target-branch network becomes
``conv + bias [+ identity] [+ ReLU]`` — one launch per conv, no norm kernels,
no matrix function per call.

``fold_resnet(model)`` takes a snapshot of a ``ResNetDWT``; after more
training it has to be made again.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import functional as Fdwt
from ..ops import oracle
from ..ops.batch_norm import _DomainBatchNorm
from ..ops.pooling import global_avg_pool, max_pool2d
from ..ops.whitening import WhiteningScaleShift, WTransform2d

NS_ITERS = 7   # WhitenMulti's Newton-Schulz iteration count (its cfg default)


def _site_affine(branch: nn.Module, gamma: Optional[torch.Tensor],
                 beta: Optional[torch.Tensor]):
    """fp64 ``(A, shift)`` of the eval-time site ``y = A x + shift``; ``A`` is
    (C, C) block-diagonal for whitening and a (C,) diagonal for BN."""
    if isinstance(branch, (WhiteningScaleShift, WTransform2d)):
        wh = branch.wh if isinstance(branch, WhiteningScaleShift) else branch
        c = wh.num_features
        cov_s = oracle.shrink_cov(wh.running_variance.detach().double(), wh.eps)
        if wh.mode == "chol":
            wmat, _ = Fdwt.matfn_chol_forward(cov_s)
        else:
            wmat, _ = Fdwt.matfn_ns_forward(cov_s, NS_ITERS)
        a = torch.block_diag(*wmat)                       # (C, C)
        mean = wh.running_mean.detach().double().reshape(c)
    elif isinstance(branch, (_DomainBatchNorm, nn.modules.batchnorm._BatchNorm)):
        c = branch.num_features
        a = torch.rsqrt(branch.running_var.detach().double() + branch.eps)
        mean = branch.running_mean.detach().double().reshape(c)
    else:
        raise TypeError(f"unsupported norm branch type {type(branch)}")
    g = gamma.detach().double().reshape(c).to(a.device) if gamma is not None \
        else torch.ones(c, dtype=torch.float64, device=a.device)
    b = beta.detach().double().reshape(c).to(a.device) if beta is not None \
        else torch.zeros(c, dtype=torch.float64, device=a.device)
    if a.dim() == 2:
        a = g[:, None] * a
        shift = b - a @ mean
    else:
        a = g * a
        shift = b - a * mean
    return a, shift


def fold_norm_into_conv(conv_weight: torch.Tensor, branch: nn.Module,
                        gamma: Optional[torch.Tensor],
                        beta: Optional[torch.Tensor]
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fold the eval-time norm site ``branch`` (+ shared ``gamma`` / ``beta``)
    into the bias-free conv in front of it.

    With ``A = diag(gamma) . blockdiag(wmat)`` (whitening; ``wmat`` computed
    exactly as eval computes it) or ``A = diag(gamma / sqrt(var + eps))``
    (BN): ``weight' = A . weight`` over Cout, ``bias' = beta - A . mean``.
    Computed in fp64; the weight comes back in ``conv_weight``'s dtype,
    channels_last, the bias in fp32.
    """
    w = conv_weight.detach().double()
    a, shift = _site_affine(branch, gamma, beta)
    a, shift = a.to(w.device), shift.to(w.device)
    if a.dim() == 2:
        wf = torch.einsum("oc,cikl->oikl", a, w)
    else:
        wf = a.reshape(-1, 1, 1, 1) * w
    wf = wf.to(conv_weight.dtype).contiguous(memory_format=torch.channels_last)
    return wf, shift.float()


class _FoldedConv(nn.Module):
    """conv + bias with frozen tensors; stride / padding kept as ints."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, stride: int,
                 padding: int):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.bias = nn.Parameter(bias, requires_grad=False)
        self.stride = stride
        self.padding = padding

    def forward(self, x, relu: bool = False, residual=None, fused: bool = False,
                route: bool = True):
        if fused:
            from ..ops import mfma
            return mfma.conv2d_fused_fwd(x, self.weight, self.bias,
                                         stride=self.stride,
                                         padding=self.padding, relu=relu,
                                         residual=residual, route=route)
        w = self.weight
        if w.shape[1] != x.shape[1]:        # stem weight padded 3 -> 4
            w = w[:, :x.shape[1]]
        out = F.conv2d(x, w, self.bias.to(x.dtype), self.stride, self.padding)
        if residual is not None:
            out = out + residual
        return torch.relu(out) if relu else out


class _FoldedBlock(nn.Module):
    def __init__(self, conv1, conv2, conv3, downsample=None):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = conv1, conv2, conv3
        # nn.Sequential keeps the source name `downsample.0`
        self.downsample = nn.Sequential(downsample) if downsample is not None \
            else None

    def forward(self, x, fused: bool = False, route: bool = True):
        kw = dict(fused=fused, route=route)
        identity = x
        if self.downsample is not None:
            identity = self.downsample[0](x, relu=False, **kw)
        out = self.conv1(x, relu=True, **kw)
        out = self.conv2(out, relu=True, **kw)
        return self.conv3(out, relu=True, residual=identity, **kw)


class _FoldedFc(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)
        self.bias = nn.Parameter(bias, requires_grad=False)


def _conv_geom(conv: nn.Conv2d):
    assert conv.bias is None and conv.groups == 1 and conv.dilation == (1, 1) \
        and conv.stride[0] == conv.stride[1] \
        and conv.padding[0] == conv.padding[1], "conv shape not foldable"
    return conv.stride[0], conv.padding[0]


class FoldedResNetDWT(nn.Module):
    """The target-branch (or any one branch's) eval network of a ``ResNetDWT``
    with every norm site folded into its conv.

    ``convs`` maps the source module names (``conv1``, ``layerL.B.conv{1,2,3}``,
    ``layerL.0.downsample.0``) to ``(weight, bias, stride, padding)``; build it
    with :func:`fold_resnet` or :func:`checkpoint.load_folded`.

    On the GPU in bf16 with the HIP extension every conv goes through
    ``ops.mfma.conv2d_fused_fwd``, NHWC end to end: one launch of the MFMA
    kernel with the bias / residual / ReLU epilogue, except the shapes its
    measured routing table sends to the library conv + elementwise op
    (``self.route = False`` keeps every conv on the kernel).  Everywhere else
    it is ``F.conv2d`` + add + relu on the same tensors.
    """

    def __init__(self, layers: Sequence[int], convs: dict, fc_weight, fc_bias,
                 meta: Optional[dict] = None):
        super().__init__()
        self.layers = [int(v) for v in layers]
        self.meta = dict(meta or {})
        self.conv1 = _FoldedConv(*convs["conv1"])      # first parameter: model dtype
        for li, nblocks in enumerate(self.layers, start=1):
            blocks: List[nn.Module] = []
            for b in range(nblocks):
                pre = f"layer{li}.{b}"
                ds = convs.get(f"{pre}.downsample.0")
                blocks.append(_FoldedBlock(
                    _FoldedConv(*convs[f"{pre}.conv1"]),
                    _FoldedConv(*convs[f"{pre}.conv2"]),
                    _FoldedConv(*convs[f"{pre}.conv3"]),
                    _FoldedConv(*ds) if ds is not None else None))
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        self.fc_out = _FoldedFc(fc_weight, fc_bias)
        self.num_classes = int(fc_weight.shape[0])
        self.route = True
        self.eval()

    def conv_specs(self) -> dict:
        """``{name: (weight, bias, stride, padding)}`` — what the constructor
        takes (the checkpoint writer's view of the model)."""
        out = {}
        for name, m in self.named_modules():
            if isinstance(m, _FoldedConv):
                out[name] = (m.weight.data, m.bias.data, m.stride, m.padding)
        return out

    def _use_kernel(self, x: torch.Tensor) -> bool:
        if not (x.is_cuda and x.dtype == torch.bfloat16
                and self.conv1.weight.dtype == torch.bfloat16):
            return False
        from ..kernels import dispatch
        return dispatch.available()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.conv1.weight.dtype)
        fused = self._use_kernel(x)
        if fused:
            x = x.contiguous(memory_format=torch.channels_last)
        x = self.conv1(x, relu=True, fused=fused, route=self.route)
        x = max_pool2d(x, 3, 2, 1)
        for li in range(1, len(self.layers) + 1):
            for block in getattr(self, f"layer{li}"):
                x = block(x, fused=fused, route=self.route)
        x = global_avg_pool(x)
        if fused:
            from ..ops import mfma
            return mfma.mfma_gemm(x, self.fc_out.weight, bias=self.fc_out.bias)
        return F.linear(x, self.fc_out.weight, self.fc_out.bias.to(x.dtype))


def _pad_stem(weight: torch.Tensor) -> torch.Tensor:
    """Cin 3 -> 4 with a zero channel, once: the kernel's stem path reads
    NHWC C=4 pixels (the input is padded per batch)."""
    if weight.shape[1] != 3:
        return weight
    w4 = weight.new_zeros(weight.shape[0], 4, *weight.shape[2:])
    w4[:, :3] = weight
    return w4.contiguous(memory_format=torch.channels_last)


def fold_resnet(model: nn.Module, branch: int = 1) -> FoldedResNetDWT:
    """Snapshot ``model`` (a ``ResNetDWT``, possibly inside a data-parallel
    wrapper) as a :class:`FoldedResNetDWT`.  ``branch`` indexes each site's
    ``[bns, bnt, bnt_aug]``; 1 is the target branch eval uses."""
    while hasattr(model, "module") and isinstance(model.module, nn.Module):
        model = model.module
    if not 0 <= branch <= 2:
        raise ValueError(f"branch must be 0, 1 or 2 (got {branch})")

    def pick(owner, names):
        return getattr(owner, names[branch])

    def fold(conv, site, gamma, beta):
        stride, padding = _conv_geom(conv)
        w, b = fold_norm_into_conv(conv.weight, site, gamma, beta)
        return (w, b, stride, padding)

    convs = {}
    w, b, s, p = fold(model.conv1, pick(model, ("bns1", "bnt1", "bnt1_aug")),
                      model.gamma1, model.beta1)
    convs["conv1"] = (_pad_stem(w), b, s, p)
    layers = []
    for li in range(1, 5):
        stage = getattr(model, f"layer{li}")
        layers.append(len(stage))
        for bi, blk in enumerate(stage):
            pre = f"layer{li}.{bi}"
            for k in (1, 2, 3):
                site = pick(blk, (f"bns{k}", f"bnt{k}", f"bnt{k}_aug"))
                convs[f"{pre}.conv{k}"] = fold(
                    getattr(blk, f"conv{k}"), site,
                    getattr(blk, f"gamma{k}"), getattr(blk, f"beta{k}"))
            if blk.downsample is not None:
                assert len(blk.downsample) == 1, "downsample is one conv"
                site = pick(blk, ("downsample_bns", "downsample_bnt",
                                  "downsample_bnt_aug"))
                convs[f"{pre}.downsample.0"] = fold(
                    blk.downsample[0], site, blk.downsample_gamma,
                    blk.downsample_beta)
    fc = model.fc_out
    dtype = model.conv1.weight.dtype
    meta = dict(layers=layers, num_classes=fc.out_features, branch=branch,
                whiten_mode=getattr(model, "whiten_mode", "chol"),
                dtype=str(dtype).replace("torch.", ""))
    return FoldedResNetDWT(layers, convs, fc.weight.detach().clone(),
                           fc.bias.detach().float().clone(), meta)
