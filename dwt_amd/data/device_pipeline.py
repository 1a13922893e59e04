"""Device-side input pipeline: resized uint8 HWC frames -> the model's batch.

The loaders hand over what a decoder produces anyway — uint8 ``[H, W, 3]``
frames at ``img_resize`` — and one HIP kernel
(``kernels/src/input_pipeline.hip``) writes the whole
``(source, target, target_aug)`` batch in the model's dtype and in NHWC:
crop, flip, the reference's random affine with the reference's border
constant, and normalization.  No host float work, ``cat``, cast or layout
conversion is left.

Semantics, in the loaders' order (RandomCrop, RandomHorizontalFlip, ToTensor,
``random_affine_augmentation``, Normalize)::

    crop(r, c) = images[src, top + r, left + (flip ? cw-1-c : c), :] / 255
    plain :  out = (crop(r, c) - mean) / std
    affine:  p = inv_affine @ (r, c); 0 outside [0, ch-1] x [0, cw-1]
             (scipy mode="constant", cval=0), else bilinear(crop, p);
             then the same normalization

The reference's ``gaussian_blur`` at sigma 0.1 has kernel size 1 — the
identity — and is omitted, as ``augment.gpu_target_views`` already does.

``assemble_views_reference`` is the pure-torch statement of these semantics:
the oracle for the GPU tests and the path CPU runs take.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple, Union

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_DTYPES = (torch.float32, torch.bfloat16)


class ViewParams(NamedTuple):
    """Host-side table of ``n`` views (CPU tensors)."""
    top: torch.Tensor         # int32 [n]
    left: torch.Tensor        # int32 [n]
    flip: torch.Tensor        # bool  [n]
    inv_affine: torch.Tensor  # fp32  [n, 4], inverse of the forward matrix
    affine: torch.Tensor      # bool  [n]


def _pair(crop) -> Tuple[int, int]:
    if isinstance(crop, int):
        return crop, crop
    ch, cw = crop
    return int(ch), int(cw)


def draw_view_params(n: int, src_hw, crop, flip_p: float = 0.5,
                     affine_std: float = 0.1,
                     generator: torch.Generator = None,
                     aug: bool = False) -> ViewParams:
    """Draw ``n`` views on the host from a CPU generator: a uniform crop
    position, and for augmented views a flip with probability ``flip_p`` and
    the matrix ``I + N(0, affine_std)``, like ``random_affine_augmentation``
    stored as fp32, inverted in closed form in fp64 and stored as fp32.
    Plain views (``aug=False``: the reference's ``data_transform``) have no
    flip and no affine."""
    hs, ws = src_hw
    ch, cw = _pair(crop)
    if ch > hs or cw > ws:
        raise ValueError(f"crop {ch}x{cw} does not fit frames of {hs}x{ws}")
    top = torch.randint(0, hs - ch + 1, (n,), generator=generator).to(torch.int32)
    left = torch.randint(0, ws - cw + 1, (n,), generator=generator).to(torch.int32)
    if not aug:
        return ViewParams(top, left, torch.zeros(n, dtype=torch.bool),
                          torch.tensor([1.0, 0.0, 0.0, 1.0]).repeat(n, 1),
                          torch.zeros(n, dtype=torch.bool))
    flip = torch.rand(n, generator=generator) < flip_p
    m = torch.eye(2) + affine_std * torch.randn(n, 2, 2, generator=generator)
    m = m.to(torch.float64)
    a, b, c, d = m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1]
    det = a * d - b * c
    inv = torch.stack((d, -b, -c, a), dim=1) / det[:, None]
    return ViewParams(top, left, flip, inv.to(torch.float32),
                      torch.ones(n, dtype=torch.bool))


def _host_table(x, n, dtype, name):
    t = torch.as_tensor(x).detach().to("cpu")
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"{name} must have one entry per output image "
                         f"({n}), got shape {tuple(t.shape)}")
    return t.to(dtype)


def _validate(images_u8, src_index, top, left, flip, inv_affine, affine, crop,
              mean, std, dtype):
    """Host-side checks; returns the normalized CPU tables."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8:
        raise ValueError("images must be a uint8 tensor")
    if images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError(f"images must be [N, H, W, 3], got {tuple(images_u8.shape)}")
    if not images_u8.is_contiguous():
        raise ValueError("images must be contiguous")
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be float32 or bfloat16, got {dtype}")
    n_in, hs, ws, _ = images_u8.shape
    ch, cw = _pair(crop)
    if n_in < 1 or ch < 1 or cw < 1 or ch > hs or cw > ws:
        raise ValueError(f"crop {ch}x{cw} does not fit {n_in} frames of {hs}x{ws}")
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError("mean and std take three values each, std non-zero")
    src_index = torch.as_tensor(src_index)
    if src_index.dim() != 1:
        raise ValueError("src_index must be one-dimensional")
    n = src_index.shape[0]
    src_index = _host_table(src_index, n, torch.int64, "src_index")
    top = _host_table(top, n, torch.int64, "top")
    left = _host_table(left, n, torch.int64, "left")
    flip = _host_table(flip, n, torch.bool, "flip")
    affine = _host_table(affine, n, torch.bool, "affine")
    inv = torch.as_tensor(inv_affine).detach().to("cpu", torch.float32)
    if inv.numel() != 4 * n or inv.shape[0] != n:
        raise ValueError(f"inv_affine must be [{n}, 4] or [{n}, 2, 2], "
                         f"got {tuple(inv.shape)}")
    inv = inv.reshape(n, 4)
    if not bool(torch.isfinite(inv).all()):
        raise ValueError("inv_affine must be finite")
    if n and (int(src_index.min()) < 0 or int(src_index.max()) >= n_in):
        raise ValueError(f"src_index must lie in [0, {n_in})")
    if n and (int(top.min()) < 0 or int(top.max()) > hs - ch):
        raise ValueError(f"top must lie in [0, {hs - ch}]")
    if n and (int(left.min()) < 0 or int(left.max()) > ws - cw):
        raise ValueError(f"left must lie in [0, {ws - cw}]")
    return src_index, top, left, flip, inv, affine, (ch, cw)


def assemble_views_reference(images_u8, src_index, top, left, flip, inv_affine,
                             affine, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                             dtype=torch.float32) -> torch.Tensor:
    """Pure-torch statement of the kernel's semantics, computed on the CPU in
    fp32 and rounded once at the end.  Returns ``[N_out, 3, ch, cw]`` in
    channels_last on the CPU."""
    src_index, top, left, flip, inv, affine, (ch, cw) = _validate(
        images_u8, src_index, top, left, flip, inv_affine, affine, crop,
        mean, std, dtype)
    images = images_u8.detach().to("cpu")
    n = src_index.shape[0]
    mean_t = torch.tensor(mean, dtype=torch.float32)
    std_t = torch.tensor(std, dtype=torch.float32)
    out = torch.empty(n, ch, cw, 3, dtype=torch.float32)
    rr, cc = torch.meshgrid(torch.arange(ch, dtype=torch.float32),
                            torch.arange(cw, dtype=torch.float32), indexing="ij")
    for i in range(n):
        t, l = int(top[i]), int(left[i])
        view = images[int(src_index[i]), t:t + ch, l:l + cw]      # [ch, cw, 3]
        if bool(flip[i]):
            view = view.flip(1)
        view = view.to(torch.float32) / 255.0
        if bool(affine[i]):
            a = inv[i]
            pr = a[0] * rr + a[1] * cc
            pc = a[2] * rr + a[3] * cc
            inside = (pr >= 0) & (pr <= ch - 1) & (pc >= 0) & (pc <= cw - 1)
            r0 = pr.floor().clamp(0, ch - 1)
            c0 = pc.floor().clamp(0, cw - 1)
            fr = (pr - r0)[..., None]
            fc = (pc - c0)[..., None]
            r0, c0 = r0.long(), c0.long()
            r1 = (r0 + 1).clamp(max=ch - 1)
            c1 = (c0 + 1).clamp(max=cw - 1)
            t0 = view[r0, c0] + fc * (view[r0, c1] - view[r0, c0])
            t1 = view[r1, c0] + fc * (view[r1, c1] - view[r1, c0])
            view = torch.where(inside[..., None], t0 + fr * (t1 - t0),
                               torch.zeros(()))
        out[i] = (view - mean_t) / std_t
    return out.to(dtype).permute(0, 3, 1, 2)


def _upload_tables(src_index, top, left, flip, inv, affine, device):
    """One pinned host buffer, one transfer: four int32 columns, then the
    fp32 matrices (their bits) — returned as views of the device copy."""
    n = src_index.shape[0]
    host = torch.empty(8 * n, dtype=torch.int32,
                       pin_memory=torch.cuda.is_available())
    cols = host[:4 * n].view(4, n)
    cols[0] = src_index
    cols[1] = top
    cols[2] = left
    cols[3] = flip.to(torch.int32) + 2 * affine.to(torch.int32)
    host[4 * n:].view(torch.float32).view(n, 4).copy_(inv)
    dev = host.to(device, non_blocking=True)
    d = dev[:4 * n].view(4, n)
    return d[0], d[1], d[2], d[3], dev[4 * n:].view(torch.float32).view(n, 4)


def assemble_views(images_u8, src_index, top, left, flip, inv_affine, affine,
                   crop, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                   dtype=torch.float32) -> torch.Tensor:
    """Write ``N_out`` views of the uint8 frames ``images_u8``
    ``[N_in, Hs, Ws, 3]`` as one ``[N_out, 3, ch, cw]`` channels_last batch of
    ``dtype`` on the frames' device.

    Row ``n`` crops frame ``src_index[n]`` at ``(top[n], left[n])``, flips it
    if ``flip[n]``, applies the affine whose inverse is ``inv_affine[n]`` if
    ``affine[n]``, and normalizes.  The tables are host values (sequences or
    CPU tensors) and are checked before anything is launched (``ValueError``).
    On a GPU this is one launch of the HIP kernel; on the CPU it is
    ``assemble_views_reference``."""
    tables = _validate(images_u8, src_index, top, left, flip, inv_affine,
                       affine, crop, mean, std, dtype)
    if not images_u8.is_cuda:
        return assemble_views_reference(images_u8, src_index, top, left, flip,
                                        inv_affine, affine, crop, mean, std,
                                        dtype)
    from ..kernels import dispatch
    if not dispatch.available():
        dispatch.require_or_warn("assemble_views")
        return assemble_views_reference(
            images_u8, src_index, top, left, flip, inv_affine, affine, crop,
            mean, std, dtype).to(images_u8.device)
    src_index, top, left, flip, inv, affine, (ch, cw) = tables
    n = src_index.shape[0]
    out = torch.empty((n, 3, ch, cw), dtype=dtype, device=images_u8.device,
                      memory_format=torch.channels_last)
    if n == 0:
        return out
    with torch.cuda.device(images_u8.device):
        d_src, d_top, d_left, d_flags, d_inv = _upload_tables(
            src_index, top, left, flip, inv, affine, images_u8.device)
        dispatch.ext().assemble_views(
            images_u8, d_src, d_top, d_left, d_flags, d_inv, out,
            [float(m) for m in mean], [float(s) for s in std])
    return out


class DeviceBatcher:
    """Turns the loaders' uint8 frame batches into model batches, one launch
    each and no ``cat``: the frames are copied (``non_blocking``) into one
    staging buffer on the device and every stream is a set of rows of the
    view table over that buffer."""

    def __init__(self, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 dtype=torch.float32, device="cpu", seed: int = 0,
                 flip_p: float = 0.5, affine_std: float = 0.1):
        self.crop = _pair(crop)
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.dtype = dtype
        self.device = torch.device(device)
        self.flip_p = flip_p
        self.affine_std = affine_std
        self.generator = torch.Generator().manual_seed(seed)
        self._staging = None

    def _stage(self, *batches: torch.Tensor) -> torch.Tensor:
        for b in batches:
            if b.dtype != torch.uint8 or b.dim() != 4 or b.shape[3] != 3:
                raise ValueError("DeviceBatcher takes uint8 [B, H, W, 3] "
                                 f"frames, got {b.dtype} {tuple(b.shape)}")
            if b.shape[1:] != batches[0].shape[1:]:
                raise ValueError("all streams must share one frame size")
        n = sum(b.shape[0] for b in batches)
        shape = (n,) + tuple(batches[0].shape[1:])
        if len(batches) == 1 and batches[0].device == self.device \
                and batches[0].is_contiguous():
            return batches[0]
        if self._staging is None or self._staging.shape[1:] != shape[1:] \
                or self._staging.shape[0] < n:
            self._staging = torch.empty(shape, dtype=torch.uint8,
                                        device=self.device)
        staging = self._staging[:n]
        at = 0
        for b in batches:
            staging[at:at + b.shape[0]].copy_(b, non_blocking=True)
            at += b.shape[0]
        return staging

    def _draw(self, n, src_hw, aug):
        return draw_view_params(n, src_hw, self.crop, self.flip_p,
                                self.affine_std, self.generator, aug=aug)

    def _assemble(self, frames, src_index, views: Sequence[ViewParams]):
        return assemble_views(
            frames, src_index,
            torch.cat([v.top for v in views]),
            torch.cat([v.left for v in views]),
            torch.cat([v.flip for v in views]),
            torch.cat([v.inv_affine for v in views]),
            torch.cat([v.affine for v in views]),
            self.crop, self.mean, self.std, self.dtype)

    def train_batch(self, src_u8: torch.Tensor, tgt_u8: torch.Tensor) -> torch.Tensor:
        """``[Bs + 2 Bt, 3, ch, cw]``: a plain view of every source frame, a
        plain view of every target frame, and the target duplicate with its
        own crop, flip and affine."""
        bs, bt = src_u8.shape[0], tgt_u8.shape[0]
        frames = self._stage(src_u8, tgt_u8)
        hw = frames.shape[1:3]
        views = [self._draw(bs, hw, False), self._draw(bt, hw, False),
                 self._draw(bt, hw, True)]
        tgt_rows = torch.arange(bs, bs + bt)
        src_index = torch.cat((torch.arange(bs), tgt_rows, tgt_rows))
        return self._assemble(frames, src_index, views)

    def eval_batch(self, u8: torch.Tensor, streams: int = 1) -> torch.Tensor:
        """One random crop per frame (the reference's test transform);
        ``streams=3`` repeats that view in all three streams, which is what
        the statistics re-estimation pass feeds the model."""
        if streams not in (1, 3):
            raise ValueError("streams must be 1 or 3")
        frames = self._stage(u8)
        b = u8.shape[0]
        view = self._draw(b, frames.shape[1:3], False)
        return self._assemble(frames, torch.arange(b).repeat(streams),
                              [view] * streams)
