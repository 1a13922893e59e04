"""The HIP `assemble_views` kernel against the pure-torch reference on the CPU,
and the engine driven by a `DeviceBatcher` on the GPU.

Tolerances (derived, not fitted): fp32 plain rows 1e-5 (one fma against the
reference's divide-subtract-divide, values up to ~2.7); fp32 affine rows 1e-4
(the coordinate is a two-term fp32 dot product of magnitude <= 32, error about
6e-6 px, slope <= 1 per px, division by std >= 0.224); bf16
`|out - ref| <= 2^-8 |ref| + 1e-4` (one rounding is at most 2^-9 relative;
2^-8 leaves one ulp)."""
import types

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from dwt_amd.data import (DeviceBatcher, SyntheticOfficeHome, assemble_views,
                          assemble_views_reference, draw_view_params)

pytestmark = pytest.mark.gpu

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]
FORWARD = ([[1.07, 0.05], [-0.08, 0.93]], [[1.19, -0.13], [0.09, 0.88]])
IDENT = [1.0, 0.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _frames(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def _inv32(forward):
    m = np.float32(forward).astype(np.float64)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    inv = np.array([m[1, 1], -m[0, 1], -m[1, 0], m[0, 0]]) / det
    return inv.astype(np.float32).tolist()


def _edge_margin(inv32, crop):
    """fp64 distance of the source coordinates to the frame edges; pixel
    (0, 0) maps to exactly 0 in any arithmetic and is left out."""
    a = np.float64(inv32)
    rr, cc = np.meshgrid(np.arange(crop), np.arange(crop), indexing="ij")
    pr, pc = a[0] * rr + a[1] * cc, a[2] * rr + a[3] * cc
    dist = np.minimum(np.minimum(np.abs(pr), np.abs(pr - (crop - 1))),
                      np.minimum(np.abs(pc), np.abs(pc - (crop - 1))))
    dist[0, 0] = np.inf
    return dist.min()


def _table(n_in, hs, ws, crop, n_out):
    """Rows mixing a repeated frame, crop positions at 0 and at their maxima,
    flip on and off, and no affine / each of the two matrices."""
    tmax, lmax = hs - crop, ws - crop
    kinds = [None, FORWARD[0], FORWARD[1]]
    t = dict(src_index=[], top=[], left=[], flip=[], inv_affine=[], affine=[])
    for i in range(n_out):
        t["src_index"].append((i // 2) % n_in)       # every frame twice
        t["top"].append((0, tmax, tmax // 2)[i % 3])
        t["left"].append((lmax, 0, lmax // 2)[(i // 2) % 3])
        t["flip"].append(i % 2 == 1)
        kind = kinds[(i + i // 3) % 3]
        t["affine"].append(kind is not None)
        t["inv_affine"].append(IDENT if kind is None else _inv32(kind))
    return t


def _check(out, ref, affine, dtype):
    assert out.shape == ref.shape
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert out.dtype == dtype
    out = out.float().cpu()
    # the bf16 reference is already rounded: compare with its fp32 original
    err = (out - ref).abs()
    if dtype == torch.bfloat16:
        bound = 2.0 ** -8 * ref.abs() + 1e-4
        assert bool((err <= bound).all()), (err - bound).max().item()
        return
    aff = torch.tensor(affine)
    if bool((~aff).any()):
        assert err[~aff].max().item() <= 1e-5
    if bool(aff.any()):
        assert err[aff].max().item() <= 1e-4


CASES = [
    # n_in, hs, ws, crop, n_out
    (3, 12, 10, 7, 7),      # 147 elements per image: scalar tail, straddling
    (3, 12, 10, 8, 7),      # 192 per image: whole chunks
    (3, 20, 18, 16, 7),
    (5, 40, 36, 32, 15),    # 46,080 elements: several workgroups
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_in,hs,ws,crop,n_out", CASES)
def test_kernel_matches_reference(dev, n_in, hs, ws, crop, n_out, dtype):
    frames = _frames(n_in, hs, ws, seed=crop)
    t = _table(n_in, hs, ws, crop, n_out)
    assert any(t["affine"]) and not all(t["affine"])
    # no pixel's inside/outside decision depends on rounding
    assert min(_edge_margin(_inv32(f), crop) for f in FORWARD) >= 1e-3
    ref = assemble_views_reference(frames, crop=crop, mean=MEAN, std=STD,
                                   dtype=torch.float32, **t)
    out = assemble_views(frames.to(dev), crop=crop, mean=MEAN, std=STD,
                         dtype=dtype, **t)
    _check(out, ref, t["affine"], dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_is_deterministic(dev, dtype):
    frames = _frames(3, 20, 18).to(dev)
    t = _table(3, 20, 18, 16, 7)
    a = assemble_views(frames, crop=16, mean=MEAN, std=STD, dtype=dtype, **t)
    b = assemble_views(frames, crop=16, mean=MEAN, std=STD, dtype=dtype, **t)
    assert torch.equal(a, b)


@pytest.mark.parametrize("crop", [7, 8])
def test_repeated_views_are_bit_identical(dev, crop):
    """streams=3 of the statistics pass: the same view in three rows.  At
    crop 7 the rows start at different offsets inside a 16-B chunk."""
    frames = _frames(2, 12, 10).to(dev)
    out = assemble_views(frames, [1, 1, 1], [3, 3, 3], [2, 2, 2],
                         [True] * 3, [_inv32(FORWARD[0])] * 3, [True] * 3,
                         crop, MEAN, STD, torch.bfloat16)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])

    bat = DeviceBatcher(crop, MEAN, STD, torch.bfloat16, dev, seed=1)
    ev = bat.eval_batch(_frames(2, 12, 10), streams=3)
    assert ev.shape == (6, 3, crop, crop)
    assert torch.equal(ev[:2], ev[2:4]) and torch.equal(ev[:2], ev[4:])


def test_batcher_matches_its_cpu_twin(dev):
    """Same seed, same draws: the GPU batcher's train batch is the CPU
    batcher's (the reference) within the bf16 bound."""
    src, tgt = _frames(2, 40, 40, seed=1), _frames(2, 40, 40, seed=2)
    # the seed's two duplicate views keep every coordinate clear of the edges
    g = torch.Generator().manual_seed(9)
    for aug in (False, False, True):
        views = draw_view_params(2, (40, 40), 32, 0.5, 0.1, g, aug=aug)
    assert min(_edge_margin(a.tolist(), 32) for a in views.inv_affine) >= 1e-3
    gpu = DeviceBatcher(32, MEAN, STD, torch.bfloat16, dev, seed=9)
    cpu = DeviceBatcher(32, MEAN, STD, torch.float32, "cpu", seed=9)
    out, ref = gpu.train_batch(src, tgt), cpu.train_batch(src, tgt)
    assert out.shape == (6, 3, 32, 32) and out.device.type == "cuda"
    _check(out, ref, [False] * 4 + [True] * 2, torch.bfloat16)


def test_engine_trains_from_uint8_frames(dev):
    from dwt_amd.engine.officehome import train_infinite_collect_stats
    from dwt_amd.models import Bottleneck, ResNetDWT

    torch.manual_seed(0)

    def loader(n, seed, **kw):
        ds = SyntheticOfficeHome(n, num_classes=7, img_size=40, seed=seed,
                                 uint8=True)
        return DataLoader(ds, batch_size=2, **kw)

    src_loader = loader(8, 1, drop_last=True)
    tgt_loader = loader(8, 2, drop_last=True)
    test_loader = loader(4, 2)

    model = ResNetDWT(Bottleneck, [1, 1, 1, 1], None, num_classes=7)
    model = model.to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    batcher = DeviceBatcher(32, MEAN, STD, torch.bfloat16, dev, seed=0)

    losses = []

    class Log:
        def log(self, **row):
            if row.get("kind") == "train":
                losses.append((row["cls_loss"], row["mec_loss"]))

    args = types.SimpleNamespace(log_interval=1, num_iters=2,
                                 check_acc_step=100)
    acc = train_infinite_collect_stats(
        args, model, dev, src_loader, tgt_loader, opt, 0.1, test_loader,
        logger=Log(), stats_passes=1, batcher=batcher)
    assert len(losses) == 2
    assert all(np.isfinite(v) for pair in losses for v in pair), losses
    assert 0.0 <= acc <= 100.0
