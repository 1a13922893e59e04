"""Device-side input pipeline on the CPU: the pure-torch reference
(`assemble_views_reference`, the oracle of tests/test_gpu_device_pipeline.py)
against the loaders' own transforms and scipy, the view-table draws, the
host-side validation and the entrypoint flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

from dwt_amd.data import (DeviceBatcher, Normalize, SyntheticOfficeHome,
                          ToTensor, ToUint8HWC, assemble_views,
                          assemble_views_reference, draw_view_params)

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]
FORWARD = ([[1.07, 0.05], [-0.08, 0.93]], [[1.19, -0.13], [0.09, 0.88]])
IDENT = [1.0, 0.0, 0.0, 1.0]


def _frames(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def _inv32(forward):
    """Closed-form fp64 inverse of the fp32-stored forward matrix, as fp32."""
    m = np.float32(forward).astype(np.float64)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    inv = np.array([[m[1, 1], -m[0, 1]], [-m[1, 0], m[0, 0]]]) / det
    return inv.astype(np.float32)


def _expected_plain(frame, top, left, crop, flip):
    view = frame[top:top + crop, left:left + crop].numpy()
    if flip:
        view = view[:, ::-1]
    return Normalize(MEAN, STD)(ToTensor()(np.ascontiguousarray(view)))


@pytest.mark.parametrize("flip", [False, True])
def test_plain_and_flipped_views_match_the_transforms(flip):
    frames = _frames(2, 12, 10)
    crop = 7
    corners = [(t, l) for t in (0, 12 - crop) for l in (0, 10 - crop)]
    n = len(corners)
    out = assemble_views(frames, [1] * n, [t for t, _ in corners],
                         [l for _, l in corners], [flip] * n, [IDENT] * n,
                         [False] * n, crop, MEAN, STD, torch.float32)
    assert out.shape == (n, 3, crop, crop)
    assert out.is_contiguous(memory_format=torch.channels_last)
    for i, (t, l) in enumerate(corners):
        exp = _expected_plain(frames[1], t, l, crop, flip)
        assert (out[i] - exp).abs().max().item() <= 1e-6


def _margin_and_outside(inv32, crop):
    """fp64: every source coordinate's distance to the frame edges (pixel
    (0, 0) maps to exactly 0 in any arithmetic and is left out), and the
    outside mask."""
    inv = inv32.astype(np.float64)
    rr, cc = np.meshgrid(np.arange(crop), np.arange(crop), indexing="ij")
    pr = inv[0, 0] * rr + inv[0, 1] * cc
    pc = inv[1, 0] * rr + inv[1, 1] * cc
    dist = np.minimum(np.minimum(np.abs(pr), np.abs(pr - (crop - 1))),
                      np.minimum(np.abs(pc), np.abs(pc - (crop - 1))))
    dist[0, 0] = np.inf
    outside = (pr < 0) | (pr > crop - 1) | (pc < 0) | (pc > crop - 1)
    return dist.min(), outside


@pytest.mark.parametrize("crop", [7, 8, 12, 16])
@pytest.mark.parametrize("forward", FORWARD)
def test_affine_views_match_scipy(crop, forward):
    frames = _frames(2, 20, 18, seed=crop)
    inv32 = _inv32(forward)
    margin, outside = _margin_and_outside(inv32, crop)
    assert margin >= 1e-3, margin          # no decision depends on rounding
    frac = outside.mean()
    assert 0.1 < frac < 0.3, frac          # both branches are exercised

    rows = [(0, 0, 0, False), (1, 20 - crop, 18 - crop, True), (1, 2, 1, True)]
    n = len(rows)
    out = assemble_views(frames, [r[0] for r in rows], [r[1] for r in rows],
                         [r[2] for r in rows], [r[3] for r in rows],
                         [inv32.reshape(4).tolist()] * n, [True] * n, crop,
                         MEAN, STD, torch.float32)
    norm = Normalize(MEAN, STD)
    for i, (src, t, l, flip) in enumerate(rows):
        view = frames[src, t:t + crop, l:l + crop].numpy()
        if flip:
            view = view[:, ::-1]
        chw = ToTensor()(np.ascontiguousarray(view)).numpy()
        warped = np.stack([
            ndimage.affine_transform(chw[c], inv32.astype(np.float64), order=1,
                                     mode="constant", cval=0.0)
            for c in range(3)])
        exp = norm(torch.from_numpy(warped))
        assert (out[i] - exp).abs().max().item() <= 1e-4

        # border constant: out-of-frame pixels are normalized black
        mask = torch.from_numpy(outside)
        for c in range(3):
            black = (0.0 - MEAN[c]) / STD[c]
            assert (out[i, c][mask] - black).abs().max().item() <= 1e-6


def test_draw_view_params():
    def draw(seed, aug):
        g = torch.Generator().manual_seed(seed)
        return draw_view_params(256, (12, 12), 8, 0.5, 0.1, g, aug=aug)

    a, b = draw(3, True), draw(3, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for t in (a.top, a.left):
        assert int(t.min()) == 0 and int(t.max()) == 4
    assert a.inv_affine.dtype == torch.float32 and a.inv_affine.shape == (256, 4)
    assert bool(a.affine.all()) and 0 < int(a.flip.sum()) < 256
    # closed-form inverse: inv @ forward == I for a matrix near the identity
    m = a.inv_affine[0].double().view(2, 2)
    assert (m - torch.eye(2).double()).abs().max() < 1.0

    plain = draw(3, False)
    assert not bool(plain.flip.any()) and not bool(plain.affine.any())
    assert torch.equal(plain.inv_affine,
                       torch.tensor(IDENT).repeat(256, 1))

    # the duplicate's crop is its own: target and duplicate come from one
    # generator, drawn one after the other, as DeviceBatcher.train_batch does
    g = torch.Generator().manual_seed(5)
    tgt = draw_view_params(256, (12, 12), 8, 0.5, 0.1, g, aug=False)
    dup = draw_view_params(256, (12, 12), 8, 0.5, 0.1, g, aug=True)
    assert bool(((tgt.top != dup.top) | (tgt.left != dup.left)).any())


def test_validation_raises_before_any_work():
    frames = _frames(2, 12, 10)
    ok = dict(images_u8=frames, src_index=[0, 1], top=[0, 5], left=[0, 3],
              flip=[False, True], inv_affine=[IDENT, IDENT],
              affine=[False, False], crop=7, mean=MEAN, std=STD,
              dtype=torch.float32)
    assemble_views(**ok)
    bad = [
        dict(images_u8=frames.float()),                       # not uint8
        dict(images_u8=frames[0]),                            # not 4-D
        dict(images_u8=_frames(2, 12, 10)[..., :2]),          # last dim != 3
        dict(images_u8=frames.permute(0, 2, 1, 3)),           # not contiguous
        dict(src_index=[0, 2]),
        dict(src_index=[-1, 0]),
        dict(top=[0, 6]),
        dict(top=[-1, 0]),
        dict(left=[4, 0]),
        dict(left=[0, -1]),
        dict(top=[0]),                                        # lengths
        dict(flip=[False]),
        dict(affine=[False, False, False]),
        dict(inv_affine=[IDENT]),
        dict(crop=13),
        dict(dtype=torch.float16),
    ]
    for change in bad:
        with pytest.raises(ValueError):
            assemble_views(**{**ok, **change})


def test_batcher_streams_on_cpu():
    src, tgt = _frames(2, 12, 10, seed=1), _frames(2, 12, 10, seed=2)
    bat = DeviceBatcher(8, MEAN, STD, torch.float32, "cpu", seed=4)
    out = bat.train_batch(src, tgt)
    assert out.shape == (6, 3, 8, 8) and bool(torch.isfinite(out).all())
    ev = bat.eval_batch(tgt, streams=3)
    assert ev.shape == (6, 3, 8, 8)
    assert torch.equal(ev[:2], ev[2:4]) and torch.equal(ev[:2], ev[4:])
    assert bat.eval_batch(tgt, streams=1).shape == (2, 3, 8, 8)
    # same seed, same batches
    again = DeviceBatcher(8, MEAN, STD, torch.float32, "cpu", seed=4)
    assert torch.equal(again.train_batch(src, tgt), out)


def test_uint8_frames_from_loaders():
    ds = SyntheticOfficeHome(4, num_classes=5, img_size=40, seed=1, uint8=True)
    img, label = ds[1]
    assert img.dtype == torch.uint8 and img.shape == (40, 40, 3)
    assert torch.equal(img, ds[1][0]) and 0 <= int(label) < 5
    with pytest.raises(ValueError):
        SyntheticOfficeHome(4, transform_aug=True, uint8=True)

    from PIL import Image
    arr = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3)
    for x in (arr, Image.fromarray(arr)):
        t = ToUint8HWC()(x)
        assert t.dtype == torch.uint8 and torch.equal(t, torch.from_numpy(arr))
    gray = ToUint8HWC()(Image.fromarray(arr[..., 0]))
    assert gray.shape == (5, 4, 3)


def _entrypoint(*extra):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run(
        [sys.executable, "resnet50_dwt_mec_officehome.py", "--synthetic",
         "--synthetic_size", "64", "--num_iters", "3", "--check_acc_step",
         "100", "--source_batch_size", "4", "--test_batch_size", "8",
         "--num_workers", "0", "--log_interval", "1", "--img_resize", "72",
         "--img_crop_size", "64", "--stats_passes", "1", *extra],
        cwd=repo, capture_output=True, text=True, timeout=900)


def test_officehome_entrypoint_device_pipeline_cpu():
    r = _entrypoint("--device_pipeline")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Train Iter" in r.stdout
    assert "Test set" in r.stdout


def test_device_pipeline_excludes_gpu_augment():
    r = _entrypoint("--device_pipeline", "--gpu_augment")
    assert r.returncode != 0
    assert "not allowed with" in r.stderr
