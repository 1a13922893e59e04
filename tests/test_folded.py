"""Folded target-domain inference (models/folded.py), CPU side: the fold is
exact, picks the right branch, round-trips through its checkpoint and plugs
into the engine and the entrypoint."""
import copy
import functools
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from dwt_amd.data import SyntheticOfficeHome
from dwt_amd.engine import officehome as engine
from dwt_amd.models import (Bottleneck, FoldedResNetDWT, ResNetDWT, checkpoint,
                            fold_norm_into_conv, fold_resnet)
from dwt_amd.models import resnet_dwt
from dwt_amd.models.sites import norm_site
from dwt_amd.ops.batch_norm import DomainBatchNorm2d, _DomainBatchNorm
from dwt_amd.ops.whitening import WhiteningScaleShift, WTransform2d

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def randomize_stats(model, seed=0):
    """Random running mean / covariance / variance in every norm branch and
    random shared gamma / beta.  Covariances are SPD: a a^T / g + 0.1 I."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, WTransform2d):
                G, g, _ = m.running_variance.shape
                a = torch.randn(G, g, g, generator=gen)
                cov = a @ a.transpose(1, 2) / g + 0.1 * torch.eye(g)
                m.running_variance.copy_(cov)
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=gen))
            elif isinstance(m, _DomainBatchNorm):
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
        for name, p in model.named_parameters():
            leaf = name.split(".")[-1]
            if "gamma" in leaf:
                p.copy_(0.5 + torch.rand(p.shape, generator=gen))
            elif "beta" in leaf:
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))


def make_model(layers, mode="chol", group_size=4, dtype=torch.float64, seed=0):
    torch.manual_seed(seed)
    model = ResNetDWT(Bottleneck, layers, None, num_classes=7,
                      group_size=group_size, whiten_mode=mode)
    randomize_stats(model, seed)
    return model.to(dtype).eval()


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


# ---------------------------------------------------------------------------
# fold equals eval
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layers", [[2, 1, 2, 1], [3, 4, 6, 3]],
                         ids=["small", "r50"])
@pytest.mark.parametrize("mode", ["chol", "zca"])
@pytest.mark.parametrize("group_size", [4, 16])
def test_fold_equals_eval(layers, mode, group_size):
    model = make_model(layers, mode, group_size)
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    with torch.no_grad():
        ref = model(x)
        folded = fold_resnet(model)
        got = folded(x)
    assert folded.layers == layers
    assert got.shape == ref.shape == (2, 7)
    err = rel_err(got, ref)
    print(f"fold vs eval {layers} {mode} g={group_size}: {err:.3e}")
    assert err <= 1e-5


def test_folded_module_surface():
    model = make_model([2, 1, 2, 1], dtype=torch.float32)
    folded = fold_resnet(model)
    assert isinstance(folded, FoldedResNetDWT)
    params = dict(folded.named_parameters())
    assert all(not p.requires_grad for p in params.values())
    # engine.test reads the model dtype from the first parameter
    assert next(folded.parameters()).dtype == torch.float32
    for key in ("conv1.weight", "conv1.bias", "layer1.0.conv1.weight",
                "layer1.1.conv3.bias", "layer2.0.downsample.0.weight",
                "layer3.1.conv2.weight", "fc_out.weight", "fc_out.bias"):
        assert key in params, key
    assert "layer1.1.downsample.0.weight" not in params
    assert params["conv1.weight"].shape == (64, 4, 7, 7)   # stem padded once
    assert params["conv1.weight"][:, 3].abs().max() == 0
    assert params["conv1.bias"].dtype == torch.float32
    assert params["layer1.0.conv2.weight"].is_contiguous(
        memory_format=torch.channels_last)
    assert folded.meta["layers"] == [2, 1, 2, 1] and folded.meta["branch"] == 1
    # NCHW and channels_last inputs give the same output
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        a = folded(x)
        b = folded(x.contiguous(memory_format=torch.channels_last))
    assert torch.allclose(a, b, atol=1e-5 * a.abs().max().item())


def test_fold_unwraps_data_parallel_wrapper():
    model = make_model([1, 1, 1, 1], dtype=torch.float32)
    wrapper = types.SimpleNamespace(module=model)
    a = fold_resnet(model).state_dict()
    b = fold_resnet(wrapper).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------
# branch selection
# ---------------------------------------------------------------------------

def _sd_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_branch_selection(monkeypatch):
    model = make_model([2, 1, 2, 1])
    base = fold_resnet(model).state_dict()

    def touched(kind):
        m2 = copy.deepcopy(model)
        gen = torch.Generator().manual_seed(123)
        with torch.no_grad():
            for name, mod in m2.named_modules():
                parts = name.split(".")
                owner = parts[-2] if parts[-1] == "wh" else parts[-1]
                is_src = owner.startswith("bns") or owner == "downsample_bns"
                is_aug = owner.endswith("_aug")
                is_tgt = (owner.startswith("bnt") or owner == "downsample_bnt") \
                    and not is_aug
                hit = {"source": is_src, "aug": is_aug, "target": is_tgt}[kind]
                if not hit:
                    continue
                if isinstance(mod, (WTransform2d, _DomainBatchNorm)):
                    mod.running_mean.add_(torch.randn(mod.running_mean.shape,
                                                      generator=gen))
        return m2

    assert _sd_equal(base, fold_resnet(touched("source")).state_dict())
    assert _sd_equal(base, fold_resnet(touched("aug")).state_dict())
    assert not _sd_equal(base, fold_resnet(touched("target")).state_dict())

    # branch=0 is an eval routed through the source branch
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    monkeypatch.setattr(resnet_dwt, "norm_site",
                        functools.partial(norm_site, eval_branch=0))
    with torch.no_grad():
        ref_src = model(x)
    monkeypatch.undo()
    with torch.no_grad():
        ref_tgt = model(x)
        got_src = fold_resnet(model, branch=0)(x)
    assert rel_err(got_src, ref_src) <= 1e-5
    assert rel_err(got_src, ref_tgt) > 1e-3     # the branches really differ
    with pytest.raises(ValueError):
        fold_resnet(model, branch=3)


# ---------------------------------------------------------------------------
# one site
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["whiten_chol", "whiten_zca", "bn"])
@pytest.mark.parametrize("ksize", [1, 3])
def test_fold_norm_into_conv_one_site(kind, ksize):
    cin, cout = 8, 16
    gen = torch.Generator().manual_seed(5)
    if kind == "bn":
        branches = [DomainBatchNorm2d(cout, affine=False) for _ in range(3)]
    else:
        branches = [WhiteningScaleShift(cout, 4, affine=False,
                                        mode=kind.split("_")[1])
                    for _ in range(3)]
    holder = torch.nn.ModuleList(branches)
    randomize_stats(holder, seed=7)
    holder.double()
    gamma = (0.5 + torch.rand(cout, 1, 1, generator=gen)).double()
    beta = torch.randn(cout, 1, 1, generator=gen).double()
    w = torch.randn(cout, cin, ksize, ksize, generator=gen).double()
    x = torch.randn(2, cin, 9, 9, generator=gen).double()
    pad = ksize // 2
    ref = norm_site(F.conv2d(x, w, None, 1, pad), branches, gamma, beta,
                    training=False, relu=False)
    wf, bf = fold_norm_into_conv(w, branches[1], gamma, beta)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float32
    assert wf.is_contiguous(memory_format=torch.channels_last)
    got = F.conv2d(x, wf, bf.double(), 1, pad)
    assert rel_err(got, ref) <= 1e-5
    # the source branch gives another map
    w0, _ = fold_norm_into_conv(w, branches[0], gamma, beta)
    assert not torch.allclose(w0, wf)


# ---------------------------------------------------------------------------
# checkpoint
# ---------------------------------------------------------------------------

def test_checkpoint_round_trip(tmp_path):
    model = make_model([2, 1, 2, 1], mode="zca", dtype=torch.float32)
    folded = fold_resnet(model)
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        want = folded(x)
    path = str(tmp_path / "sub" / "folded.pt")
    checkpoint.save_folded(path, folded)
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    sd = {k: v.clone() for k, v in folded.state_dict().items()}
    del model, folded
    loaded = checkpoint.load_folded(path, device="cpu")
    assert isinstance(loaded, FoldedResNetDWT)
    sd2 = loaded.state_dict()
    assert sd.keys() == sd2.keys()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert loaded.meta["layers"] == [2, 1, 2, 1]
    assert loaded.meta["num_classes"] == 7
    assert loaded.meta["branch"] == 1
    assert loaded.meta["whiten_mode"] == "zca"
    assert loaded.meta["dtype"] == "float32"
    with torch.no_grad():
        assert torch.equal(loaded(x), want)


# ---------------------------------------------------------------------------
# engine and entrypoint
# ---------------------------------------------------------------------------

def test_engine_test_same_for_folded(capsys):
    model = make_model([1, 1, 1, 1], dtype=torch.float32)
    tst = SyntheticOfficeHome(16, num_classes=7, img_size=64, seed=2)
    loader = DataLoader(tst, batch_size=4)
    args = types.SimpleNamespace()
    dev = torch.device("cpu")
    acc_model = engine.test(args, model, dev, loader)
    line_model = capsys.readouterr().out
    acc_folded = engine.test(args, fold_resnet(model), dev, loader)
    line_folded = capsys.readouterr().out
    acc_flag = engine.test(types.SimpleNamespace(folded_eval=True), model, dev,
                           loader)
    line_flag = capsys.readouterr().out
    assert "Test set: Average loss:" in line_model
    assert acc_folded == acc_model == acc_flag
    assert line_folded == line_model == line_flag


def test_entrypoint_folded_eval_and_export(tmp_path):
    out = str(tmp_path / "folded.pt")
    r = subprocess.run(
        [sys.executable, "resnet50_dwt_mec_officehome.py", "--synthetic",
         "--synthetic_size", "64", "--num_iters", "2", "--check_acc_step",
         "1", "--source_batch_size", "4", "--test_batch_size", "8",
         "--num_workers", "0", "--log_interval", "1", "--img_crop_size",
         "64", "--stats_passes", "1", "--dtype", "float32",
         "--folded_eval", "--export_folded", out],
        cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("Test set: Average loss:") == 3
    loaded = checkpoint.load_folded(out)
    assert loaded.layers == [3, 4, 6, 3]
    assert loaded.meta["whiten_mode"] == "zca"
    with torch.no_grad():
        y = loaded(torch.randn(1, 3, 64, 64))
    assert y.shape == (1, 65) and torch.isfinite(y).all()
