"""CPU checks of which launchers a norm site calls, in which order and on
which operands.  A recording stand-in replaces the extension, so nothing is
computed: _HipWhitenMulti, _HipBatchNormMulti and the two join Functions run
forward and backward on CPU tensors and the recorded calls are compared with
the route each input must take.  A change to hip_ops.py cannot silently
reroute a site past this."""
import pytest
import torch

from dwt_amd.kernels import hip_ops


class _Recorder:
    """Any attribute is a launcher that records (name, args), returns None."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def launcher(*args):
            self.calls.append((name, args))
        return launcher

    def names(self):
        return [name for name, _ in self.calls]

    def args(self, name):
        found = [a for n, a in self.calls if n == name]
        assert len(found) == 1, (name, self.names())
        return found[0]


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(hip_ops, "_ext", lambda: r)
    return r


# launchers whose first argument is the site's whole input and which take
# `parts`: position of `parts` in the arguments
_PARTS_AT = {"bn_bwd_apply_cl": -2}
_STREAMING = {
    "whiten_stats_partial", "whiten_stats_partial_cl", "whiten_apply",
    "whiten_apply_cl", "whiten_apply_res_cl", "whiten_bwd_reduce",
    "whiten_bwd_reduce_cl", "whiten_join_bwd_reduce_cl", "whiten_bwd_apply",
    "whiten_bwd_apply_cl", "bn_stats_partial", "bn_stats_partial_cl",
    "bn_apply", "bn_apply_cl", "bn_apply_res_cl", "bn_bwd_reduce",
    "bn_bwd_reduce_cl", "bn_join_bwd_reduce_cl", "bn_bwd_apply",
    "bn_bwd_apply_cl",
}


def _check_streaming(rec, x, parts):
    """Each launcher ran once, on the whole x, with parts passed through."""
    names = rec.names()
    assert len(set(names)) == len(names), names
    for name, args in rec.calls:
        if name in _STREAMING:
            assert args[0].data_ptr() == x.data_ptr(), name
            assert args[0].shape == x.shape, name
            assert args[_PARTS_AT.get(name, -1)] == parts, name


def _numels(rec, name, *idx):
    args = rec.args(name)
    return [args[i].numel() for i in idx]


def _whiten_inputs(c, cl):
    torch.manual_seed(0)
    x = torch.randn(6, c, 5, 7)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    return x.requires_grad_(True), \
        torch.randn(c, 1, 1, requires_grad=True), \
        torch.randn(c, 1, 1, requires_grad=True)


def _whiten_cfg(parts, groups, **kw):
    return dict(parts=parts, num_groups=groups, eps=1e-3, momentum=0.1,
                training=True, mode="chol", relu=True, **kw)


def _check_whiten_sizes(rec, suffix, parts, c, g, use_batch=True):
    """Stacked operands of the whitening launchers: parts x per-branch."""
    nw = parts * (c // g) * g * g
    if use_batch:
        acc, mean, cov = _numels(rec, "whiten_stats_final", 0, 1, 2)
        assert (acc, mean, cov) == (parts * (c // g) * (g + g * g),
                                    parts * c, nw)
        assert rec.args("whiten_stats_final")[3:] == (g, parts * (c // g), 70)
    apply_name = "whiten_apply_res_cl" if suffix == "_join" \
        else "whiten_apply" + suffix
    assert _numels(rec, apply_name, 1, 2) == [parts * c, nw]
    if suffix == "_join":
        assert _numels(rec, "whiten_join_bwd_reduce_cl", 4, 5, 8, 9) \
            == [parts * c, nw, nw, parts * 2 * c]
        suffix = "_cl"
    elif suffix == "_cl":
        assert _numels(rec, "whiten_bwd_reduce_cl", 2, 3, 6, 7) \
            == [parts * c, nw, nw, parts * 2 * c]
    else:
        assert _numels(rec, "whiten_bwd_reduce", 3, 4, 6, 7) \
            == [parts * c, nw, nw, parts * 2 * c]
    want = [nw, parts * c] if use_batch else [0, 0]     # S, corr
    assert _numels(rec, "whiten_bwd_apply" + suffix, 6, 7) == want


@pytest.mark.parametrize("c,cl,cfg_kw", [
    (16, False, {}),
    (64, True, {}),
    (64, True, {"stats_sync": True}),
], ids=["nchw", "nhwc", "nhwc_sync"])
def test_whiten_route(rec, c, cl, cfg_kw):
    parts, g = 3, 4
    x, gamma, beta = _whiten_inputs(c, cl)
    cfg = _whiten_cfg(parts, c // g, **cfg_kw)
    out = hip_ops._HipWhitenMulti.apply(x, gamma, beta, None, None, cfg)
    sfx = "_cl" if cl else ""
    assert rec.names() == ["whiten_stats_partial" + sfx, "whiten_stats_final",
                           "matfn_chol_fwd", "whiten_apply" + sfx]
    assert out.shape == x.shape
    assert out.is_contiguous(memory_format=torch.channels_last) == cl
    assert _numels(rec, "whiten_stats_partial" + sfx, 1) \
        == [parts * (c // g) * (g + g * g)]
    out.backward(torch.ones_like(out))
    assert rec.names()[4:] == ["whiten_bwd_reduce" + sfx, "matfn_chol_bwd",
                               "whiten_bwd_apply" + sfx]
    _check_streaming(rec, x, parts)
    _check_whiten_sizes(rec, sfx, parts, c, g)
    assert x.grad.shape == x.shape and gamma.grad.shape == gamma.shape


def test_whiten_route_one_part(rec):
    """parts = 1 takes the same launchers, once each."""
    x, gamma, beta = _whiten_inputs(16, False)
    out = hip_ops._HipWhitenMulti.apply(x, gamma, beta, None, None,
                                        _whiten_cfg(1, 4))
    out.backward(torch.ones_like(out))
    assert rec.names() == ["whiten_stats_partial", "whiten_stats_final",
                           "matfn_chol_fwd", "whiten_apply",
                           "whiten_bwd_reduce", "matfn_chol_bwd",
                           "whiten_bwd_apply"]
    _check_streaming(rec, x, 1)
    assert rec.args("whiten_stats_final")[3:] == (4, 4, 210)


@pytest.mark.parametrize("right_size", [True, False])
def test_whiten_handed_over_stats(rec, right_size):
    """Raw sums from the producing conv replace the partial launch, when
    they are this site's size."""
    parts, c, g = 3, 64, 4
    x, gamma, beta = _whiten_inputs(c, True)
    numel = parts * (c // g) * (g + g * g)
    handed = torch.zeros(numel if right_size else numel - 1)
    cfg = _whiten_cfg(parts, c // g)
    cfg_before = dict(cfg)
    hip_ops._HipWhitenMulti.apply(x, gamma, beta, None, None, cfg, handed)
    # the accumulator is an argument: cfg is left as it was and holds no tensor
    assert cfg == cfg_before
    assert not any(isinstance(v, torch.Tensor) for v in cfg.values())
    tail = ["whiten_stats_final", "matfn_chol_fwd", "whiten_apply_cl"]
    acc = rec.args("whiten_stats_final")[0]
    if right_size:
        assert rec.names() == tail
        assert acc.data_ptr() == handed.data_ptr()
    else:
        assert rec.names() == ["whiten_stats_partial_cl"] + tail
        assert acc.data_ptr() != handed.data_ptr() and acc.numel() == numel
        assert rec.args("whiten_stats_partial_cl")[1] is acc


def test_whiten_join_route(rec):
    parts, c, g = 3, 64, 4
    x, gamma, beta = _whiten_inputs(c, True)
    identity = torch.randn(6, c, 5, 7) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    cfg = _whiten_cfg(parts, c // g)
    assert hip_ops.join_supported("whiten", x, identity, cfg)
    ya, yb = hip_ops.whiten_join(x, identity, gamma, beta, None, None, cfg)
    assert ya.data_ptr() == yb.data_ptr()
    assert rec.names() == ["whiten_stats_partial_cl", "whiten_stats_final",
                           "matfn_chol_fwd", "whiten_apply_res_cl"]
    assert rec.args("whiten_apply_res_cl")[5].data_ptr() == identity.data_ptr()
    (ya.sum() + 2 * yb.sum()).backward()
    assert rec.names()[4:] == ["whiten_join_bwd_reduce_cl", "matfn_chol_bwd",
                               "whiten_bwd_apply_cl"]
    _check_streaming(rec, x, parts)
    _check_whiten_sizes(rec, "_join", parts, c, g)
    red = rec.args("whiten_join_bwd_reduce_cl")
    assert red[1].data_ptr() == ya.data_ptr()          # the block output
    assert red[2] is not None and red[3] is not None   # both consumers
    # gid is the identity's gradient and the dout of the apply pass
    assert rec.args("whiten_bwd_apply_cl")[1] is red[7]
    assert identity.grad.shape == identity.shape


def _bn_inputs(shape, cl):
    torch.manual_seed(1)
    x = torch.randn(*shape)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    c = shape[1]
    gshape = (c, 1, 1) if len(shape) == 4 else (1, c)
    return x.requires_grad_(True), \
        torch.randn(*gshape, requires_grad=True), \
        torch.randn(*gshape, requires_grad=True)


def _bn_cfg(parts, **kw):
    return dict(parts=parts, eps=1e-5, momentum=0.1, training=True, relu=True,
                **kw)


@pytest.mark.parametrize("shape,cl,sfx", [
    ((6, 12, 5, 7), False, ""),
    ((6, 128, 5, 7), True, "_cl"),
    ((6, 32), False, "_cl"),     # (N, C) is channels-last as it stands
], ids=["nchw", "nhwc", "2d"])
def test_bn_route(rec, shape, cl, sfx):
    parts, c = 3, shape[1]
    cnt = 2 * (35 if len(shape) == 4 else 1)
    x, gamma, beta = _bn_inputs(shape, cl)
    out = hip_ops._HipBatchNormMulti.apply(x, gamma, beta, None, None,
                                           _bn_cfg(parts))
    assert rec.names() == ["bn_stats_partial" + sfx, "bn_stats_final",
                           "bn_apply" + sfx]
    assert out.shape == x.shape and out.stride() == x.stride()
    out.backward(torch.ones_like(out))
    assert rec.names()[3:] == ["bn_bwd_reduce" + sfx, "bn_bwd_apply" + sfx]
    _check_streaming(rec, x, parts)
    assert _numels(rec, "bn_stats_partial" + sfx, 1) == [parts * 2 * c]
    assert _numels(rec, "bn_stats_final", 0, 1, 2, 3) \
        == [parts * 2 * c] + [parts * c] * 3
    assert rec.args("bn_stats_final")[4:] == (c, parts, cnt, 1e-5)
    assert _numels(rec, "bn_apply" + sfx, 1, 2) == [parts * c] * 2
    if sfx:
        assert _numels(rec, "bn_bwd_reduce_cl", 2, 3, 6) \
            == [parts * c, parts * c, parts * 2 * c]
        assert _numels(rec, "bn_bwd_apply_cl", 2, 3, 6) \
            == [parts * c, parts * c, parts * 2 * c]
        assert rec.args("bn_bwd_apply_cl")[-1] == cnt
    else:
        assert _numels(rec, "bn_bwd_reduce", 3, 4, 5) \
            == [parts * c, parts * c, parts * 2 * c]
        assert _numels(rec, "bn_bwd_apply", 3, 4, 6) \
            == [parts * c, parts * c, parts * 2 * c]
        assert rec.args("bn_bwd_apply")[-2] == cnt
    assert x.grad.shape == x.shape and gamma.grad.shape == gamma.shape


@pytest.mark.parametrize("join", [False, True], ids=["plain", "join"])
def test_bn_handed_over_stats(rec, join):
    """As test_whiten_handed_over_stats; the join Function passes the
    accumulator through to the site's forward."""
    parts, c = 3, 128
    x, gamma, beta = _bn_inputs((6, c, 5, 7), True)
    handed = torch.zeros(parts * 2 * c)
    cfg = _bn_cfg(parts)
    cfg_before = dict(cfg)
    if join:
        identity = torch.randn(6, c, 5, 7) \
            .contiguous(memory_format=torch.channels_last)
        hip_ops.batch_norm_join(x, identity, gamma, beta, None, None, cfg,
                                handed)
    else:
        hip_ops._HipBatchNormMulti.apply(x, gamma, beta, None, None, cfg,
                                         handed)
    assert cfg == cfg_before
    assert not any(isinstance(v, torch.Tensor) for v in cfg.values())
    assert rec.names() == ["bn_stats_final",
                           "bn_apply_res_cl" if join else "bn_apply_cl"]
    assert rec.args("bn_stats_final")[0].data_ptr() == handed.data_ptr()


def test_bn_route_one_part(rec):
    x, gamma, beta = _bn_inputs((6, 12, 5, 7), False)
    out = hip_ops._HipBatchNormMulti.apply(x, gamma, beta, None, None,
                                           _bn_cfg(1))
    out.backward(torch.ones_like(out))
    assert rec.names() == ["bn_stats_partial", "bn_stats_final", "bn_apply",
                           "bn_bwd_reduce", "bn_bwd_apply"]
    _check_streaming(rec, x, 1)
    assert rec.args("bn_stats_final")[4:] == (12, 1, 210, 1e-5)


def test_bn_join_route(rec):
    parts, c = 3, 128
    x, gamma, beta = _bn_inputs((6, c, 5, 7), True)
    identity = torch.randn(6, c, 5, 7) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    cfg = _bn_cfg(parts)
    assert hip_ops.join_supported("bn", x, identity, cfg)
    ya, yb = hip_ops.batch_norm_join(x, identity, gamma, beta, None, None, cfg)
    assert ya.data_ptr() == yb.data_ptr()
    assert rec.names() == ["bn_stats_partial_cl", "bn_stats_final",
                           "bn_apply_res_cl"]
    assert rec.args("bn_apply_res_cl")[5].data_ptr() == identity.data_ptr()
    ya.sum().backward()                        # one consumer only
    assert rec.names()[3:] == ["bn_join_bwd_reduce_cl", "bn_bwd_apply_cl"]
    _check_streaming(rec, x, parts)
    red = rec.args("bn_join_bwd_reduce_cl")
    assert red[1].data_ptr() == ya.data_ptr()
    assert red[2] is not None and red[3] is None
    assert _numels(rec, "bn_join_bwd_reduce_cl", 4, 5, 7) \
        == [parts * c, parts * c, parts * 2 * c]
    assert rec.args("bn_bwd_apply_cl")[1] is red[6]
    assert identity.grad.shape == identity.shape


def test_join_functions_keep_their_names():
    assert hip_ops._HipWhitenJoin.__name__ == "_HipWhitenJoin"
    assert hip_ops._HipBatchNormJoin.__name__ == "_HipBatchNormJoin"
    assert hip_ops._HipWhitenJoin is not hip_ops._HipBatchNormJoin


def test_whiten_eval_route(rec):
    """Eval: running statistics, so no statistics launch in forward and no
    matrix-function backward; S and corr reach the apply pass empty."""
    parts, c, g = 3, 16, 4
    x, gamma, beta = _whiten_inputs(c, False)
    rms = [torch.full((1, c, 1, 1), float(p)) for p in range(parts)]
    rvs = [torch.eye(g).repeat(c // g, 1, 1) * (p + 1) for p in range(parts)]
    cfg = _whiten_cfg(parts, c // g)
    cfg["training"] = False
    out = hip_ops._HipWhitenMulti.apply(x, gamma, beta, rms, rvs, cfg)
    assert rec.names() == ["matfn_chol_fwd", "whiten_apply"]
    mean, cov = rec.args("whiten_apply")[1], rec.args("matfn_chol_fwd")[0]
    assert torch.equal(mean.reshape(parts, c)[:, 0], torch.arange(3.0))
    assert torch.equal(cov.reshape(parts, -1)[:, 0], torch.arange(1.0, 4.0))
    out.backward(torch.ones_like(out))
    assert rec.names()[2:] == ["whiten_bwd_reduce", "whiten_bwd_apply"]
    _check_streaming(rec, x, parts)
    _check_whiten_sizes(rec, "", parts, c, g, use_batch=False)
    assert rec.args("whiten_bwd_apply")[-2] is False    # train_stats


def test_bn_eval_route(rec):
    parts, c = 3, 12
    x, gamma, beta = _bn_inputs((6, c, 5, 7), False)
    rms = [torch.full((c,), float(p)) for p in range(parts)]
    rvs = [torch.full((c,), float(p + 1)) for p in range(parts)]
    cfg = _bn_cfg(parts)
    cfg["training"] = False
    out = hip_ops._HipBatchNormMulti.apply(x, gamma, beta, rms, rvs, cfg)
    assert rec.names() == ["bn_apply"]
    mean, istd = rec.args("bn_apply")[1:3]
    assert torch.equal(mean.reshape(parts, c)[:, 0], torch.arange(3.0))
    assert torch.allclose(istd.reshape(parts, c)[:, 0],
                          torch.rsqrt(torch.arange(1.0, 4.0) + 1e-5))
    out.backward(torch.ones_like(out))
    assert rec.names()[1:] == ["bn_bwd_reduce", "bn_bwd_apply"]
    _check_streaming(rec, x, parts)
    assert rec.args("bn_bwd_apply")[-3] is False        # use_batch
