"""GPU autograd Functions backed by the gfx950 HIP kernels.

Mirrors the algorithm contract of dwt_amd/ops/functional.py exactly (these
are numerically tested against it in tests/test_gpu_kernels.py).  The
register-blocked fast path covers group sizes {2, 4, 8}; 8 < g <= 32 runs
the generic LDS-tiled NCHW kernels (every group size the reference models
can construct); fp32/bf16 inputs; anything else falls back to the torch
implementation (warned once).

Every site stacks its domain branches: the launchers of both layouts take the
whole (parts*B, ...) batch, statistics buffers laid out [parts, ...] and
``parts``, so a pass is a two-way fork on the layout and nothing here loops
over branches but the running-buffer EMA and the stacking of running buffers
in eval.  Batch statistics are taken in one place per Function: raw sums
(handed over by the producing conv, or a partial launch) -> all-reduce when
``stats_sync`` spans ranks -> finalize.
"""
from __future__ import annotations

import warnings
import torch

from . import dispatch
from ..ops.functional import _dist_world

_GEN_G_MAX = 32  # register-blocked kernels cover g in {2,4,8};
                 # 8 < g <= 32 runs the LDS-tiled generic NCHW kernels
_warned = set()


def _whiten_layout(x, c, g):
    """'cl' when x is channels_last and the NHWC kernels support (C, g):
    the lane map needs GW = min(C,256)/g to divide the 256-thread block.
    g > 8 always routes NCHW (the generic LDS-tiled kernels)."""
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
            and not x.is_contiguous():
        if whiten_cl_supported(c, g):
            return "cl"
    return "nchw"


def whiten_cl_supported(c, g):
    """(C, g) the NHWC whitening kernels serve (see _whiten_layout)."""
    if c % 64 == 0 and (c <= 256 or c % 256 == 0) and g in (2, 4):
        # g=8 NHWC instantiations spill registers (profiles/
        # kernel_resources.md) — route them to the NCHW path
        gw = min(c, 256) // g
        return gw > 0 and 256 % gw == 0
    return False


def bn_cl_supported(c):
    """The NHWC BN kernels map lanes as t %% NCH with NCH = min(C,1024)/4;
    rows advance by blockDim/NCH — NCH must divide the block (else boundary
    rows are double-counted)."""
    if c % 4 != 0 or (c > 1024 and c % 1024 != 0):
        return False
    nch = min(c, 1024) // 4
    return 256 % nch == 0


def _bn_layout(x, c):
    if x.dim() == 2 and x.is_contiguous() and bn_cl_supported(c):
        return "cl"  # (N, C) IS channels-last: C contiguous per position
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
            and not x.is_contiguous() and bn_cl_supported(c):
        return "cl"
    return "nchw"


def _flat_affine(gamma, beta, c, like):
    """(has_affine, gamma, beta) with the affine flattened to (C,) for the
    kernels; empty placeholders without one."""
    if gamma is None:
        return False, torch.empty(0, device=like.device, dtype=like.dtype), \
            torch.empty(0, device=like.device, dtype=like.dtype)
    return True, gamma.detach().reshape(c).contiguous(), \
        beta.detach().reshape(c).contiguous()


def _ema_update(ext, rm, new_mean, rv, new_var, momentum):
    """Running-statistics EMA: the fused kernel on fp32 contiguous buffers,
    mul_/add_ otherwise."""
    if rm.dtype == torch.float32 and rm.is_contiguous() \
            and rv.dtype == torch.float32 and rv.is_contiguous():
        ext.ema_update(rm, new_mean, rv, new_var, momentum)
    else:
        rm.mul_(1.0 - momentum).add_(
            new_mean.reshape(rm.shape).to(rm.dtype), alpha=momentum)
        rv.mul_(1.0 - momentum).add_(
            new_var.reshape(rv.shape).to(rv.dtype), alpha=momentum)


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(msg)


def _allreduce(t):
    import torch.distributed as dist
    dist.all_reduce(t)
    return t


def _ext():
    return dispatch.ext()


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _usable_stats_acc(acc, x, layout, training, numel):
    """``acc``: the pre-accumulated raw sums a producing conv handed over
    (ops/mfma.py::conv1x1_stats), or None.  Returns them flat when this
    forward can use them — NHWC training statistics of exactly this site's
    size — else None: the site computes its own statistics."""
    if acc is None or not training or layout != "cl" or x.dim() != 4:
        return None
    if acc.dtype != torch.float32 or acc.device != x.device \
            or acc.numel() != numel or not acc.is_contiguous():
        return None
    return acc.detach().reshape(-1)


class _HipWhitenMulti(torch.autograd.Function):
    """All per-branch statistics are STACKED ([parts*C] means, [parts*G, g, g]
    covariances/W) and every pass is one launcher call on the whole batch,
    in either layout.  The channels_last launchers run ONE launch per pass
    across all domain branches (grid.y = branch — late-layer sites are
    launch-bound otherwise, profiles/norm_bench.md); the NCHW launchers
    launch the branches one after another on offsets into the same stacked
    tensors; the matrix-function kernels always see the stacked group axis."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_means, running_vars, cfg,
                stats_acc=None, res=None):
        # stats_acc: see _usable_stats_acc
        # res (channels_last layout only; passed by _HipWhitenJoin, never
        # through apply): the apply pass writes relu(norm(x) + res)
        ext = _ext()
        parts = cfg["parts"]
        g = x.shape[1] // cfg["num_groups"]
        eps, momentum = cfg["eps"], cfg["momentum"]
        training, mode, relu = cfg["training"], cfg["mode"], cfg["relu"]
        track = cfg.get("track_running_stats", True)
        ns_iters = cfg.get("ns_iters", 7)
        use_batch = training or not track

        c = x.shape[1]
        layout = _whiten_layout(x, c, g)
        if layout == "nchw":
            x = x.contiguous()
        n, c, h, w = x.shape
        assert n % parts == 0,             f"batch {n} not divisible by {parts} domain branches"
        b = n // parts
        n_groups = c // g
        ng_all = parts * n_groups
        dev = x.device
        m_count = b * h * w

        has_affine, gflat, bflat = _flat_affine(gamma, beta, c, x)

        # world > 1 only with stats_sync: cross-rank (SyncBN-style) statistics
        world = _dist_world()[1] if cfg.get("stats_sync") and use_batch else 1
        ctx_count = m_count * world  # global positions per branch

        out = torch.empty_like(x)
        if use_batch:
            # raw sums (from the producing conv's epilogue, or a partial pass
            # here) -> all-reduce -> finalize over the global batch
            acc = _usable_stats_acc(stats_acc, x, layout, training,
                                    ng_all * (g + g * g))
            if acc is None:
                acc = torch.zeros(ng_all * (g + g * g), device=dev, dtype=torch.float32)
                if layout == "cl":
                    ext.whiten_stats_partial_cl(x, acc, g, c, m_count, parts)
                else:
                    ext.whiten_stats_partial(x, acc, g, parts)
            if world > 1:
                _allreduce(acc)
            mean = torch.empty(parts * c, device=dev, dtype=torch.float32)
            cov = torch.empty(ng_all, g, g, device=dev, dtype=torch.float32)
            ext.whiten_stats_final(acc, mean, cov, g, ng_all, ctx_count)
        else:
            mean = torch.stack([_f32c(running_means[p]).reshape(c)
                                for p in range(parts)]).reshape(-1).contiguous()
            cov = torch.stack([_f32c(running_vars[p]).reshape(n_groups, g, g)
                               for p in range(parts)]).reshape(ng_all, g, g).contiguous()

        wmat = torch.empty(ng_all, g, g, device=dev, dtype=torch.float32)
        if mode == "chol":
            ell = torch.empty_like(wmat)
            ext.matfn_chol_fwd(cov, wmat, ell, eps)
            saved_mat = ell
        else:
            ys = torch.empty(ng_all, ns_iters, g, g, device=dev, dtype=torch.float32)
            zs = torch.empty_like(ys)
            svals = torch.empty(ng_all, device=dev, dtype=torch.float32)
            ext.matfn_ns_fwd(cov, wmat, ys, zs, svals, eps, ns_iters)
            saved_mat = (ys, zs, svals)

        if res is not None:
            assert layout == "cl"
            ext.whiten_apply_res_cl(x, mean, wmat, gflat, bflat, res, out, g,
                                    c, m_count, True, has_affine, parts)
        elif layout == "cl":
            ext.whiten_apply_cl(x, mean, wmat, gflat, bflat, out, g, c,
                                m_count, relu, has_affine, parts)
        else:
            ext.whiten_apply(x, mean, wmat, gflat, bflat, out, g, relu,
                             has_affine, parts)

        if training and track and running_means is not None:
            with torch.no_grad():
                for p in range(parts):
                    _ema_update(ext, running_means[p], mean[p * c:(p + 1) * c],
                                running_vars[p],
                                cov[p * n_groups:(p + 1) * n_groups], momentum)

        ctx.cfg = cfg
        ctx.g = g
        ctx.layout = layout
        ctx.m_count = ctx_count   # global positions per branch (for 1/m)
        ctx.m_local = m_count     # this rank's rows per branch (kernel M)
        ctx.sync_world = world
        ctx.mean = mean
        ctx.wmat = wmat
        ctx.saved_mat = saved_mat
        ctx.has_affine = has_affine
        ctx.gflat = gflat
        ctx.bflat = bflat
        ctx.save_for_backward(x, gamma, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, _, dgamma, dbeta = _HipWhitenMulti.run_backward(ctx, dout)
        return dx, dgamma, dbeta, None, None, None, None

    @staticmethod
    def run_backward(ctx, dout, gb=None, join=False):
        """Returns (dx, gid, dgamma, dbeta).  ``join``: ``dout``/``gb`` are
        the two consumers' gradients of y = relu(norm(x) + identity) (gb may
        be None); the join reduce writes gid = (dout + gb) * (y > 0), which
        is the identity's gradient and the dout of the plain apply pass."""
        ext = _ext()
        cfg = ctx.cfg
        parts, relu, mode, eps = cfg["parts"], cfg["relu"], cfg["mode"], cfg["eps"]
        training = cfg["training"]
        track = cfg.get("track_running_stats", True)
        ns_iters = cfg.get("ns_iters", 7)
        use_batch = training or not track
        g = ctx.g
        x, gamma, out = ctx.saved_tensors
        c = x.shape[1]
        ng_all = parts * (c // g)
        dev = x.device
        layout = ctx.layout
        if layout == "cl":
            dout = dout.contiguous(memory_format=torch.channels_last)
        else:
            dout = dout.contiguous()
        mean, wmat = ctx.mean, ctx.wmat
        m_count = ctx.m_count
        # the kernels index x with the LOCAL per-branch row count; the global
        # count (sync-stats mode) only enters through inv_m
        m_local = ctx.m_local

        dgb = torch.zeros(parts, 2, c, device=dev, dtype=torch.float32)
        dW = torch.zeros(ng_all, g, g, device=dev, dtype=torch.float32)
        dx = torch.empty_like(x)

        gid = None
        if join:
            assert layout == "cl"
            if gb is not None:
                gb = gb.contiguous(memory_format=torch.channels_last)
            gid = torch.empty_like(x)
            ext.whiten_join_bwd_reduce_cl(x, out, dout, gb, mean, wmat,
                                          ctx.gflat, gid, dW, dgb.reshape(-1),
                                          g, c, m_local, ctx.has_affine, parts)
            dout, relu = gid, False
        elif layout == "cl":
            ext.whiten_bwd_reduce_cl(x, dout, mean, wmat, ctx.gflat, ctx.bflat,
                                     dW, dgb.reshape(-1), g, c, m_local,
                                     relu, ctx.has_affine, parts)
        else:
            ext.whiten_bwd_reduce(x, dout, out, mean, wmat, ctx.gflat, dW,
                                  dgb.reshape(-1), g, relu, ctx.has_affine,
                                  parts)

        if use_batch:
            gdb = (ctx.gflat.float().unsqueeze(0) * dgb[:, 1]) if ctx.has_affine \
                else dgb[:, 1]
            gdb = gdb.reshape(-1).contiguous()
            dW_in = dW
            if ctx.sync_world > 1:
                # global-batch statistics: the matrix-function backward sees
                # the cross-rank sums (dgamma/dbeta stay LOCAL — the DP
                # gradient all-reduce handles parameter grads)
                dW_in = _allreduce(dW.clone())
                gdb = _allreduce(gdb.clone())
            S = torch.empty(ng_all, g, g, device=dev, dtype=torch.float32)
            corr = torch.empty(parts * c, device=dev, dtype=torch.float32)
            inv_m = 1.0 / m_count
            if mode == "chol":
                ext.matfn_chol_bwd(dW_in, wmat, ctx.saved_mat, gdb, S, corr,
                                   eps, inv_m)
            else:
                ys, zs, svals = ctx.saved_mat
                ext.matfn_ns_bwd(dW_in, wmat, ys, zs, svals, gdb, S, corr,
                                 eps, inv_m, ns_iters)
        else:
            S = torch.empty(0, device=dev)
            corr = torch.empty(0, device=dev)

        if layout == "cl":
            ext.whiten_bwd_apply_cl(x, dout, mean, wmat, ctx.gflat, ctx.bflat,
                                    S, corr, dx, g, c, m_local, relu,
                                    ctx.has_affine, use_batch, parts)
        else:
            ext.whiten_bwd_apply(x, dout, out, mean, wmat, ctx.gflat, S, corr,
                                 dx, g, relu, ctx.has_affine, use_batch, parts)

        if ctx.has_affine:
            dgamma = dgb[:, 0].sum(0).reshape(gamma.shape).to(gamma.dtype)
            dbeta = dgb[:, 1].sum(0).reshape(gamma.shape).to(gamma.dtype)
        else:
            dgamma = dbeta = None
        return dx, gid, dgamma, dbeta


def join_supported(kind, x, identity, cfg):
    """True when the fused residual join serves this site: channels_last
    fp32/bf16 in the NHWC kernels' (C, g) range, identity shaped and laid
    out like x (an identity in another layout would need a hidden copy pass,
    so such a site takes the unfused composition instead)."""
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 4:
        return False
    if identity.shape != x.shape or identity.dtype != x.dtype \
            or identity.device != x.device \
            or identity.stride() != x.stride():
        return False
    c = x.shape[1]
    if kind == "whiten":
        return _whiten_layout(x, c, c // cfg["num_groups"]) == "cl"
    return _bn_layout(x, c) == "cl"


def whiten_join(x, identity, gamma, beta, running_means, running_vars, cfg,
                stats_acc=None):
    return _HipWhitenJoin.apply(x, identity, gamma, beta, running_means,
                                running_vars, cfg, stats_acc)


def batch_norm_join(x, identity, gamma, beta, running_means, running_vars, cfg,
                    stats_acc=None):
    return _HipBatchNormJoin.apply(x, identity, gamma, beta, running_means,
                                   running_vars, cfg, stats_acc)


def whiten_multi(x, gamma, beta, running_means, running_vars, cfg,
                 stats_acc=None):
    g = x.shape[1] // cfg["num_groups"]
    if g > _GEN_G_MAX or x.dtype not in (torch.float32, torch.bfloat16):
        _warn_once(("wh", g, x.dtype),
                   f"dwt_amd: whiten_multi g={g} dtype={x.dtype} uses the "
                   "torch path (HIP kernels cover g <= 32, fp32/bf16)")
        from ..ops.functional import WhitenMulti
        # the torch path takes its own statistics
        return WhitenMulti.apply(x, gamma, beta, running_means, running_vars, cfg)
    return _HipWhitenMulti.apply(x, gamma, beta, running_means, running_vars,
                                 cfg, stats_acc)


class _HipBatchNormMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_means, running_vars, cfg,
                stats_acc=None, res=None):
        # stats_acc, res: as in _HipWhitenMulti.forward
        ext = _ext()
        parts = cfg["parts"]
        eps, momentum = cfg["eps"], cfg["momentum"]
        training, relu = cfg["training"], cfg["relu"]
        track = cfg.get("track_running_stats", True)
        use_batch = training or not track

        spatial = x.dim() == 4
        c = x.shape[1]
        layout = _bn_layout(x, c)
        if layout == "nchw" or x.dim() == 2:
            x = x.contiguous()
        n = x.shape[0]
        assert n % parts == 0,             f"batch {n} not divisible by {parts} domain branches"
        dev = x.device
        cnt = (x.numel() // parts) // c

        has_affine, gflat, bflat = _flat_affine(gamma, beta, c, x)

        # as in _HipWhitenMulti.forward
        world = _dist_world()[1] if cfg.get("stats_sync") and use_batch else 1
        cnt_total = cnt * world

        out = torch.empty_like(x)
        if use_batch:
            acc = _usable_stats_acc(stats_acc, x, layout, training,
                                    parts * 2 * c)
            if acc is None:
                acc = torch.zeros(parts * 2 * c, device=dev, dtype=torch.float32)
                if layout == "cl":
                    ext.bn_stats_partial_cl(x, acc, c, cnt, parts)
                else:
                    ext.bn_stats_partial(x, acc, parts)
            if world > 1:
                _allreduce(acc)
            mean = torch.empty(parts * c, device=dev, dtype=torch.float32)
            istd = torch.empty(parts * c, device=dev, dtype=torch.float32)
            var_unb = torch.empty(parts * c, device=dev, dtype=torch.float32)
            ext.bn_stats_final(acc, mean, istd, var_unb, c, parts, cnt_total,
                               eps)
            if training and track and running_means is not None:
                with torch.no_grad():
                    for p in range(parts):
                        _ema_update(ext, running_means[p],
                                    mean[p * c:(p + 1) * c], running_vars[p],
                                    var_unb[p * c:(p + 1) * c], momentum)
        else:
            mean = torch.stack([_f32c(running_means[p]).reshape(c)
                                for p in range(parts)]).reshape(-1).contiguous()
            var = torch.stack([_f32c(running_vars[p]).reshape(c)
                               for p in range(parts)]).reshape(-1)
            istd = torch.rsqrt(var + eps).contiguous()

        if res is not None:
            assert layout == "cl" and x.dim() == 4
            ext.bn_apply_res_cl(x, mean, istd, gflat, bflat, res, out, c, cnt,
                                True, has_affine, parts)
        elif layout == "cl":
            ext.bn_apply_cl(x, mean, istd, gflat, bflat, out, c, cnt, relu,
                            has_affine, parts)
        else:
            ext.bn_apply(x, mean, istd, gflat, bflat, out, relu, has_affine,
                         parts)

        ctx.cfg = cfg
        ctx.layout = layout
        ctx.cnt = cnt
        ctx.cnt_total = cnt_total
        ctx.sync_world = world
        ctx.spatial = spatial
        ctx.mean = mean
        ctx.istd = istd
        ctx.has_affine = has_affine
        ctx.gflat = gflat
        ctx.bflat = bflat
        ctx.use_batch = use_batch
        ctx.save_for_backward(x, gamma, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, _, dgamma, dbeta = _HipBatchNormMulti.run_backward(ctx, dout)
        return dx, dgamma, dbeta, None, None, None, None

    @staticmethod
    def run_backward(ctx, dout, gb=None, join=False):
        """Returns (dx, gid, dgamma, dbeta); ``join`` as in
        _HipWhitenMulti.run_backward."""
        ext = _ext()
        cfg = ctx.cfg
        parts, relu = cfg["parts"], cfg["relu"]
        x, gamma, out = ctx.saved_tensors
        c = x.shape[1]
        dev = x.device
        layout = ctx.layout
        if layout == "cl" and x.dim() == 4:
            dout = dout.contiguous(memory_format=torch.channels_last)
        else:
            dout = dout.contiguous()
        mean, istd = ctx.mean, ctx.istd

        sums = torch.zeros(parts, 2, c, device=dev, dtype=torch.float32)
        dx = torch.empty_like(x)
        gid = None
        if join:
            assert layout == "cl"
            if gb is not None:
                gb = gb.contiguous(memory_format=torch.channels_last)
            gid = torch.empty_like(x)
            ext.bn_join_bwd_reduce_cl(x, out, dout, gb, mean, istd, gid,
                                      sums.reshape(-1), c, ctx.cnt, parts)
            dout, relu = gid, False
        elif layout == "cl":
            ext.bn_bwd_reduce_cl(x, dout, mean, istd, ctx.gflat, ctx.bflat,
                                 sums.reshape(-1), c, ctx.cnt, relu,
                                 ctx.has_affine, parts)
        else:
            ext.bn_bwd_reduce(x, dout, out, mean, istd, sums.reshape(-1), relu,
                              parts)

        # global-batch statistics: the apply pass sees the cross-rank sums
        # (dgamma / dbeta below stay local, as in _HipWhitenMulti)
        apply_sums = sums.reshape(-1)
        if ctx.sync_world > 1:
            apply_sums = _allreduce(apply_sums.clone())
        if layout == "cl":
            ext.bn_bwd_apply_cl(x, dout, mean, istd, ctx.gflat, ctx.bflat,
                                apply_sums, dx, c, ctx.cnt, relu,
                                ctx.has_affine, ctx.use_batch, parts,
                                ctx.cnt_total)
        else:
            ext.bn_bwd_apply(x, dout, out, mean, istd, ctx.gflat, apply_sums,
                             dx, relu, ctx.has_affine, ctx.use_batch,
                             ctx.cnt_total, parts)

        if ctx.has_affine:
            # dgamma = sum dy * xhat ; dbeta = sum dy  (sums[:,1] is dy*xhat)
            dgamma = sums[:, 1].sum(0).reshape(gamma.shape).to(gamma.dtype)
            dbeta = sums[:, 0].sum(0).reshape(gamma.shape).to(gamma.dtype)
        else:
            dgamma = dbeta = None
        return dx, gid, dgamma, dbeta


def _join_function(name, site):
    """y = relu(site(x) + identity) with the join fused into the apply pass
    (forward) and into the reduce pass (backward); channels_last only.

    Returns TWO outputs aliasing one buffer, one per consumer of a block
    output (the next block's conv1 and its identity).  Backward then gets
    the two gradients un-summed (either may be None) and adds them inside
    the join reduce kernel — autograd never runs its accumulation kernel."""

    def forward(ctx, x, identity, gamma, beta, running_means, running_vars,
                cfg, stats_acc=None):
        ctx.set_materialize_grads(False)
        res = identity.detach()  # channels_last: join_supported checked it
        y = site.forward(ctx, x, gamma, beta, running_means, running_vars,
                         cfg, stats_acc, res=res)
        return y, y.view_as(y)

    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return (None,) * 8
        if ga is None:
            ga, gb = gb, None
        dx, gid, dgamma, dbeta = site.run_backward(ctx, ga, gb, join=True)
        return dx, gid, dgamma, dbeta, None, None, None, None

    return type(name, (torch.autograd.Function,),
                {"__doc__": _join_function.__doc__,
                 "forward": staticmethod(forward),
                 "backward": staticmethod(backward)})


_HipWhitenJoin = _join_function("_HipWhitenJoin", _HipWhitenMulti)
_HipBatchNormJoin = _join_function("_HipBatchNormJoin", _HipBatchNormMulti)


def batch_norm_multi(x, gamma, beta, running_means, running_vars, cfg,
                     stats_acc=None):
    if x.dtype not in (torch.float32, torch.bfloat16):
        from ..ops.functional import BatchNormMulti
        return BatchNormMulti.apply(x, gamma, beta, running_means, running_vars, cfg)
    return _HipBatchNormMulti.apply(x, gamma, beta, running_means, running_vars,
                                    cfg, stats_acc)


class _HipMecLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        ext = _ext()
        x32 = x.detach().to(torch.float32).contiguous()
        y32 = y.detach().to(torch.float32).contiguous()
        n, k = x32.shape
        lx = torch.empty_like(x32)
        ly = torch.empty_like(y32)
        amin = torch.empty(n, device=x.device, dtype=torch.int32)
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        ext.mec_fwd(x32, y32, lx, ly, amin, loss)
        ctx.save_for_backward(lx, ly, amin)
        ctx.dtypes = (x.dtype, y.dtype)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        ext = _ext()
        lx, ly, amin = ctx.saved_tensors
        gscale = dloss.detach().to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(lx)
        dy = torch.empty_like(ly)
        ext.mec_bwd(lx, ly, amin, gscale, dx, dy)
        return dx.to(ctx.dtypes[0]), dy.to(ctx.dtypes[1])


class _HipEntropyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = _ext()
        x32 = x.detach().to(torch.float32).contiguous()
        n, k = x32.shape
        q = torch.empty_like(x32)
        hper = torch.empty(n, device=x.device, dtype=torch.float32)
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        ext.entropy_fwd(x32, q, hper, loss)
        ctx.save_for_backward(q, hper)
        ctx.dtype = x.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        ext = _ext()
        q, hper = ctx.saved_tensors
        gscale = dloss.detach().to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(q)
        ext.entropy_bwd(q, hper, gscale, dx)
        return dx.to(ctx.dtype)


def mec_loss(x, y):
    return _HipMecLoss.apply(x, y)


def entropy_loss(x):
    return _HipEntropyLoss.apply(x)


class _HipCELoss(torch.autograd.Function):
    """mean_n -log softmax(x)[n, target_n] (reference source loss)."""

    @staticmethod
    def forward(ctx, x, target):
        ext = _ext()
        x32 = x.detach().to(torch.float32).contiguous()
        q = torch.empty_like(x32)
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        ext.ce_fwd(x32, target.contiguous(), q, loss)
        ctx.save_for_backward(q, target)
        ctx.dtype = x.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        ext = _ext()
        q, target = ctx.saved_tensors
        gscale = dloss.detach().to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(q)
        ext.ce_bwd(q, target.contiguous(), gscale, dx)
        return dx.to(ctx.dtype), None


def ce_loss(x, target):
    return _HipCELoss.apply(x, target)
