"""Wide (16-byte) against narrow (8-byte) forms of the bf16 NHWC norm kernels.

The extension's entry points are called directly, once with the wide forms
allowed (``set_norm_wide(True)``) and once forced narrow, on identical inputs,
statistics and sums.

* Elementwise outputs (``*_apply`` with and without ``res``, ``*_bwd_apply``,
  the ``gid`` of the join reduce) must be ``torch.equal``: every element is
  the same fp32 expression with one rounding in both forms.
* Reduction outputs (statistics accumulators, ``sums``, ``dW``/``dgb``) are
  checked for each form on its own against the same sum taken in fp64 from
  the same bf16 inputs, with the worst case of fp32 accumulation as the bound:
  ``|err| <= M * 2^-24 * sum|term|``.

For that bound to speak about the accumulation alone, every TERM has to be
the same number in the kernel's fp32 and in the fp64 reference.  The terms of
the statistics are: x and x_i * x_j of bf16 values are exact in fp32.  The
terms of the backward reduces (dy * xhat, dy_i * gamma_i * (x_j - mean_j),
dy_i * (W (x - mean))_i) are not in general, and at M = 1 the bound is half an
ulp of a single term.  So the backward-reduce cases draw their inputs,
statistics and parameters from coarse dyadic grids (eighths, quarters,
halves, small ranges) on which every intermediate of a term is exact in fp32
whether or not the compiler contracts it into an fma; x stays a bf16 tensor.
The arithmetic of the terms on general inputs is what the elementwise cases
here and the existing suites cover.

Shapes are (C, B per part, H, W), bf16, 3 parts.  ``off`` places the streamed
tensors at element offset 4 of a larger bf16 buffer: 8-byte aligned only, so
the launchers must take the narrow form and stay right.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

PARTS = 3
G = 4
U = 2.0 ** -24

# id -> (C, M per part, element offset, must the wide form be taken)
BN_CASES = {
    "c64_m9": (64, 1 * 3 * 3, 0, True),        # 8 lanes per row, M odd
    "c128_m140": (128, 4 * 7 * 5, 0, True),    # mid-size
    "c2048_m4": (2048, 1 * 2 * 2, 0, True),    # two slices, M < rows per block
    "2d_n37_c256": (256, 37, 0, True),         # the (N, C) entry point's shape
    "c4": (4, 2 * 3 * 3, 0, False),            # C % 8 != 0: narrow
    "c64_m9_off4": (64, 9, 4, False),          # 8-byte aligned only: narrow
}
WH_CASES = {
    "c64_m9": (64, 9, 0, True),                # M odd: a pair lacks its 2nd row
    "c64_m1": (64, 1, 0, True),                # M = 1
    "c256_m18": (256, 2 * 3 * 3, 0, True),     # mid-size
    "c512_m8": (512, 2 * 2 * 2, 0, True),      # two slices
    "c64_m9_off4": (64, 9, 4, False),          # 8-byte aligned only: narrow
}


@pytest.fixture(scope="module")
def ext():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dwt_amd.kernels import dispatch
    assert dispatch.available(), "HIP extension must be built+loaded on a GPU box"
    e = dispatch.ext()
    yield e
    e.set_norm_wide(os.environ.get("DWT_AMD_NORM_WIDE", "1") != "0")


DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _place(t, off):
    """t (bf16, any shape) on the device; with off, as a view at that element
    offset of a larger buffer."""
    t = t.to(torch.bfloat16)
    if not off:
        return t.to(DEV).contiguous()
    buf = torch.zeros(t.numel() + 16, dtype=torch.bfloat16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2 * off
    return v


def _normal(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _grid(gen, lo, hi, den, *shape):
    """Uniform on {lo, ..., hi} / den (fp32, exact)."""
    return torch.randint(lo, hi + 1, shape, generator=gen).float() / den


def _both(ext, fn):
    """fn() with the wide forms allowed, then forced narrow."""
    ext.set_norm_wide(True)
    wide = fn()
    ext.set_norm_wide(False)
    narrow = fn()
    ext.set_norm_wide(True)
    torch.cuda.synchronize()
    return wide, narrow


def _assert_selected(ext, kind, tensors, c, expect):
    ext.set_norm_wide(True)
    assert ext.norm_wide_selected(kind, list(tensors), G, c) == expect
    ext.set_norm_wide(False)
    assert not ext.norm_wide_selected(kind, list(tensors), G, c)
    ext.set_norm_wide(True)


def _assert_within(name, got, ref, abs_terms, m):
    """|got - ref| <= m * 2^-24 * sum|term|, right side in fp64."""
    err = (got.double().cpu() - ref).abs()
    bound = m * U * abs_terms
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, min slack {-worst:.3e}")
    assert worst <= 0.0, f"{name}: exceeds the fp32 accumulation bound by {worst:.3e}"


# ------------------------------- BN ---------------------------------------

def _bn_elem_inputs(c, m, off, seed):
    gen = _gen(seed)
    t = {k: _place(_normal(gen, PARTS, m, c), off)
         for k in ("x", "res", "dout", "y", "ga", "gb")}
    t["mean"] = _normal(gen, PARTS * c, scale=0.3).to(DEV)
    t["istd"] = (torch.rand(PARTS * c, generator=gen) + 0.5).to(DEV)
    t["gamma"] = _normal(gen, c).to(torch.bfloat16).to(DEV)
    t["beta"] = _normal(gen, c).to(torch.bfloat16).to(DEV)
    t["sums"] = _normal(gen, PARTS * 2 * c, scale=float(m) ** 0.5).to(DEV)
    return t


@pytest.mark.parametrize("case", BN_CASES)
def test_bn_elementwise_equal(ext, case):
    c, m, off, expect = BN_CASES[case]
    t = _bn_elem_inputs(c, m, off, seed=11)
    _assert_selected(ext, "bn", [t["x"], t["res"], t["dout"]], c, expect)

    def run():
        outs = []
        for res in (None, t["res"]):
            out = _place(torch.zeros(PARTS, m, c), off)
            ext.bn_apply_res_cl(t["x"], t["mean"], t["istd"], t["gamma"],
                                t["beta"], res, out, c, m, True, True, PARTS)
            outs.append(out.clone())
        dx = _place(torch.zeros(PARTS, m, c), off)
        ext.bn_bwd_apply_cl(t["x"], t["dout"], t["mean"], t["istd"],
                            t["gamma"], t["beta"], t["sums"], dx, c, m, True,
                            True, True, PARTS, m)
        outs.append(dx.clone())
        for gb in (None, t["gb"]):
            gid = _place(torch.zeros(PARTS, m, c), off)
            sums = torch.zeros(PARTS * 2 * c, device=DEV)
            ext.bn_join_bwd_reduce_cl(t["x"], t["y"], t["ga"], gb, t["mean"],
                                      t["istd"], gid, sums, c, m, PARTS)
            outs.append(gid.clone())
        return outs

    wide, narrow = _both(ext, run)
    names = ["apply", "apply_res", "bwd_apply", "gid_one", "gid_two"]
    for name, a, b in zip(names, wide, narrow):
        assert torch.isfinite(a.float()).all(), name
        assert a.float().abs().sum() > 0, name
        assert torch.equal(a, b), f"bn {name}: wide differs from narrow"


@pytest.mark.parametrize("case", BN_CASES)
def test_bn_stats_within_bound(ext, case):
    c, m, off, _ = BN_CASES[case]
    x = _place(_normal(_gen(21), PARTS, m, c), off)
    x64 = x.double().cpu()
    ref = torch.stack([x64.sum(1), (x64 * x64).sum(1)], 1).reshape(-1)
    mag = torch.stack([x64.abs().sum(1), (x64 * x64).sum(1)], 1).reshape(-1)

    def run():
        acc = torch.zeros(PARTS * 2 * c, device=DEV)
        ext.bn_stats_partial_cl(x, acc, c, m, PARTS)
        return acc

    for form, acc in zip(("wide", "narrow"), _both(ext, run)):
        _assert_within(f"bn_stats {case} {form}", acc, ref, mag, m)


def _bn_reduce_inputs(c, m, off, seed):
    """Dyadic grids (module docstring): x, dy in eighths up to 2, mean in
    quarters up to 1, istd in {1/2, 1, 2}, gamma in halves up to 2, beta in
    quarters: xhat has 7 bits at most, dy * xhat 13."""
    gen = _gen(seed)
    t = {k: _place(_grid(gen, -16, 16, 8, PARTS, m, c), off)
         for k in ("x", "dout", "y", "ga", "gb")}
    t["mean"] = _grid(gen, -4, 4, 4, PARTS * c).to(DEV)
    t["istd"] = (2.0 ** _grid(gen, -1, 1, 1, PARTS * c)).to(DEV)
    t["gamma"] = _grid(gen, -4, 4, 2, c).to(torch.bfloat16).to(DEV)
    t["beta"] = _grid(gen, -4, 4, 4, c).to(torch.bfloat16).to(DEV)
    return t


def _bn_sums_ref(t, c, dy, mask):
    """(ref, sum|term|) of sums[p][0] = sum dy, sums[p][1] = sum dy * xhat."""
    x64 = t["x"].double().cpu()
    xh = (x64 - t["mean"].double().cpu().view(PARTS, 1, c)) \
        * t["istd"].double().cpu().view(PARTS, 1, c)
    if mask == "relu":
        pre = t["gamma"].double().cpu() * xh + t["beta"].double().cpu()
        dy = torch.where(pre <= 0, torch.zeros_like(dy), dy)
    terms = torch.stack([dy, dy * xh], 1)          # [P, 2, M, C]
    return terms.sum(2).reshape(-1), terms.abs().sum(2).reshape(-1), dy


@pytest.mark.parametrize("case", BN_CASES)
def test_bn_bwd_reduce_within_bound(ext, case):
    c, m, off, _ = BN_CASES[case]
    t = _bn_reduce_inputs(c, m, off, seed=31)
    ref, mag, _ = _bn_sums_ref(t, c, t["dout"].double().cpu(), "relu")

    def run():
        sums = torch.zeros(PARTS * 2 * c, device=DEV)
        ext.bn_bwd_reduce_cl(t["x"], t["dout"], t["mean"], t["istd"],
                             t["gamma"], t["beta"], sums, c, m, True, True,
                             PARTS)
        return sums

    for form, sums in zip(("wide", "narrow"), _both(ext, run)):
        _assert_within(f"bn_bwd_reduce {case} {form}", sums, ref, mag, m)


@pytest.mark.parametrize("two", [False, True], ids=["one_consumer", "two_consumers"])
@pytest.mark.parametrize("case", BN_CASES)
def test_bn_join_reduce_within_bound(ext, case, two):
    c, m, off, _ = BN_CASES[case]
    t = _bn_reduce_inputs(c, m, off, seed=41)
    g = t["ga"].double().cpu() + (t["gb"].double().cpu() if two else 0.0)
    # eighths up to 4: a bf16 value, so the kernel's rounding of g is exact
    g = torch.where(t["y"].double().cpu() > 0, g, torch.zeros_like(g))
    ref, mag, _ = _bn_sums_ref(t, c, g, None)

    def run():
        sums = torch.zeros(PARTS * 2 * c, device=DEV)
        gid = _place(torch.zeros(PARTS, m, c), off)
        ext.bn_join_bwd_reduce_cl(t["x"], t["y"], t["ga"],
                                  t["gb"] if two else None, t["mean"],
                                  t["istd"], gid, sums, c, m, PARTS)
        return sums, gid.clone()

    for form, (sums, gid) in zip(("wide", "narrow"), _both(ext, run)):
        assert torch.equal(gid.double().cpu(), g), f"gid {form}"
        _assert_within(f"bn_join_reduce {case} {form}", sums, ref, mag, m)


# ---------------------------- whitening g=4 --------------------------------

def _wh_elem_inputs(c, m, off, seed):
    gen = _gen(seed)
    ng = PARTS * c // G
    t = {k: _place(_normal(gen, PARTS, m, c), off)
         for k in ("x", "res", "dout", "y", "ga", "gb")}
    t["mean"] = _normal(gen, PARTS * c, scale=0.3).to(DEV)
    t["W"] = _normal(gen, ng, G, G, scale=0.5).to(DEV)
    t["S"] = _normal(gen, ng, G, G, scale=0.5).to(DEV)
    t["corr"] = _normal(gen, PARTS * c, scale=0.3).to(DEV)
    t["gamma"] = _normal(gen, c).to(torch.bfloat16).to(DEV)
    t["beta"] = _normal(gen, c).to(torch.bfloat16).to(DEV)
    return t


@pytest.mark.parametrize("case", WH_CASES)
def test_whiten_elementwise_equal(ext, case):
    c, m, off, expect = WH_CASES[case]
    t = _wh_elem_inputs(c, m, off, seed=51)
    _assert_selected(ext, "whiten", [t["x"], t["res"], t["dout"]], c, expect)
    ng = PARTS * c // G

    def run():
        outs = []
        for res in (None, t["res"]):
            out = _place(torch.zeros(PARTS, m, c), off)
            ext.whiten_apply_res_cl(t["x"], t["mean"], t["W"], t["gamma"],
                                    t["beta"], res, out, G, c, m, True, True,
                                    PARTS)
            outs.append(out.clone())
        dx = _place(torch.zeros(PARTS, m, c), off)
        ext.whiten_bwd_apply_cl(t["x"], t["dout"], t["mean"], t["W"],
                                t["gamma"], t["beta"], t["S"], t["corr"], dx,
                                G, c, m, True, True, True, PARTS)
        outs.append(dx.clone())
        for gb in (None, t["gb"]):
            gid = _place(torch.zeros(PARTS, m, c), off)
            dW = torch.zeros(ng, G, G, device=DEV)
            dgb = torch.zeros(PARTS * 2 * c, device=DEV)
            ext.whiten_join_bwd_reduce_cl(t["x"], t["y"], t["ga"], gb,
                                          t["mean"], t["W"], t["gamma"], gid,
                                          dW, dgb, G, c, m, True, PARTS)
            outs.append(gid.clone())
        return outs

    wide, narrow = _both(ext, run)
    names = ["apply", "apply_res", "bwd_apply", "gid_one", "gid_two"]
    for name, a, b in zip(names, wide, narrow):
        assert torch.isfinite(a.float()).all(), name
        assert a.float().abs().sum() > 0, name
        assert torch.equal(a, b), f"whiten {name}: wide differs from narrow"


@pytest.mark.parametrize("case", WH_CASES)
def test_whiten_stats_within_bound(ext, case):
    c, m, off, _ = WH_CASES[case]
    ng = PARTS * c // G
    x = _place(_normal(_gen(61), PARTS, m, c), off)
    xg = x.double().cpu().view(PARTS, m, c // G, G)
    # acc[group] = [sum x_i (G), sum x_i x_j (G x G, lower triangle)]
    outer = torch.tril(torch.ones(G, G, dtype=torch.float64)) \
        * xg.unsqueeze(-1) * xg.unsqueeze(-2)               # [P, M, NG, G, G]
    ref = torch.cat([xg.sum(1), outer.sum(1).flatten(-2)], -1).reshape(-1)
    mag = torch.cat([xg.abs().sum(1), outer.abs().sum(1).flatten(-2)],
                    -1).reshape(-1)

    def run():
        acc = torch.zeros(ng * (G + G * G), device=DEV)
        ext.whiten_stats_partial_cl(x, acc, G, c, m, PARTS)
        return acc

    for form, acc in zip(("wide", "narrow"), _both(ext, run)):
        _assert_within(f"whiten_stats {case} {form}", acc, ref, mag, m)


def _wh_reduce_inputs(c, m, off, seed):
    """Dyadic grids (module docstring): x, dy in eighths up to 2, mean in
    quarters up to 1, W in halves up to 2, gamma in halves up to 2, beta in
    quarters: x - mean has 6 bits, y0 = W (x - mean) sixteenths up to 24
    (9 bits), dy * y0 and dy * gamma * (x - mean) 14 bits at most."""
    gen = _gen(seed)
    ng = PARTS * c // G
    t = {k: _place(_grid(gen, -16, 16, 8, PARTS, m, c), off)
         for k in ("x", "dout", "y", "ga", "gb")}
    t["mean"] = _grid(gen, -4, 4, 4, PARTS * c).to(DEV)
    t["W"] = _grid(gen, -4, 4, 2, ng, G, G).to(DEV)
    t["gamma"] = _grid(gen, -4, 4, 2, c).to(torch.bfloat16).to(DEV)
    t["beta"] = _grid(gen, -4, 4, 4, c).to(torch.bfloat16).to(DEV)
    return t


def _wh_reduce_ref(t, c, m, dy, mask):
    """fp64 (dW, dgb) and their sum|term| for per-position gradient dy
    [P, M, C]: dgb[p] = [sum dy * y0, sum dy] and dW[group][i][j] =
    sum dy_i gamma_i (x_j - mean_j), with y0 = W (x - mean)."""
    ngp = c // G
    xc = (t["x"].double().cpu()
          - t["mean"].double().cpu().view(PARTS, 1, c)).view(PARTS, m, ngp, G)
    W = t["W"].double().cpu().view(PARTS, 1, ngp, G, G)
    y0 = (W * xc.unsqueeze(-2)).sum(-1)                     # [P, M, NG, G]
    gm = t["gamma"].double().cpu().view(ngp, G)
    bt = t["beta"].double().cpu().view(ngp, G)
    dy = dy.view(PARTS, m, ngp, G)
    if mask == "relu":
        dy = torch.where(gm * y0 + bt <= 0, torch.zeros_like(dy), dy)
    tg = torch.stack([dy * y0, dy], 1).reshape(PARTS, 2, m, c)
    tw = (dy * gm).unsqueeze(-1) * xc.unsqueeze(-2)         # [P, M, NG, G, G]
    return (tw.sum(1).reshape(-1), tw.abs().sum(1).reshape(-1),
            tg.sum(2).reshape(-1), tg.abs().sum(2).reshape(-1))


@pytest.mark.parametrize("case", WH_CASES)
def test_whiten_bwd_reduce_within_bound(ext, case):
    c, m, off, _ = WH_CASES[case]
    ng = PARTS * c // G
    t = _wh_reduce_inputs(c, m, off, seed=71)
    dw_ref, dw_mag, dgb_ref, dgb_mag = _wh_reduce_ref(
        t, c, m, t["dout"].double().cpu(), "relu")

    def run():
        dW = torch.zeros(ng, G, G, device=DEV)
        dgb = torch.zeros(PARTS * 2 * c, device=DEV)
        ext.whiten_bwd_reduce_cl(t["x"], t["dout"], t["mean"], t["W"],
                                 t["gamma"], t["beta"], dW, dgb, G, c, m,
                                 True, True, PARTS)
        return dW.reshape(-1), dgb

    for form, (dW, dgb) in zip(("wide", "narrow"), _both(ext, run)):
        _assert_within(f"whiten dW {case} {form}", dW, dw_ref, dw_mag, m)
        _assert_within(f"whiten dgb {case} {form}", dgb, dgb_ref, dgb_mag, m)


@pytest.mark.parametrize("two", [False, True], ids=["one_consumer", "two_consumers"])
@pytest.mark.parametrize("case", WH_CASES)
def test_whiten_join_reduce_within_bound(ext, case, two):
    c, m, off, _ = WH_CASES[case]
    ng = PARTS * c // G
    t = _wh_reduce_inputs(c, m, off, seed=81)
    g = t["ga"].double().cpu() + (t["gb"].double().cpu() if two else 0.0)
    g = torch.where(t["y"].double().cpu() > 0, g, torch.zeros_like(g))
    dw_ref, dw_mag, dgb_ref, dgb_mag = _wh_reduce_ref(t, c, m, g, None)

    def run():
        dW = torch.zeros(ng, G, G, device=DEV)
        dgb = torch.zeros(PARTS * 2 * c, device=DEV)
        gid = _place(torch.zeros(PARTS, m, c), off)
        ext.whiten_join_bwd_reduce_cl(t["x"], t["y"], t["ga"],
                                      t["gb"] if two else None, t["mean"],
                                      t["W"], t["gamma"], gid, dW, dgb, G, c,
                                      m, True, PARTS)
        return dW.reshape(-1), dgb, gid.clone()

    for form, (dW, dgb, gid) in zip(("wide", "narrow"), _both(ext, run)):
        assert torch.equal(gid.double().cpu(), g), f"gid {form}"
        _assert_within(f"whiten join dW {case} {form}", dW, dw_ref, dw_mag, m)
        _assert_within(f"whiten join dgb {case} {form}", dgb, dgb_ref,
                       dgb_mag, m)


def test_switch_follows_environment(ext):
    """dispatch sets the switch once from DWT_AMD_NORM_WIDE; the module
    fixture restores that setting."""
    x = torch.zeros(PARTS * 9 * 64, dtype=torch.bfloat16, device=DEV)
    ext.set_norm_wide(False)
    assert not ext.norm_wide_selected("bn", [x], G, 64)
    assert not ext.norm_wide_selected("whiten", [x], G, 64)
    ext.set_norm_wide(True)
    assert ext.norm_wide_selected("bn", [x], G, 64)
    assert ext.norm_wide_selected("whiten", [x], G, 64)
    assert not ext.norm_wide_selected("whiten", [x], 2, 64)      # g=2: narrow
    assert not ext.norm_wide_selected("bn", [x.float()], G, 64)  # fp32: narrow
