#!/usr/bin/env python3
"""Folded target-domain inference against `model.eval()`, and the fused conv
kernel against the library composition it replaces, per R50 conv shape.

Two parts, both bf16 channels_last on one GPU:

* end to end: forward time of `model.eval()` (53 norm sites through the norm
  kernels with running statistics) against `fold_resnet(model)` (conv + bias
  [+ identity] [+ ReLU], one launch per conv);
* per conv: `ops.mfma.conv2d_fused_fwd(route=False)` against the library conv
  with bias plus the elementwise op it needs (in-place relu, `add_relu`, or
  nothing for the downsample conv), for every distinct conv of the network.

The two variants of each comparison alternate in one sitting: warm-up, then
`--repeats` rounds of (A x iters, B x iters) timed with device events, medians
reported.  The per-conv table decides `ops.mfma._FUSED_FWD_LIBRARY_SHAPES`: a
shape whose fused time is above the library composition's goes there.

Run on the GPU box:
    python benchmarks/inference_bench.py --out profiles/inference_folded.md
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16


def r50_conv_shapes(layers=(3, 4, 6, 3), img=224):
    """Every distinct conv of the network as
    ``(name, cin, h, cout, k, stride, pad, epilogue, count)``; epilogue is
    "relu", "res+relu" or "none" (the downsample conv)."""
    seen = {}

    def add(name, cin, h, cout, k, s, p, epi):
        key = (cin, h, cout, k, s, p, epi)
        if key in seen:
            seen[key][-1] += 1
        else:
            seen[key] = [name, cin, h, cout, k, s, p, epi, 1]

    add("stem", 3, img, 64, 7, 2, 3, "relu")
    h = (img + 6 - 7) // 2 + 1
    h = (h + 2 - 3) // 2 + 1
    inpl = 64
    for li, (planes, blocks, stride) in enumerate(
            zip((64, 128, 256, 512), layers, (1, 2, 2, 2)), start=1):
        for b in range(blocks):
            s = stride if b == 0 else 1
            add(f"l{li}.{b}.conv1", inpl, h, planes, 1, 1, 0, "relu")
            add(f"l{li}.{b}.conv2", planes, h, planes, 3, s, 1, "relu")
            ho = (h + 2 - 3) // s + 1
            add(f"l{li}.{b}.conv3", planes, ho, planes * 4, 1, 1, 0, "res+relu")
            if b == 0:
                add(f"l{li}.0.ds", inpl, h, planes * 4, 1, s, 0, "none")
            inpl, h = planes * 4, ho
    return [tuple(v) for v in seen.values()]


def time_pair(fn_a, fn_b, iters, repeats, warmup):
    """Median ms per call of two variants, alternated in one sitting."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ta), statistics.median(tb), ta, tb


def per_conv(args, dev):
    from dwt_amd.ops import functional as Fdwt
    from dwt_amd.ops.mfma import conv2d_fused_fwd, fused_fwd_on_kernel
    rows = []
    only = [t for t in args.only.split(",") if t]
    for name, cin, h, cout, k, s, p, epi, count in r50_conv_shapes(img=args.img):
        if only and not any(t in name for t in only):
            continue
        n = args.batch
        ho = (h + 2 * p - k) // s + 1
        x = torch.randn(n, cin, h, h, device=dev).to(BF16) \
            .contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, k, k, device=dev) * 0.05).to(BF16) \
            .contiguous(memory_format=torch.channels_last)
        bias = torch.randn(cout, device=dev)
        b16 = bias.to(BF16)
        res = None
        if epi == "res+relu":
            res = torch.randn(n, cout, ho, ho, device=dev).to(BF16) \
                .contiguous(memory_format=torch.channels_last)
        relu = epi != "none"

        def fused():
            return conv2d_fused_fwd(x, wt, bias, stride=s, padding=p, relu=relu,
                                    residual=res, route=False)

        def lib():
            y = F.conv2d(x, wt, b16, s, p)
            if res is not None:
                return Fdwt.add_relu(y, res)
            return y.relu_() if relu else y

        t_f, t_l, _, _ = time_pair(fused, lib, args.iters, args.repeats,
                                   args.warmup)
        m = n * ho * ho
        gflop = 2.0 * m * cout * k * k * cin / 1e9
        rows.append(dict(name=name, cin=cin, cout=cout, k=k, stride=s, h=h,
                         epilogue=epi, count=count, m=m, fused_ms=t_f,
                         lib_ms=t_l, fused_tflops=gflop / t_f,
                         on_kernel=bool(t_f <= t_l),
                         table_says_kernel=fused_fwd_on_kernel(
                             cin, cout, k, s, res is not None)))
        print(json.dumps(rows[-1]), flush=True)
        del x, wt, res
    return rows


def end_to_end(args, dev):
    from dwt_amd.models import Bottleneck, ResNetDWT, fold_resnet
    torch.manual_seed(0)
    model = ResNetDWT(Bottleneck, [3, 4, 6, 3], None, num_classes=65,
                      whiten_mode=args.whiten_mode)
    model = model.to(dev).to(BF16).to(memory_format=torch.channels_last)
    x = torch.randn(args.batch, 3, args.img, args.img, device=dev).to(BF16) \
        .contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        # a fresh model's running covariance is all ones (near-singular after
        # shrinkage); one training-mode pass at momentum 1 puts batch
        # statistics into every branch, as a trained model would have
        sites = [m for m in model.modules() if hasattr(m, "momentum")
                 and hasattr(m, "running_mean")]
        old = [m.momentum for m in sites]
        for m in sites:
            m.momentum = 1.0
        model.train()
        model(x[:3 * min(16, args.batch // 3)])
        for m, mom in zip(sites, old):
            m.momentum = mom
        model.eval()
        folded = fold_resnet(model)
        ya, yb = model(x).float(), folded(x).float()
        diff = ((ya - yb).abs().max() / ya.abs().max()).item()
        # both against the same weights evaluated in fp32 (first 8 images):
        # how far bf16 evaluation itself is from the function, per path
        import copy
        xs = x[:8]
        oracle = copy.deepcopy(model).float().eval()(xs.float())
        scale = oracle.abs().max()
        err_eval = ((model(xs).float() - oracle).abs().max() / scale).item()
        err_fold = ((folded(xs).float() - oracle).abs().max() / scale).item()
        del oracle

        def run_eval():
            return model(x)

        def run_folded():
            return folded(x)

        t_e, t_f, le, lf = time_pair(run_eval, run_folded, args.e2e_iters,
                                     args.repeats, args.warmup)
        # the folded model with every conv on the kernel, against the routed one
        kern = fold_resnet(model)
        kern.route = False

        def run_kernel():
            return kern(x)

        t_f2, t_k, _, lk = time_pair(run_folded, run_kernel, args.e2e_iters,
                                     args.repeats, args.warmup)
    return dict(batch=args.batch, img=args.img, eval_ms=t_e, folded_ms=t_f,
                folded2_ms=t_f2, kernel_ms=t_k, eval_all=le, folded_all=lf,
                kernel_all=lk, rel_diff=diff, err_eval=err_eval,
                err_fold=err_fold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/inference_folded.md")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e2e_iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--whiten_mode", default="zca")
    ap.add_argument("--only", default="",
                    help="comma-separated substring filter on conv names")
    ap.add_argument("--parts", default="conv,e2e")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "inference_bench needs a GPU"
    from dwt_amd.kernels import dispatch
    assert dispatch.available(), "build the HIP extension first"
    dev = torch.device("cuda:0")
    parts = args.parts.split(",")

    lines = [f"# Folded inference, N={args.batch} at {args.img}x{args.img} "
             "(bf16, NHWC, one MI355X)", ""]
    if "conv" in parts:
        rows = per_conv(args, dev)
        lines += [
            "## Per conv: fused kernel vs library composition", "",
            f"Median ms per call over {args.repeats} alternated rounds of "
            f"{args.iters} calls.  `library` = library conv with bias + the "
            "elementwise op the epilogue stands for (in-place relu, "
            "`add_relu`, nothing for the downsample conv).  `routed to` is "
            "what this sitting's times decide; `count` = occurrences in the "
            "network.", "",
            "| conv | Cin x HxH -> Cout, k/s | epilogue | count | fused ms | "
            "library ms | lib/fused | fused TFLOP/s | routed to |",
            "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(
                f"| {r['name']} | {r['cin']} x {r['h']}x{r['h']} -> {r['cout']}, "
                f"{r['k']}/{r['stride']} | {r['epilogue']} | {r['count']} | "
                f"{r['fused_ms']:.3f} | {r['lib_ms']:.3f} | "
                f"{r['lib_ms'] / r['fused_ms']:.2f}x | {r['fused_tflops']:.0f} | "
                f"{'kernel' if r['on_kernel'] else 'library'} |")
        lose = sorted({(r['cin'], r['cout'], r['k'], r['stride'],
                        r['epilogue'] == 'res+relu')
                       for r in rows if not r['on_kernel']})
        lines += ["", "Shapes `(cin, cout, k, stride, has_residual)` this sitting sends to "
                  "the library composition:", "", "```", repr(lose), "```", ""]
        mism = [r['name'] for r in rows
                if r['table_says_kernel'] != r['on_kernel']]
        lines += [f"Rows where the routing table in `ops/mfma.py` disagrees "
                  f"with this sitting: {mism if mism else 'none'}.", ""]
    if "e2e" in parts:
        e = end_to_end(args, dev)
        print(json.dumps(e), flush=True)
        lines += [
            "## End to end", "",
            f"Forward of the full R50, median ms over {args.repeats} "
            f"alternated rounds of {args.e2e_iters} forwards, routing table "
            "as committed.", "",
            "| variant | ms per forward | img/s |", "|---|---|---|",
            f"| `model.eval()` | {e['eval_ms']:.2f} | "
            f"{args.batch / e['eval_ms'] * 1e3:.0f} |",
            f"| `fold_resnet(model)` | {e['folded_ms']:.2f} | "
            f"{args.batch / e['folded_ms'] * 1e3:.0f} |",
            f"| folded, every conv on the kernel (`route = False`) | "
            f"{e['kernel_ms']:.2f} | {args.batch / e['kernel_ms'] * 1e3:.0f} |",
            "",
            f"(The last row alternated with the routed model, which measured "
            f"{e['folded2_ms']:.2f} ms in that pair.)", "",
            f"eval / folded = {e['eval_ms'] / e['folded_ms']:.2f}x; logits "
            f"differ by {e['rel_diff']:.2e} of max|logit| (bf16).  Against the "
            f"same weights evaluated in fp32 (8 images): `model.eval()` "
            f"{e['err_eval']:.2e}, folded {e['err_fold']:.2e} of max|logit| "
            "(randomly initialised weights, statistics from one batch).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
