#!/usr/bin/env python3
"""Per-shape microbenchmark: hand-written MFMA implicit-GEMM conv/GEMM vs
MIOpen/rocBLAS on the R50 forward shapes. Writes a markdown table.

Run on the GPU box:  python benchmarks/conv_bench.py [--out profiles/conv_bench.md]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

R50_SHAPES = [
    # (name, N, Cin, H, W, Cout, K, stride, pad)
    ("stem7x7", 192, 3, 224, 224, 64, 7, 2, 3),
    ("l1.conv1", 192, 64, 56, 56, 64, 1, 1, 0),
    ("l1.conv2", 192, 64, 56, 56, 64, 3, 1, 1),
    ("l1.conv3", 192, 64, 56, 56, 256, 1, 1, 0),
    ("l2.conv1", 192, 256, 56, 56, 128, 1, 1, 0),
    ("l2.conv2s", 192, 128, 56, 56, 128, 3, 2, 1),
    ("l2.conv3", 192, 128, 28, 28, 512, 1, 1, 0),
    ("l3.conv2", 192, 256, 28, 28, 256, 3, 2, 1),
    ("l3.conv3", 192, 256, 14, 14, 1024, 1, 1, 0),
    ("l4.conv2", 192, 512, 14, 14, 512, 3, 2, 1),
    ("l4.conv3", 192, 512, 7, 7, 2048, 1, 1, 0),
    # the remaining 1x1 stride-1 shapes (conv1 of later blocks / stage entry)
    ("l1.conv1b", 192, 256, 56, 56, 64, 1, 1, 0),
    ("l2.conv1b", 192, 512, 28, 28, 128, 1, 1, 0),
    ("l3.conv1", 192, 512, 28, 28, 256, 1, 1, 0),
    ("l3.conv1b", 192, 1024, 14, 14, 256, 1, 1, 0),
    ("l4.conv1", 192, 1024, 14, 14, 512, 1, 1, 0),
    ("l4.conv1b", 192, 2048, 7, 7, 512, 1, 1, 0),
]

GEMM_SHAPES = [
    ("fc_out", 192, 2048, 65),
    ("sq2048", 2048, 2048, 2048),
    ("sq4096", 4096, 4096, 4096),
]


# every 1x1 stride-1 forward conv of the backbone with the norm site behind
# it: (name, Cin, H=W, Cout, norm kind)
STATS_SHAPES = [
    ("l1.conv1", 64, 56, 64, "whiten"),
    ("l1.conv1b", 256, 56, 64, "whiten"),
    ("l1.conv3/ds", 64, 56, 256, "whiten"),
    ("l2.conv1", 256, 56, 128, "bn"),
    ("l2.conv1b", 512, 28, 128, "bn"),
    ("l2.conv3", 128, 28, 512, "bn"),
    ("l3.conv1", 512, 28, 256, "bn"),
    ("l3.conv1b", 1024, 14, 256, "bn"),
    ("l3.conv3", 256, 14, 1024, "bn"),
    ("l4.conv1", 1024, 14, 512, "bn"),
    ("l4.conv1b", 2048, 7, 512, "bn"),
    ("l4.conv3", 512, 7, 2048, "bn"),
]


def stats_mode(args):
    """Per shape: library forward, the stand-alone stats kernel on its
    output, our forward with the generic epilogue, and the fused forward +
    stats kernel (dwt_amd.ops.mfma.conv1x1_stats), on the register-staged
    main loop (`fused regs`, set_dense_glds(False)) and on the direct-to-LDS
    one (`fused`).  `old/fused` isolates the wide-store epilogue plus the
    stats cost; `(lib+stats)/fused` is what routing a shape gains."""
    from dwt_amd.kernels import dispatch
    from dwt_amd.ops.mfma import (conv2d_fwd, conv_stats_shape_ok,
                                  stats_acc_numel)
    ext = dispatch.ext()
    dev = torch.device("cuda:0")
    n, parts, g = args.batch, 3, 4
    lines = [f"# 1x1 conv forward + norm statistics, N={n} (bf16, NHWC, "
             f"{parts} branches)",
             "",
             "ms per call; `stats` = accumulator zeroing + partial + finalize "
             "kernels on the conv output; `fused` = zeroing + fused conv + "
             "finalize kernel, on the direct-to-LDS main loop; `ours old` = "
             "our forward without statistics, register-staged loop; `gain` = "
             "(lib fwd + stats) / fused; `routed` is `conv_stats_shape_ok` "
             "(gain > 1.05 routes).  The second table sets the fused kernel "
             "on the register-staged loop (`fused regs`, set_dense_glds(False))"
             " beside it.",
             "",
             "| shape | M x Cout x Cin | lib fwd | stats | ours old | fused | "
             "old/fused | gain | fused GB/s | routed |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    loops = ["", "| shape | fused regs | fused | regs/fused | fused TF |",
             "|---|---|---|---|---|"]
    only = [t for t in args.only.split(",") if t]
    for name, cin, hw, cout, kind in STATS_SHAPES:
        if only and not any(t in name for t in only):
            continue
        x = torch.randn(n, cin, hw, hw, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, 1, 1, device=dev) * 0.05).to(torch.bfloat16)
        w2 = wt.reshape(cout, cin).contiguous()
        m = n * hw * hw
        mp = m // parts
        out = torch.empty(n, cout, hw, hw, device=dev, dtype=torch.bfloat16,
                          memory_format=torch.channels_last)
        nacc = stats_acc_numel(kind, cout, parts, g)
        kid = 0 if kind == "bn" else 1

        def lib_fn():
            return F.conv2d(x, wt)

        # both sides as the step runs them: the old path's stats launch is the
        # partial + finalize pair, the fused conv is followed by the finalize
        mean = torch.empty(parts * cout, device=dev, dtype=torch.float32)
        istd, var_unb = torch.empty_like(mean), torch.empty_like(mean)
        ng_all = parts * cout // g
        cov = torch.empty(ng_all, g, g, device=dev, dtype=torch.float32)

        def final(acc):
            if kind == "bn":
                ext.bn_stats_final(acc, mean, istd, var_unb, cout, parts, mp,
                                   1e-5)
            else:
                ext.whiten_stats_final(acc, mean, cov, g, ng_all, mp)

        def stats_fn():
            acc = torch.zeros(nacc, device=dev, dtype=torch.float32)
            if kind == "bn":
                ext.bn_stats_partial_cl(out, acc, cout, mp, parts)
            else:
                ext.whiten_stats_partial_cl(out, acc, g, cout, mp, parts)
            final(acc)

        def old_fn():
            return conv2d_fwd(x, wt)

        def new_fn():
            acc = torch.zeros(nacc, device=dev, dtype=torch.float32)
            ext.conv1x1_stats(x, w2, out, acc, kid, g, parts, 0)
            final(acc)

        t_lib = timeit(lib_fn, args.iters)
        ext.set_dense_glds(False)
        t_old = timeit(old_fn, args.iters)
        t_regs = timeit(new_fn, args.iters)
        ext.set_dense_glds(True)
        t_new = timeit(new_fn, args.iters)   # leaves `out` filled for stats
        t_st = timeit(stats_fn, args.iters)
        gbs = 2.0 * m * (cin + cout) / t_new / 1e9
        tf = 2.0 * m * cin * cout / t_new / 1e12
        lines.append(
            f"| {name} ({kind}) | {m}x{cout}x{cin} | {t_lib*1e3:.3f} | "
            f"{t_st*1e3:.3f} | {t_old*1e3:.3f} | {t_new*1e3:.3f} | "
            f"{t_old/t_new:.2f}x | {(t_lib+t_st)/t_new:.2f}x | {gbs:.0f} | "
            f"{'yes' if conv_stats_shape_ok(m, cin, cout) else 'no'} |")
        loops.append(f"| {name} ({kind}) | {t_regs*1e3:.3f} | {t_new*1e3:.3f} | "
                     f"{t_regs/t_new:.2f}x | {tf:.0f} |")
        print(lines[-1], loops[-1], flush=True)
        del x, out
    with open(args.out, "w") as f:
        f.write("\n".join(lines + loops) + "\n")
    print(f"wrote {args.out}")


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/conv_bench.md")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=192,
                    help="N (the flagship bench step runs N=1536 = 3x512)")
    ap.add_argument("--only", default="",
                    help="comma-separated substring filter on shape names")
    ap.add_argument("--passes", default="fwd,dgrad,wgrad")
    ap.add_argument("--stats", action="store_true",
                    help="1x1 forward + norm-statistics mode (use --batch "
                         "1536 --out profiles/conv_stats_bench_b1536.md)")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    if args.stats:
        return stats_mode(args)
    from dwt_amd.kernels import dispatch
    from dwt_amd.ops.mfma import conv2d_fwd, mfma_gemm
    ext = dispatch.ext()
    dev = torch.device("cuda:0")
    lines = ["# MFMA implicit-GEMM conv/GEMM vs MIOpen/rocBLAS (bf16, NHWC)",
             "",
             "`regs ms` = the dense kernel on the register-staged main loop "
             "(set_dense_glds(False)), for the shapes the direct-to-LDS loop "
             "takes; `ours` is the default.  dgrad times include the "
             "per-call weight transpose.",
             "",
             "| shape | M x N x K | GFLOP | regs ms | ours ms | lib ms | "
             "ours TF | lib TF | ratio |",
             "|---|---|---|---|---|---|---|---|---|"]

    def regs_ms(fn, dense):
        if not dense:
            return "-"
        ext.set_dense_glds(False)
        t = timeit(fn, args.iters)
        ext.set_dense_glds(True)
        return f"{t*1e3:.3f}"

    from dwt_amd.ops.mfma import conv2d_dgrad, conv2d_wgrad

    def lib_dgrad(g, x, wt, stride, pad):
        return torch.ops.aten.convolution_backward(
            g, x, wt, None, [stride, stride], [pad, pad], [1, 1], False,
            [0, 0], 1, [True, False, False])[0]

    def lib_wgrad(g, x, wt, stride, pad):
        return torch.ops.aten.convolution_backward(
            g, x, wt, None, [stride, stride], [pad, pad], [1, 1], False,
            [0, 0], 1, [False, True, False])[1]

    only = [t for t in args.only.split(",") if t]
    passes_on = args.passes.split(",")
    for name, n, cin, h, w, cout, k, stride, pad in R50_SHAPES:
        n = args.batch
        if only and not any(t in name for t in only):
            continue
        x = torch.randn(n, cin, h, w, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(cout, cin, k, k, device=dev) * 0.05).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        p = (h + 2 * pad - k) // stride + 1
        m = n * p * p
        kk = k * k * cin
        g = torch.randn(n, cout, p, p, device=dev).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        gflop = 2.0 * m * cout * kk / 1e9
        passes = [
            ("fwd", lambda: conv2d_fwd(x, wt, stride=stride, padding=pad),
             lambda: F.conv2d(x, wt, stride=stride, padding=pad)),
            ("dgrad", lambda: conv2d_dgrad(g, wt, x.shape, stride=stride, padding=pad),
             lambda: lib_dgrad(g, x, wt, stride, pad)),
            ("wgrad", lambda: conv2d_wgrad(g, x, tuple(wt.shape), stride=stride, padding=pad),
             lambda: lib_wgrad(g, x, wt, stride, pad)),
        ]
        for pname, ours_fn, lib_fn in passes:
            if pname not in passes_on:
                continue
            if pname == "dgrad" and name == "stem7x7":
                continue  # stem never needs dx
            dense = k == 1 and stride == 1 and cin % 64 == 0 \
                and cout % 64 == 0 and pname in ("fwd", "dgrad")
            t_regs = regs_ms(ours_fn, dense)
            t_ours = timeit(ours_fn, args.iters)
            t_lib = timeit(lib_fn, args.iters)
            lines.append(f"| {name}:{pname} | {m}x{cout}x{kk} | {gflop:.1f} | "
                         f"{t_regs} | {t_ours*1e3:.3f} | {t_lib*1e3:.3f} | "
                         f"{gflop/t_ours/1e3:.0f} | {gflop/t_lib/1e3:.0f} | "
                         f"{t_lib/t_ours:.2f}x |")
            print(lines[-1], flush=True)

    for name, m, k, n in GEMM_SHAPES:
        a = torch.randn(m, k, device=dev).to(torch.bfloat16)
        bt = torch.randn(n, k, device=dev).to(torch.bfloat16)
        b = bt.t().contiguous()
        gflop = 2.0 * m * n * k / 1e9
        t_regs = regs_ms(lambda: mfma_gemm(a, bt), k % 64 == 0 and n % 8 == 0)
        t_ours = timeit(lambda: mfma_gemm(a, bt), args.iters)
        t_lib = timeit(lambda: a @ b, args.iters)
        lines.append(f"| gemm:{name} | {m}x{n}x{k} | {gflop:.1f} | "
                     f"{t_regs} | {t_ours*1e3:.3f} | {t_lib*1e3:.3f} | "
                     f"{gflop/t_ours/1e3:.0f} | {gflop/t_lib/1e3:.0f} | "
                     f"{t_lib/t_ours:.2f}x |")
        print(lines[-1], flush=True)

    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
