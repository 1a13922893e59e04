#!/usr/bin/env python3
"""Input pipeline microbenchmark: today's eager composition against the
device-side pipeline, for the same (source, target, target_aug) batch.

(a) eager (the engine's --gpu_augment path, plus the layout conversion the
    NHWC model needs): pinned fp32 NCHW host tensors of the cropped,
    normalized source and target -> .to(device) -> .to(bf16) ->
    gpu_target_views -> cat -> .contiguous(channels_last).  The host-side
    crop / ToTensor / Normalize / cat that produce those tensors are NOT
    timed — (a) is charged only for what the GPU and the link do.
(b) device pipeline: pinned uint8 HWC frames -> DeviceBatcher.train_batch
    (staging copy, host draw of the view table, one kernel).

Transfer and device work are timed separately with device events, (a) and
(b) alternating round by round in one process.  The kernel's achieved
bandwidth counts the frames read once and the output written once, and is
put beside add_relu (2 reads + 1 write, bf16) at the same byte count.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timed(fn, iters):
    """Device-event time per call in ms, after one untimed call."""
    fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512, help="frames per domain")
    ap.add_argument("--frame", type=int, default=256)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5,
                    help="calls per timed window of the transfers; the "
                         "shorter device and kernel rows take 10x / 40x as "
                         "many, so every window is tens of milliseconds")
    ap.add_argument("--out", default="", help="write a markdown report here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")

    from dwt_amd.data import augment
    from dwt_amd.data.device_pipeline import (IMAGENET_MEAN, IMAGENET_STD,
                                              DeviceBatcher, _upload_tables,
                                              assemble_views_reference,
                                              draw_view_params)
    from dwt_amd.kernels import dispatch
    ext = dispatch.ext()

    b, fr, cr = args.batch, args.frame, args.crop
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(0)

    # ---- inputs -----------------------------------------------------------
    src_u8 = torch.randint(0, 256, (b, fr, fr, 3), dtype=torch.uint8,
                           generator=g).pin_memory()
    tgt_u8 = torch.randint(0, 256, (b, fr, fr, 3), dtype=torch.uint8,
                           generator=g).pin_memory()
    block = torch.randn(min(b, 32), 3, cr, cr, generator=g)
    pair_f32 = block.repeat((2 * b + block.shape[0] - 1) // block.shape[0],
                            1, 1, 1)[:2 * b].contiguous().pin_memory()

    # ---- (a) eager ----------------------------------------------------------
    state = {}

    def a_transfer():
        state["pair"] = pair_f32.to(dev, non_blocking=True)

    def a_device():
        pair = state["pair"].to(dtype)
        data = torch.cat((pair, augment.gpu_target_views(pair[b:])), dim=0)
        state["a_out"] = data.contiguous(memory_format=torch.channels_last)

    def a_total():
        a_transfer()
        a_device()

    # ---- (b) device pipeline ------------------------------------------------
    batcher = DeviceBatcher(cr, IMAGENET_MEAN, IMAGENET_STD, dtype, dev, seed=0)

    def b_transfer():
        state["frames"] = batcher._stage(src_u8, tgt_u8)

    def b_device():
        # what train_batch does after staging: draw, upload the table, launch
        hw = (fr, fr)
        views = [batcher._draw(b, hw, False), batcher._draw(b, hw, False),
                 batcher._draw(b, hw, True)]
        rows = torch.arange(b, 2 * b)
        state["b_out"] = batcher._assemble(
            state["frames"], torch.cat((torch.arange(b), rows, rows)), views)

    def b_total():
        state["b_out"] = batcher.train_batch(src_u8, tgt_u8)

    # ---- kernels alone ------------------------------------------------------
    b_transfer()
    gen = torch.Generator().manual_seed(1)
    plain = draw_view_params(2 * b, (fr, fr), cr, generator=gen, aug=False)
    dup = draw_view_params(b, (fr, fr), cr, generator=gen, aug=True)
    rows = torch.arange(b, 2 * b)
    table = dict(
        src_index=torch.cat((torch.arange(2 * b), rows)),
        top=torch.cat((plain.top, dup.top)),
        left=torch.cat((plain.left, dup.left)),
        flip=torch.cat((plain.flip, dup.flip)),
        inv_affine=torch.cat((plain.inv_affine, dup.inv_affine)),
        affine=torch.cat((plain.affine, dup.affine)))
    d_tab = _upload_tables(table["src_index"], table["top"], table["left"],
                           table["flip"], table["inv_affine"], table["affine"],
                           dev)
    k_out = torch.empty((3 * b, 3, cr, cr), dtype=dtype, device=dev,
                        memory_format=torch.channels_last)
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)

    def kernel():
        ext.assemble_views(state["frames"], *d_tab, k_out, mean, std)

    # the same launch with every row plain / every row flipped + affine: how
    # the kernel's time splits between its two kinds of row
    d_plain = _upload_tables(table["src_index"], table["top"], table["left"],
                             torch.zeros(3 * b, dtype=torch.bool),
                             table["inv_affine"],
                             torch.zeros(3 * b, dtype=torch.bool), dev)
    d_affine = _upload_tables(table["src_index"], table["top"], table["left"],
                              dup.flip.repeat(3), dup.inv_affine.repeat(3, 1),
                              torch.ones(3 * b, dtype=torch.bool), dev)

    def kernel_plain():
        ext.assemble_views(state["frames"], *d_plain, k_out, mean, std)

    def kernel_affine():
        ext.assemble_views(state["frames"], *d_affine, k_out, mean, std)

    kernel_bytes = 2 * b * fr * fr * 3 + k_out.numel() * 2
    n_ar = kernel_bytes // 6            # bf16: two reads + one write
    n_ar -= n_ar % 8
    ar_a = torch.randn(n_ar, device=dev, dtype=dtype)
    ar_b = torch.randn(n_ar, device=dev, dtype=dtype)
    ar_out = torch.empty_like(ar_a)

    def add_relu():
        ext.add_relu_fwd(ar_a, ar_b, ar_out)

    # ---- correctness at the timed size (a few rows of every stream) --------
    kernel()
    pick = [0, b - 1, b, 2 * b - 1, 2 * b, 3 * b - 1]
    ref = assemble_views_reference(
        state["frames"].cpu(), crop=cr, mean=mean, std=std, dtype=torch.float32,
        **{k: v[pick] for k, v in table.items()})
    got = k_out[pick].float().cpu()
    excess = ((got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-4)).max().item()
    # a random matrix may put a coordinate within rounding of the frame edge;
    # report rather than assert, the bound is asserted by the test suite
    print(f"check vs reference on rows {pick}: max(err - bf16 bound) = {excess:.3e}")

    # ---- timing: alternate everything round by round -----------------------
    names = ["a_transfer", "a_device", "a_total", "b_transfer", "b_device",
             "b_total", "kernel", "kernel_plain", "kernel_affine", "add_relu"]
    fns = dict(a_transfer=a_transfer, a_device=a_device, a_total=a_total,
               b_transfer=b_transfer, b_device=b_device, b_total=b_total,
               kernel=kernel, kernel_plain=kernel_plain,
               kernel_affine=kernel_affine, add_relu=add_relu)
    a_transfer()
    samples = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            mult = 40 if n.startswith("kernel") or n == "add_relu" else \
                10 if n.endswith("_device") else 1
            samples[n].append(timed(fns[n], args.iters * mult))

    res = {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
           for n, v in samples.items()}
    a_bytes = pair_f32.numel() * 4
    b_bytes = src_u8.numel() + tgt_u8.numel()
    ar_bytes = n_ar * 6
    res["a_transfer"]["GBps"] = a_bytes / res["a_transfer"]["median_ms"] / 1e6
    res["b_transfer"]["GBps"] = b_bytes / res["b_transfer"]["median_ms"] / 1e6
    for k in ("kernel", "kernel_plain", "kernel_affine"):
        res[k]["TBps"] = kernel_bytes / res[k]["median_ms"] / 1e9
    res["add_relu"]["TBps"] = ar_bytes / res["add_relu"]["median_ms"] / 1e9
    summary = dict(batch_per_domain=b, frame=fr, crop=cr, dtype="bfloat16",
                   rounds=args.rounds, iters=args.iters,
                   a_transfer_bytes=a_bytes, b_transfer_bytes=b_bytes,
                   kernel_bytes=kernel_bytes, add_relu_bytes=ar_bytes,
                   check_excess=excess, device=torch.cuda.get_device_name(0),
                   results=res)
    print(json.dumps(summary))

    if args.out:
        label = {
            "a_transfer": f"(a) transfer: fp32 NCHW pair, {a_bytes / 1e6:.0f} MB",
            "a_device": "(a) device: cast, gpu_target_views, cat, to NHWC",
            "a_total": "(a) transfer + device",
            "b_transfer": f"(b) transfer: uint8 frames, {b_bytes / 1e6:.0f} MB",
            "b_device": "(b) device: draw, table upload, assemble_views",
            "b_total": "(b) DeviceBatcher.train_batch",
            "kernel": f"assemble_views kernel alone, {kernel_bytes / 1e6:.0f} MB",
            "kernel_plain": "the same launch, all 3B rows plain",
            "kernel_affine": "the same launch, all 3B rows flip + affine",
            "add_relu": f"add_relu_fwd kernel alone, {ar_bytes / 1e6:.0f} MB",
        }
        lines = ["| what | median ms | min | max | rate |", "|---|---|---|---|---|"]
        for n in names:
            r = res[n]
            rate = (f"{r['GBps']:.1f} GB/s" if "GBps" in r else
                    f"{r['TBps']:.2f} TB/s" if "TBps" in r else "")
            lines.append(f"| {label[n]} | {r['median_ms']:.3f} | "
                         f"{r['min_ms']:.3f} | {r['max_ms']:.3f} | {rate} |")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
