#!/usr/bin/env python3
"""Times the metrics of one validation batch on two paths, in one process, alternating:

  fused        c2m_amd.ops.val_metrics (csrc/val_metrics.hip: one pass over SR and GT, two launches), without and with the
               uint8 images a save_img run asks for;
  composition  mmsr.utils.metrics.validation_metrics: stock torch ops and five float64 11 x 11 F.conv2d calls.

    python scripts/bench_val_metrics.py [--sizes 1x640x640 16x640x640 1x500x332] [--calls 400] [--rounds 7] [--warmup 10]

A measurement is the host clock around a block of back-to-back calls ending in a device synchronise, divided by the calls
(neither path waits for the device inside a call); a block is sized to last about half a second, `--calls` at the most.
`--rounds` such blocks per path, A B C A B C ...; printed per size and path: the median, the fastest and the slowest block
(the run's own spread).  Every shape is warmed up first.  One JSON line per (size, path) and one verdict per size; both
paths' numbers are compared first, to the bounds of tests/test_val_metrics_gpu.py."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "c2-matching_amd"))


def block_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1x640x640", "16x640x640", "1x500x332"], help="BxHxW")
    ap.add_argument("--crop", type=int, default=4)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_val_metrics.py measures on the GPU; none is visible")
    from c2m_amd import ops
    from mmsr.utils import metrics
    dev = torch.device("cuda:0")
    slower = []
    for size in a.sizes:
        B, H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(0)
        gt = torch.rand(B, 3, H, W, generator=g).to(dev)
        sr = (gt + 0.05 * torch.randn(B, 3, H, W, generator=g).to(dev)).contiguous()
        paths = (("fused", lambda: ops.val_metrics(sr, gt, crop_border=a.crop)),
                 ("fused_images", lambda: ops.val_metrics(sr, gt, crop_border=a.crop, images="rgb")),
                 ("composition", lambda: metrics.validation_metrics(sr, gt, crop_border=a.crop)))
        # agreement first.  torch divides a CUDA tensor by a Python scalar through the fp32 reciprocal, which is not the CPU's
        # (the reference's) `s / 255.0`; the composition is compared under metrics.true_scalar_division, as the model runs it
        # (DESIGN.md section 14).  The timed composition is the plain function: the context adds a few 0-dim fills.
        f = paths[0][1]()
        with metrics.true_scalar_division():
            c = paths[2][1]()
        diff = {k: float((f[k] - c[k]).abs().max()) for k in ("psnr", "psnr_y", "ssim_y")}
        calls = {}
        for name, fn in paths:
            block_ms(fn, a.warmup)
            # a block lasts about half a second, with at most --calls and at least 3 calls
            calls[name] = int(min(a.calls, max(3, round(500.0 / max(block_ms(fn, 3), 1e-3)))))
        ms = {name: [] for name, _ in paths}
        for _ in range(a.rounds):
            for name, fn in paths:
                ms[name].append(block_ms(fn, calls[name]))
        med = {}
        for name, _ in paths:
            t = sorted(ms[name])
            med[name] = t[len(t) // 2]
            print(json.dumps({"what": "val_metrics", "path": name, "B": B, "H": H, "W": W, "crop": a.crop, "calls_per_block": calls[name],
                              "ms_median": round(med[name], 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}), flush=True)
        spread = max(max(v) - min(v) for v in ms.values())
        worse = bool(med["fused"] - med["composition"] > 0)
        if worse:
            slower.append(size)
        print(json.dumps({"what": "verdict", "device": torch.cuda.get_device_name(0), "size": size, "max_abs_diff": diff,
                          "fused_over_composition": round(med["fused"] / med["composition"], 4),
                          "fused_images_over_composition": round(med["fused_images"] / med["composition"], 4),
                          "spread_ms": round(spread, 4), "fused_slower": worse}), flush=True)
        if diff["psnr"] > 1e-9 or diff["psnr_y"] > 1e-8 or diff["ssim_y"] > 1e-9:
            raise SystemExit(f"the two paths disagree at {size}: {diff}")
    print(json.dumps({"what": "summary", "fused_slower_at": slower}))


if __name__ == "__main__":
    main()
