#!/usr/bin/env python3
"""Times the making of one stage-3 training batch from uint8 images on two paths, in one process, alternating:

  generator    mmsr.data.ref_pairs.RefPairGenerator (c2m_amd.ops.pil_bicubic_resize2d_u8: both resampling passes in one
               launch, flips / transpose on read);
  composition  the same steps from the two-pass operator (ops.pil_bicubic_resize_u8), torch flips sample by sample and the
               identity-table pass for the uint8 -> float32 / 255 images (`composed` below).

    python scripts/bench_ref_pairs.py [--batch 9] [--size 160] [--ref-size 200 140] [--calls 200] [--rounds 7] [--warmup 20]

The work is launch-bound, so a measurement is the host clock around `--calls` back-to-back batches ending in a device
synchronise, divided by the calls.  `--rounds` such blocks per path, A B A B ...; printed per path: the median, the
fastest and the slowest block (the run's own spread) and what one batch launches: kernels of this project's library
(counted at the C entry points) and torch operators that do work on the device (each at least one kernel or copy).
One JSON line per path and one with the verdict; both paths' batches are compared for equality first."""
import argparse
import json
import os
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "c2-matching_amd"))

KEYS = ("img_in", "img_in_lq", "img_in_up", "img_ref", "img_ref_lq", "img_ref_up")
# aten operators that only allocate or re-describe memory
NO_WORK = ("empty", "view", "reshape", "slice", "select", "transpose", "as_strided", "alias", "detach", "expand", "permute",
           "unsqueeze", "squeeze", "t", "_unsafe_view", "unbind", "split", "lift_fresh", "_reshape_alias", "narrow")


def composed(img_in, refs, flags, gt, scale):
    """RefPairGenerator's train phase from the two-pass operator and torch ops."""
    from c2m_amd import ops
    B = img_in.shape[0]
    refs = torch.stack([r if tuple(r.shape[-2:]) == (gt, gt) else ops.pil_bicubic_resize_u8(r, gt, gt) for r in refs])
    both = ops._orient_torch(torch.cat([img_in, refs]), flags + flags)
    lq_u8, lq = ops.pil_bicubic_resize_u8(both, gt // scale, gt // scale, as_float=True)
    _, up = ops.pil_bicubic_resize_u8(lq_u8, gt, gt, as_float=True)
    _, full = ops.pil_bicubic_resize_u8(both, gt, gt, as_float=True)
    return {"img_in": full[:B], "img_in_lq": lq[:B], "img_in_up": up[:B], "img_ref": full[B:], "img_ref_lq": lq[B:],
            "img_ref_up": up[B:]}


class _DeviceOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__
        outs = out if isinstance(out, (tuple, list)) else (out,)
        if name not in NO_WORK and not name.startswith("empty") and any(isinstance(o, torch.Tensor) and o.is_cuda for o in outs):
            self.names.append(name)
        return out


def count_launches(fn):
    """-> (launches of the library's resampling kernels, torch operators with device work) of one call of fn."""
    from c2m_amd import _lib
    L = _lib.lib()
    calls = {"c2m_pil_bicubic_u8": 0, "c2m_pil_bicubic2d_u8": 0}
    real = {k: getattr(L, k) for k in calls}

    def counting(k):
        def f(*a):
            calls[k] += 1
            return real[k](*a)
        return f
    for k in calls:
        setattr(L, k, counting(k))
    try:
        with _DeviceOps() as mode:
            fn()
    finally:
        for k in calls:
            setattr(L, k, real[k])
    return calls, sorted(mode.names)


def block_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=9)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--ref-size", type=int, nargs=2, default=(200, 140))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from mmsr.data.ref_pairs import RefPairGenerator, draw_flags
    import random
    if not torch.cuda.is_available():
        raise SystemExit("bench_ref_pairs.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img_in = torch.randint(0, 256, (a.batch, 3, a.size, a.size), generator=g, dtype=torch.uint8).to(dev)
    refs = [torch.randint(0, 256, (3, *a.ref_size), generator=g, dtype=torch.uint8).to(dev) for _ in range(a.batch)]
    gen = RefPairGenerator(phase="train", gt_size=a.size, scale=a.scale, seed=0)
    flags = draw_flags(random.Random(0), a.batch)

    def run_gen():
        gen.flip_rng.seed(0)               # the same draws every call: both paths make the same batch
        return gen(img_in, refs)

    def run_composed():
        return composed(img_in, refs, list(flags), a.size, a.scale)

    d, c = run_gen(), run_composed()
    same = all(torch.equal(d[k], c[k]) for k in KEYS)
    paths = (("generator", run_gen), ("composition", run_composed))
    launches = {name: count_launches(fn) for name, fn in paths}
    for _, fn in paths:
        block_ms(fn, a.warmup)
    ms = {name: [] for name, _ in paths}
    for _ in range(a.rounds):
        for name, fn in paths:
            ms[name].append(block_ms(fn, a.calls))
    med = {}
    for name, _ in paths:
        t = sorted(ms[name])
        med[name] = t[len(t) // 2]
        lib, aten = launches[name]
        print(json.dumps({"what": "stage3_batch", "path": name, "B": a.batch, "gt": a.size, "ref": list(a.ref_size),
                          "ms_median": round(med[name], 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                          "library_launches": lib, "torch_device_ops": len(aten), "torch_ops": aten}))
    spread = max(max(v) - min(v) for v in ms.values())
    print(json.dumps({"what": "verdict", "device": torch.cuda.get_device_name(0), "batches_equal": same,
                      "generator_over_composition": round(med["generator"] / med["composition"], 4),
                      "spread_ms": round(spread, 4),
                      "fused_slower_beyond_spread": bool(med["generator"] - med["composition"] > spread)}))
    if not same:
        raise SystemExit("the two paths made different batches")


if __name__ == "__main__":
    main()
