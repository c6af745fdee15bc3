#!/usr/bin/env python3
"""Times the stage-2 contrastive loss (forward + backward) and a whole stage-2 training step on two paths: the fused
gfx950 kernel (c2m_amd.ops.contras_loss) and a per-sample torch restatement of the reference's loss written below.

    python scripts/bench_contras.py [--steps 20] [--warmup 5] [--batch 8] [--size 160] [--pairs synthetic|generated]

--pairs generated: the batch of the training step comes from mmsr.data.contras_pairs.ContrasPairGenerator (smooth random
uint8 images, drawn homographies) instead of random tensors with synthetic coordinates, and the generator is timed next
to the stock-torch composition it replaces (torch_pairs below).

Prints one JSON line per measurement (milliseconds, median over --steps after --warmup)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "c2-matching_amd"))


def torch_loss(f1, f2, coords, teacher, margin=1.0, radius=4, steps=2, tau=0.15, wd=15.0):
    """The reference's per-sample algebra in stock torch ops (fp32), one sample at a time."""
    B, C, h1, w1 = f1.shape
    dev = f1.device
    gy, gx = torch.meshgrid(torch.arange(h1, device=dev), torch.arange(w1, device=dev), indexing="ij")
    grid = torch.stack([gy.reshape(-1), gx.reshape(-1)], 0).float()
    loss = torch.zeros(1, device=dev)
    pos_s = neg_s = kl_s = 0.
    nv = 0
    for b in range(B):
        t = coords[b, ::4, ::4, :2].reshape(-1, 2)
        x, y = t[:, 0], t[:, 1]
        ok = (x > 10) & (x < 4 * w1 - 10) & (y > 10) & (y < 4 * h1 - 10)
        ids = ok.nonzero()[:, 0]
        if ids.numel() < 128:
            continue
        p2 = torch.round(torch.stack([y[ids], x[ids]], 0) / 2 ** steps).long()
        D1 = F.normalize(f1[b].reshape(C, -1), dim=0)
        d1 = D1[:, ids]
        d2 = F.normalize(f2[b][:, p2[0], p2[1]], dim=0)
        pos = 2 - 2 * (d1 * d2).sum(0)
        out2 = (p2.unsqueeze(2).float() - p2.unsqueeze(1)).abs().max(0)[0] > radius
        neg2 = (2 - 2 * d1.t() @ d2 + (1 - out2.float()) * 10.).min(1)[0]
        out1 = (grid[:, ids].unsqueeze(2) - grid.unsqueeze(1)).abs().max(0)[0] > radius
        neg1 = (2 - 2 * d2.t() @ D1 + (1 - out1.float()) * 10.).min(1)[0]
        negm = torch.min(neg1, neg2)
        T1 = F.normalize(teacher[0][b].reshape(C, -1), dim=0)[:, ids]
        T2 = F.normalize(teacher[1][b][:, p2[0], p2[1]], dim=0)
        kl = F.kl_div(F.log_softmax(d1.t() @ d2 / tau, 1), F.softmax(T1.t() @ T2 / tau, 1), reduction="batchmean")
        loss = loss + F.relu(margin + pos - negm).mean() + wd * kl
        pos_s, neg_s, kl_s, nv = pos_s + pos.mean(), neg_s + negm.mean(), kl_s + kl, nv + 1
    return loss / nv, pos_s / nv, neg_s / nv, kl_s / nv


def coords_for(B, h, w, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(4 * h, dtype=torch.float32), torch.arange(4 * w, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(B):
        a, s, tx, ty = (torch.rand(4, generator=g) - 0.5) * torch.tensor([0.3, 0.2, 12.0, 12.0])
        cx, cy = 2.0 * w, 2.0 * h
        c, sn = torch.cos(a), torch.sin(a)
        x = (1 + s) * (c * (xx - cx) - sn * (yy - cy)) + cx + tx
        y = (1 + s) * (sn * (xx - cx) + c * (yy - cy)) + cy + ty
        out.append(torch.stack([x, y], -1))
    return torch.stack(out).to(dev)


def smooth_images(B, size, dev, seed=2):
    """uint8 [B,3,size,size]: low-frequency random images (random 10x10 fields, bicubic x16)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(size // 16, 2), max(size // 16, 2), generator=g)
    img = F.interpolate(low, size=(size, size), mode="bicubic", align_corners=False).clamp(0, 1)
    return (img * 255).to(torch.uint8).to(dev)


def torch_pairs(img_u8, matrices, scale=4):
    """What ContrasPairGenerator replaces, composed from stock torch ops on the device: the float64 coordinate grid, a
    grid_sample warp (bilinear, zero padding) and mmsr.data.pil_bicubic.pil_bicubic_resize for the four resizes."""
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    B, _, H, W = img_u8.shape
    dev = img_u8.device
    M = torch.as_tensor(matrices, dtype=torch.float64).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                            indexing="ij")
    grid = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, -1, 3)
    tc = grid @ M.transpose(1, 2)
    coords = (tc / tc[..., 2:3]).reshape(B, H, W, 3)
    sp = grid @ torch.linalg.inv(M).transpose(1, 2)
    sp = sp[..., :2] / sp[..., 2:3]
    norm = (sp + 0.5) / torch.tensor([W, H], dtype=torch.float64, device=dev) * 2 - 1
    img = img_u8.float() / 255
    ref = F.grid_sample(img, norm.float().reshape(B, H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=False)
    both = torch.cat([img_u8, (ref * 255).to(torch.uint8)])
    lq = pil_bicubic_resize(both, H // scale, W // scale)
    up = pil_bicubic_resize(lq, H, W).float() / 255
    lq = lq.float() / 255
    return {"img_in": img, "img_in_lq": lq[:B], "img_in_up": up[:B], "img_ref": ref, "img_ref_lq": lq[B:],
            "img_ref_up": up[B:], "transformed_coordinate": coords}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--pairs", choices=("synthetic", "generated"), default="synthetic")
    a = ap.parse_args()
    from c2m_amd import ops
    import mmsr.models as models
    dev = torch.device("cuda:0")
    B, h = a.batch, a.size // 4
    torch.manual_seed(0)
    f1 = torch.randn(B, 256, h, h, device=dev)
    f2 = torch.randn(B, 256, h, h, device=dev)
    t1, t2 = f1 + 0.7 * torch.randn_like(f1), f2 + 0.7 * torch.randn_like(f2)
    coords = coords_for(B, h, h, dev)
    n = ops.contras_correspondences(coords, h, h)["counts"]

    def run(fn):
        def step():
            x1, x2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
            out = fn(x1, x2)
            out[0].backward()
        return step

    fused = run(lambda x1, x2: ops.contras_loss(x1, x2, coords, teacher=(t1, t2)))
    ref = run(lambda x1, x2: torch_loss(x1, x2, coords, (t1, t2)))
    lf, lr = ops.contras_loss(f1, f2, coords, teacher=(t1, t2))[0].item(), torch_loss(f1, f2, coords, (t1, t2))[0].item()
    for name, fn in (("fused", fused), ("torch", ref)):
        print(json.dumps({"what": "loss_fwd_bwd", "path": name, "B": B, "C": 256, "map": [h, h], "rows_per_sample": n,
                          "ms": round(timed(fn, a.steps, a.warmup), 3)}))
    print(json.dumps({"what": "loss_value", "fused": lf, "torch": lr}))

    opt = {"model_type": "StudentContrasDistillationModel", "gpu_ids": [0], "is_train": True, "dist": False,
           "path": {"strict_load": True}, "network_student": {"type": "ContrasExtractorSep"},
           "network_teacher": {"type": "ContrasExtractorSep"},
           "train": {"lr_g": 1e-4, "margin": 1.0, "safe_radius": 4, "scaling_steps": 2, "temperature": 0.15,
                     "distill_weight": 15}}
    model = models.create_model(opt)
    if a.pairs == "generated":
        import numpy as np
        from mmsr.data.contras_pairs import ContrasPairGenerator, sample_pair_homography
        imgs = smooth_images(B, a.size, dev)
        gen = ContrasPairGenerator(seed=0)
        rs = np.random.RandomState(0)
        mats = np.stack([sample_pair_homography(rs, (a.size, a.size))[1] for _ in range(B)])
        for name, fn in (("generator", lambda: gen(imgs)), ("torch", lambda: torch_pairs(imgs, mats))):
            print(json.dumps({"what": "pair_generation", "path": name, "B": B, "crop": a.size,
                              "ms": round(timed(fn, a.steps, a.warmup), 3)}))
        batch = gen(imgs)
        print(json.dumps({"what": "generated_batch", "rows_per_sample":
                          ops.contras_correspondences(batch["transformed_coordinate"], h, h)["counts"]}))
        model.feed_data(batch)
    else:
        img = torch.rand(B, 3, a.size, a.size)
        model.feed_data({"img_in": img, "img_in_up": img, "img_ref": torch.rand(B, 3, a.size, a.size),
                         "transformed_coordinate": coords.cpu()})
    fused_loss = model.loss_function
    for name in ("fused", "torch"):
        if name == "torch":
            model.loss_function = lambda: torch_loss(
                model.output["dense_features1"], model.output["dense_features2"], model.transformed_coordinates,
                (model.teacher_feat["dense_features1"], model.teacher_feat["dense_features2"]))
        else:
            model.loss_function = fused_loss
        ms = timed(lambda: model.optimize_parameters(0), a.steps, a.warmup)
        print(json.dumps({"what": "stage2_train_step", "path": name, "pairs": a.pairs, "B": B, "crop": a.size, "ms": round(ms, 3)}))


if __name__ == "__main__":
    main()
