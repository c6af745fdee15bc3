#!/usr/bin/env python3
"""Times the stage-3 GAN additions on the GPU, both sides of every comparison alternated in one process:

  penalty   the WGAN-GP penalty on a gradient of [B, 3, GT, GT], forward + backward, eager:
              fused        c2m_amd.ops.gradient_penalty (csrc/gp_penalty.hip: two launches forward, one backward)
              composition  ((g.flatten(1).norm(2, dim=1) - 1) ** 2).mean() on torch's operators
  step      RefRestorationModel at the geometry of options/train/stage3_restoration_gan.yml (GT 160, batch 4, ndf 32,
            relu5_1 'fro' perceptual loss, wgan + gradient penalty), eager:
              gan_fused / gan_composition   a whole GAN-phase step with GradientPenaltyLoss.fused on / off
              pretrain                      a pretrain-phase step (pixel loss only), for scale
  parts     where the critic's side of a GAN-phase step goes: the critic's step with and without the penalty, the penalty's
            forward (D(x^), autograd.grad(create_graph=True), the penalty) and its forward + backward -- the difference of the
            last two is the critic's double backward

    python scripts/bench_gan_step.py [--gt 160] [--batch 4] [--ndf 32] [--rounds 7] [--warmup 5] [--only penalty step parts]
    python scripts/bench_gan_step.py --trace fused|composition [--calls 20]

A measurement is the host clock around a block of back-to-back calls ending in a device synchronise, divided by the calls; a
block is sized to last about half a second.  `--rounds` such blocks per path, A B C A B C ...; printed per path: the median,
the fastest and the slowest block (the run's own spread).  Every path is warmed up first.  One JSON line per path and one
verdict per comparison.  `--trace` only runs `--calls` penalty forward + backward pairs of one path after a warm-up pair and
prints a marker line: the command to put behind `rocprofv3 --kernel-trace --stats --` for the launch counts."""
import argparse
import json
import os
import sys
import time
import warnings

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


def alternate(what, paths, rounds, warmup, max_calls=400, **extra):
    """paths: [(name, fn)] -> {name: median ms}; prints one JSON line per path."""
    calls = {}
    for name, fn in paths:
        block_ms(fn, warmup)
        calls[name] = int(min(max_calls, max(3, round(500.0 / max(block_ms(fn, 3), 1e-3)))))
    ms = {name: [] for name, _ in paths}
    for _ in range(rounds):
        for name, fn in paths:
            ms[name].append(block_ms(fn, calls[name]))
    med = {}
    for name, _ in paths:
        t = sorted(ms[name])
        med[name] = t[len(t) // 2]
        print(json.dumps(dict(extra, what=what, path=name, calls_per_block=calls[name], ms_median=round(med[name], 4),
                              ms_min=round(t[0], 4), ms_max=round(t[-1], 4))), flush=True)
    return med, {name: max(v) - min(v) for name, v in ms.items()}


def composition(g):
    return ((g.flatten(1).norm(2, dim=1) - 1) ** 2).mean()


def penalty_paths(a, dev):
    from c2m_amd import ops
    gen = torch.Generator().manual_seed(0)
    g = (torch.randn(a.batch, 3, a.gt, a.gt, generator=gen) * (2.5 / (3 * a.gt * a.gt) ** 0.5)).to(dev).requires_grad_(True)

    def run(fn):
        def call():
            g.grad = None
            fn(g).backward()
        return call
    return g, (("fused", run(ops.gradient_penalty)), ("composition", run(composition)))


def build_model(a, dev):
    from mmsr.models.ref_restoration_model import RefRestorationModel
    opt = {"dist": False, "gpu_ids": [0], "is_train": True, "path": {},
           "network_g": {"type": "RestorationNet", "ngf": 64, "n_blocks": 16, "groups": 8},
           "network_d": {"type": "ImageDiscriminator", "in_nc": 3, "ndf": a.ndf},
           "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                           "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
           "network_extractor": {"type": "ContrasExtractorSep"},
           "train": {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6, "weight_decay_g": 0,
                     "beta_g": [0.9, 0.999], "lr_d": 1e-4, "weight_decay_d": 0, "beta_d": [0.9, 0.999], "pixel_weight": 1.0,
                     "perceptual_opt": {"layer_weights": {"relu5_1": 1.0}, "vgg_type": "vgg19", "use_input_norm": True,
                                        "perceptual_weight": 1e-4, "style_weight": 0, "norm_img": False, "criterion": "fro"},
                     "gan_type": "wgan", "gan_weight": 1e-6, "grad_penalty_weight": 10, "net_d_steps": 1, "net_d_init_steps": 0,
                     "net_g_pretrain_steps": 1}}
    torch.manual_seed(10)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # random VGG weights: a timing does not care
        model = RefRestorationModel(opt)
    gen = torch.Generator().manual_seed(1)
    h = a.gt // 4
    gt = torch.rand(a.batch, 3, 4 * h, 4 * h, generator=gen)
    lq = torch.nn.functional.interpolate(gt, scale_factor=0.25, mode="bicubic", align_corners=False).clamp(0, 1)
    up = torch.nn.functional.interpolate(lq, scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    model.feed_data({"img_in_lq": lq, "img_ref": torch.rand(a.batch, 3, 4 * h, 4 * h, generator=gen), "img_in": gt, "img_in_up": up})
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt", type=int, default=160)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ndf", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="+", default=["penalty", "step", "parts"], choices=["penalty", "step", "parts"])
    ap.add_argument("--trace", choices=["fused", "composition"])
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gan_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    geometry = {"batch": a.batch, "gt": a.gt}

    if a.trace:
        _, paths = penalty_paths(a, dev)
        fn = dict(paths)[a.trace]
        fn()
        torch.cuda.synchronize()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(geometry, what="trace", path=a.trace, pairs=a.calls + 1)))
        return

    if "penalty" in a.only:
        from c2m_amd import ops
        g, paths = penalty_paths(a, dev)
        # agreement first: both paths against float64 on the same tensor
        want = composition(g.detach().double())
        diff = {name: abs(float(f(g.detach())) - float(want)) / float(want) for name, f in
                (("fused", ops.gradient_penalty), ("composition", composition))}
        med, spread = alternate("penalty", paths, a.rounds, a.warmup, **geometry)
        print(json.dumps(dict(geometry, what="verdict", comparison="penalty forward + backward", device=torch.cuda.get_device_name(0),
                              rel_err_vs_float64=diff, fused_over_composition=round(med["fused"] / med["composition"], 4),
                              spread_ms={k: round(v, 4) for k, v in spread.items()},
                              fused_slower_beyond_spread=bool(med["fused"] - med["composition"] > max(spread.values())))), flush=True)
        if max(diff.values()) > 1e-5:
            raise SystemExit(f"the penalty paths disagree with float64: {diff}")

    if "step" in a.only or "parts" in a.only:
        model = build_model(a, dev)
        geometry["ndf"] = a.ndf
        cri = model.cri_grad_penalty

        def gan_step(fused):
            def call():
                cri.fused = fused
                model.optimize_parameters(2)
            return call

    if "step" in a.only:
        med, spread = alternate("step", (("gan_fused", gan_step(True)), ("gan_composition", gan_step(False)),
                                         ("pretrain", lambda: model.optimize_parameters(1))), a.rounds, a.warmup, max_calls=50,
                                **geometry)
        print(json.dumps(dict(geometry, what="verdict", comparison="GAN-phase step, penalty fused vs composition",
                              fused_over_composition=round(med["gan_fused"] / med["gan_composition"], 4),
                              gan_over_pretrain=round(med["gan_fused"] / med["pretrain"], 4),
                              spread_ms={k: round(v, 4) for k, v in spread.items()},
                              fused_slower_beyond_spread=bool(med["gan_fused"] - med["gan_composition"] >
                                                              max(spread["gan_fused"], spread["gan_composition"])))), flush=True)

    if "parts" in a.only:
        cri.fused = True
        model.optimize_parameters(2)          # leaves model.output / model.gt of a GAN-phase step
        fake = model.output.detach()

        def critic_step(with_penalty):
            def call():
                model.cri_grad_penalty = cri if with_penalty else None
                model._critic_step()
                model.cri_grad_penalty = cri
            return call

        def penalty_forward():
            cri(model.net_d, model.gt, fake)

        def penalty_both():
            model.optimizer_d.zero_grad()
            cri(model.net_d, model.gt, fake).backward()
        med, _ = alternate("parts", (("gan_step", gan_step(True)), ("critic_step", critic_step(True)),
                                     ("critic_step_no_penalty", critic_step(False)), ("penalty_forward", penalty_forward),
                                     ("penalty_forward_backward", penalty_both)), a.rounds, a.warmup, max_calls=50, **geometry)
        double_backward = med["penalty_forward_backward"] - med["penalty_forward"]
        print(json.dumps(dict(geometry, what="verdict", comparison="shares of a GAN-phase step",
                              critic_step_share=round(med["critic_step"] / med["gan_step"], 4),
                              penalty_share=round((med["critic_step"] - med["critic_step_no_penalty"]) / med["gan_step"], 4),
                              double_backward_ms=round(double_backward, 4),
                              double_backward_share=round(double_backward / med["gan_step"], 4))), flush=True)


if __name__ == "__main__":
    main()
