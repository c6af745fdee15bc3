#!/usr/bin/env python3
"""Generates tests/golden/perceptual_golden.npz by running the REFERENCE's ``PerceptualLoss`` (mmsr/models/losses.py) on the
CPU in float64, on deterministic inputs and seeded VGG weights.

Runs only where the reference checkout exists.  Nothing of the reference is copied: its module is imported by path, with
make_golden.stub_third_party() standing in for the packages that are not installed (torchvision's VGG layer layout among
them).  Neither images nor weights are stored: the tests rebuild them from synth.py seeds with the functions below; the
fixture holds the loss values and dL/dx (L = perceptual + style, whichever are not None) of every case.

    python tests/golden/make_golden_perceptual.py
"""
import functools
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

# name -> (PerceptualLoss arguments, image range); every case B = 2 at 32 x 32
CASES = {
    "fro_relu5_1": (dict(layer_weights={"relu5_1": 1.0}, criterion="fro", norm_img=False), (0.0, 1.0)),   # the GAN yaml
    "l1_two_taps_norm_img": (dict(layer_weights={"relu2_1": 0.5, "relu4_1": 1.0}, criterion="l1", norm_img=True), (-1.0, 1.0)),
    "l1_style": (dict(layer_weights={"relu1_1": 1.0, "relu2_1": 1.0}, criterion="l1", norm_img=False, style_weight=1.0), (0.0, 1.0)),
}
SHAPE = (2, 3, 32, 32)


def images(case, shape=SHAPE):
    """(x, gt) float32 arrays of the case's range."""
    lo, hi = CASES[case][1]
    seed = 9200 + 10 * sorted(CASES).index(case)
    return synth.uniform(shape, seed, lo, hi), synth.uniform(shape, seed + 1, lo, hi)


@functools.lru_cache(maxsize=None)
def conv_parameters(k, cout, cin):
    """Seeded weight / bias of the k-th convolution of the stack: He-scaled weights (features stay O(1), about half positive),
    small biases."""
    w = synth.gaussish((cout, cin, 3, 3), 9000 + k) * np.float32(np.sqrt(2.0 / (9 * cin)))
    return w.astype(np.float32), synth.uniform((cout,), 9100 + k, -0.05, 0.05)


def fill_vgg(stack):
    """Overwrite the convolutions of an nn.Sequential / ordered dict VGG stack with the seeded parameters (any dtype / device)."""
    layers = stack._modules.values() if hasattr(stack, "_modules") else stack.values()
    k = 0
    with torch.no_grad():
        for m in layers:
            if isinstance(m, torch.nn.Conv2d):
                w, b = conv_parameters(k, m.out_channels, m.in_channels)
                m.weight.copy_(torch.from_numpy(w))
                m.bias.copy_(torch.from_numpy(b))
                k += 1


def load_reference_losses():
    import make_golden
    ref = make_golden.REF
    sys.path.insert(0, ref)
    make_golden.stub_third_party()
    spec = importlib.util.spec_from_file_location("mmsr.models.losses", f"{ref}/mmsr/models/losses.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = load_reference_losses()
    out = {}
    for case, (kw, _) in CASES.items():
        loss = ref.PerceptualLoss(**kw)
        fill_vgg(loss.vgg.vgg_net)
        loss = loss.double()
        x, gt = (torch.from_numpy(a).double() for a in images(case))
        x.requires_grad_(True)
        percep, style = loss(x, gt)
        total = sum(t for t in (percep, style) if t is not None)
        total.backward()
        out[f"{case}.percep"] = np.float64(percep.item() if percep is not None else np.nan)
        out[f"{case}.style"] = np.float64(style.item() if style is not None else np.nan)
        out[f"{case}.grad"] = x.grad.numpy()
        print(case, out[f"{case}.percep"], out[f"{case}.style"], float(np.abs(out[f"{case}.grad"]).max()))
    np.savez_compressed(os.path.join(HERE, "perceptual_golden.npz"), **out)


if __name__ == "__main__":
    main()
