#!/usr/bin/env python3
"""Generates tests/golden/gan_golden.npz by running the REFERENCE's ``GANLoss``, ``GradientPenaltyLoss`` (mmsr/models/losses.py)
and ``ImageDiscriminator`` (mmsr/models/archs/discriminator_arch.py) on the CPU in float64, on seeded inputs and weights.

Runs only where the reference checkout exists.  Nothing of the reference is copied: its modules are imported by path (this
repository's ``mmsr`` must not be importable while that happens, or the reference's relative imports would resolve to it).
Neither weights nor images are stored: the tests rebuild them from synth.py seeds with the functions below; the fixture holds

  gan.<type>.<disc|gen>.<real|fake>.value / .grad   GANLoss(type, loss_weight 0.37) on PRED and its d/d(input)
  d.keys / d.shapes / d.out                          the critic's sorted state_dict keys, their shapes, D(critic_input())
  gp.alpha / gp.value / gp.grad.<parameter>          GradientPenaltyLoss(10.0) on that critic at gp_inputs(): the alpha the
                                                     reference drew (recorded by re-seeding), the loss, d loss / d parameter
                                                     (the leading rows GP_PARAMETERS names)

    python tests/golden/make_golden_gan.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

GAN_TYPES = ("vanilla", "lsgan", "wgan", "hinge")
GAN_WEIGHT = 0.37
NDF = 4
GP_WEIGHT = 10.0
GP_SEED = 9750
# the parameters whose penalty gradients are recorded, and how many leading rows (output channels) of each (None: all; the
# large tensors are cut to keep the fixture small): first and last 3x3 convolution, one BatchNorm weight, the 1x1 head
GP_PARAMETERS = {"conv_block1.0.weight": None, "conv_block5.3.weight": 16, "conv_block3.1.weight": None,
                 "out_block.1.weight": 64, "out_block.3.weight": None}


def gan_pred():
    """The critic prediction the GANLoss cases run on: [4,1,1,1], both signs, magnitudes around 1 (both hinge branches)."""
    return synth.uniform((4, 1, 1, 1), 9700, -1.5, 1.5)


def critic_input():
    return synth.uniform((2, 3, 32, 32), 9710, 0.0, 1.0)


def gp_inputs():
    """(real, fake) of the penalty case.  64 x 64: the critic's last BatchNorm then sees a 2 x 2 map (8 values per channel);
    at 32 x 32 it would see 2 values per channel, normalise them to +-1 and pass next to no gradient to the input."""
    return synth.uniform((2, 3, 64, 64), 9720, 0.0, 1.0), synth.uniform((2, 3, 64, 64), 9721, 0.0, 1.0)


def fill_critic(net):
    """Overwrite every parameter of an ImageDiscriminator with name-keyed seeded values (any dtype / device): He-scaled
    convolution weights, small biases, BatchNorm weights around 1.  Buffers (running statistics) are left alone."""
    with torch.no_grad():
        for name, p in net.named_parameters():
            g = synth.gaussish(tuple(p.shape), synth.name_seed("critic." + name)).astype(np.float64)
            if p.dim() == 4:
                v = g * np.sqrt(2.0 / (p.shape[1] * p.shape[2] * p.shape[3]))
            elif name.endswith("weight"):
                v = 1.0 + 0.1 * g
            else:
                v = 0.05 * g
            p.copy_(torch.from_numpy(v.astype(np.float32)))


def load_reference():
    """-> (the reference's losses module, its discriminator_arch module)"""
    import make_golden_perceptual as mgp
    losses = mgp.load_reference_losses()
    import make_golden
    assert all(p.startswith(make_golden.REF) for p in sys.modules["mmsr.models"].__path__), "this repository's mmsr shadows the reference's"
    name = "mmsr.models.archs.discriminator_arch"
    spec = importlib.util.spec_from_file_location(name, f"{make_golden.REF}/mmsr/models/archs/discriminator_arch.py")
    arch = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(arch)
    return losses, arch


def main():
    losses, arch = load_reference()
    out = {}
    for gan_type in GAN_TYPES:
        cri = losses.GANLoss(gan_type, loss_weight=GAN_WEIGHT)
        for is_disc in (True, False):
            for real in (True, False):
                x = torch.from_numpy(gan_pred()).double().requires_grad_(True)
                v = cri(x, real, is_disc=is_disc)
                v.backward()
                key = f"gan.{gan_type}.{'disc' if is_disc else 'gen'}.{'real' if real else 'fake'}"
                out[key + ".value"] = np.float64(v.item())
                out[key + ".grad"] = x.grad.numpy()
                print(key, v.item())

    net = arch.ImageDiscriminator(3, ndf=NDF)
    fill_critic(net)
    net = net.double().train()
    sd = net.state_dict()
    out["d.keys"] = np.array(sorted(sd))
    out["d.shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in sorted(sd)])
    with torch.no_grad():
        out["d.out"] = net(torch.from_numpy(critic_input()).double()).numpy()
    print("d.out", out["d.out"].ravel())

    real, fake = (torch.from_numpy(a).double() for a in gp_inputs())
    net.zero_grad()
    torch.manual_seed(GP_SEED)
    loss = losses.GradientPenaltyLoss(GP_WEIGHT)(net, real, fake)
    loss.backward()
    torch.manual_seed(GP_SEED)
    out["gp.alpha"] = torch.rand(real.size(0), 1, 1, 1).double().numpy()     # what the reference's call drew
    out["gp.value"] = np.float64(loss.item())
    params = dict(net.named_parameters())
    for name, rows in GP_PARAMETERS.items():
        out["gp.grad." + name] = params[name].grad[:rows].numpy()
        print("gp.grad", name, float(np.abs(out["gp.grad." + name]).max()))
    print("gp.value", loss.item(), "alpha", out["gp.alpha"].ravel())
    np.savez_compressed(os.path.join(HERE, "gan_golden.npz"), **out)


if __name__ == "__main__":
    main()
