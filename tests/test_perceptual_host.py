"""CPU: mmsr.models.losses.PerceptualLoss in float32 against the reference's class run in float64 (tests/golden/
make_golden_perceptual.py: seeded VGG19 weights and images, only loss values and dL/dx are stored).

Bars: values to 1e-5 relative; gradients to 2e-5 of max |grad| -- four times the gap between stock float32 and float64 autograd
measured on this tower with these weights (2.9e-6 .. 5.2e-6 for 'fro', 4.8e-7 .. 6.1e-7 for 'l1')."""
import numpy as np
import pytest
import torch

import make_golden_perceptual as mgp


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/perceptual_golden.npz")


def _loss(case):
    from mmsr.models.losses import PerceptualLoss
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # random VGG weights: overwritten with the seeded ones
        loss = PerceptualLoss(**mgp.CASES[case][0])
    mgp.fill_vgg(loss.vgg.vgg_net)
    return loss


@pytest.mark.parametrize("case", sorted(mgp.CASES))
def test_perceptual_loss_matches_the_reference_in_float64(gold, case):
    loss = _loss(case)
    x, gt = (torch.from_numpy(a) for a in mgp.images(case))
    x.requires_grad_(True)
    percep, style = loss(x, gt)
    total = 0
    for name, got in (("percep", percep), ("style", style)):
        want = float(gold[f"{case}.{name}"])
        if np.isnan(want):
            assert got is None, name
            continue
        print(case, name, got.item(), want)
        assert abs(got.item() - want) <= 1e-5 * abs(want), (name, got.item(), want)
        total = total + got
    total.backward()
    want = gold[f"{case}.grad"]
    e = float(np.abs(x.grad.double().numpy() - want).max() / np.abs(want).max())
    print(case, "grad e", e)
    assert e <= 2e-5, e
    assert all(not p.requires_grad for p in loss.parameters())


@pytest.mark.parametrize("criterion", ["fro", "l1", "l2"])
def test_loss_of_an_image_against_itself_is_zero_with_a_zero_gradient(criterion):
    from mmsr.models.losses import PerceptualLoss
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        loss = PerceptualLoss({"relu2_1": 1.0, "relu3_1": 0.5}, criterion=criterion, norm_img=False)
    mgp.fill_vgg(loss.vgg.vgg_net)
    x = torch.from_numpy(mgp.images("fro_relu5_1", (1, 3, 16, 16))[0]).requires_grad_(True)
    percep, style = loss(x, x.detach().clone())
    assert style is None and float(percep) == 0.0
    percep.backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) == 0.0


def test_l2_constructs_and_an_unknown_criterion_raises():
    from mmsr.models.losses import PerceptualLoss
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert isinstance(PerceptualLoss({"relu1_1": 1.0}, criterion="l2").criterion, torch.nn.MSELoss)
        with pytest.raises(NotImplementedError):
            PerceptualLoss({"relu1_1": 1.0}, criterion="charbonnier")
        with pytest.raises(ValueError):     # no criterion module for a style term
            PerceptualLoss({"relu1_1": 1.0}, criterion="fro", style_weight=1.0)
