"""GPU tests of the stage-3 perceptual loss: PerceptualLoss on the device against the float64 fixture, and
RefRestorationModel's two-phase step, eager and captured.

Weights and images are seeded (tests/golden/make_golden_perceptual.py).  The bars of the loss are those of
tests/test_perceptual_host.py: values to 1e-5 relative, dL/dx to 2e-5 of max |grad|, four times the gap between stock float32
and float64 autograd on this tower (the device's own gap was 3.7e-6 .. 4.3e-6 for 'fro' and 5.3e-7 for 'l1' over four runs:
MIOpen's convolutions do not repeat their bits)."""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_golden_perceptual as mgp
import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(mgp.CASES))
def test_perceptual_loss_on_the_device_matches_the_reference_in_float64(dev, golden_dir, case):
    from mmsr.models.losses import PerceptualLoss
    gold = np.load(f"{golden_dir}/perceptual_golden.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # random VGG weights: overwritten with the seeded ones
        loss = PerceptualLoss(**mgp.CASES[case][0])
    mgp.fill_vgg(loss.vgg.vgg_net)
    loss = loss.to(dev)
    x, gt = (torch.from_numpy(a).to(dev) for a in mgp.images(case))
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
    want = torch.from_numpy(gold[f"{case}.grad"]).to(dev)
    e = float((x.grad.double() - want).abs().max() / want.abs().max())
    print(case, "grad e", e)
    assert e <= 2e-5, e


# ---- the model ----------------------------------------------------------------------------------------------------------

PERCEPTUAL_OPT = {"layer_weights": {"relu2_1": 1.0}, "criterion": "fro", "norm_img": False, "perceptual_weight": 1e-2}


def _train_opt(pretrain_steps=None, hip_graph=False):
    """The smallest RefRestorationModel of the per-rank training tests (tests/test_restoration_gpu.py)."""
    train = {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6, "weight_decay_g": 0,
             "beta_g": [0.9, 0.999], "pixel_weight": 1.0, "hip_graph": hip_graph}
    if pretrain_steps is not None:
        train.update(perceptual_opt=copy.deepcopy(PERCEPTUAL_OPT), net_g_pretrain_steps=pretrain_steps)
    return {"dist": False, "gpu_ids": [0], "is_train": True, "path": {},
            "network_g": {"type": "RestorationNet", "ngf": 64, "n_blocks": 2, "groups": 8},
            "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                            "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
            "network_extractor": {"type": "ContrasExtractorSep"}, "train": train}


def _train_batch(B=2, h=16, seed=4000):
    gt = torch.from_numpy(synth.uniform((B, 3, 4 * h, 4 * h), seed, 0.0, 1.0))
    lq = F.interpolate(gt, scale_factor=0.25, mode="bicubic", align_corners=False).clamp(0, 1)
    up = F.interpolate(lq, scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    ref = torch.from_numpy(synth.uniform((B, 3, 4 * h, 4 * h), seed + 1, 0.0, 1.0))
    return {"img_in_lq": lq, "img_ref": ref, "img_in": gt, "img_in_up": up}


def _models(opts, seed):
    """One RefRestorationModel per opt, all with the first one's initial state and the seeded perceptual tower."""
    from mmsr.models.base_model import unwrap
    from mmsr.models.ref_restoration_model import RefRestorationModel
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        models = [RefRestorationModel(o) for o in opts]
    for stage in ("small", "medium", "large"):
        torch.nn.init.normal_(getattr(unwrap(models[0].net_g).dyn_agg_restore, f"{stage}_dyn_agg").conv_offset_mask.weight, std=0.01)
    for m in models:
        if m is not models[0]:
            for name in ("net_g", "net_map", "net_extractor"):
                getattr(m, name).load_state_dict(getattr(models[0], name).state_dict())
        if m.cri_perceptual is not None:
            mgp.fill_vgg(m.cri_perceptual.vgg.vgg_net)
    return models


def _compare_parameters(a, b, steps):
    """The tolerance of the captured-step test (test_hip_graph_training_step_matches_the_eager_step): Adam normalises every
    gradient entry, so entries whose gradient is atomics-noise can walk apart by up to 2 * lr per step between any two runs;
    the bulk must coincide."""
    worst, moved, same = 0.0, 0, 0
    for (_, pa), (_, pb) in zip(a.net_g.named_parameters(), b.net_g.named_parameters()):
        d = (pa.detach() - pb.detach()).abs()
        worst = max(worst, float(d.max()))
        moved += int((d > 1e-5).sum())
        same += d.numel()
    print(f"parameters after {steps} steps: worst {worst:.3e}, moved {moved} of {same}")
    assert worst <= 2 * steps * 1e-4 + 1e-6, worst
    assert moved < 0.02 * same, (moved, same)


@pytest.fixture()
def train_kernels():
    """Hand-written (deterministic) convolution kernels in the decoder's training step, as in the captured-step test."""
    import mmsr.models.archs.ref_restoration_arch as arch
    old = arch._TRAIN_KERNELS
    arch._TRAIN_KERNELS = "1"
    yield
    arch._TRAIN_KERNELS = old


def test_model_two_phase_step_matches_a_torch_restatement(dev, train_kernels):
    model, plain = _models([_train_opt(pretrain_steps=1), _train_opt()], seed=21)
    assert plain.cri_perceptual is None and model.net_g_pretrain_steps == 1
    assert not any(k.startswith("cri_perceptual") for k in model.net_g.state_dict())
    batches = [_train_batch(seed=4400 + 10 * s) for s in (1, 2)]
    # step 1: the pixel loss alone
    for m in (model, plain):
        m.feed_data(batches[0])
        m.optimize_parameters(1)
    assert list(model.log_dict) == ["l_pix"] and isinstance(model.log_dict["l_pix"], torch.Tensor)
    assert float(model.log_dict["l_pix"]) == pytest.approx(float(plain.log_dict["l_g_pix"]), rel=1e-4)
    # step 2: pixel + perceptual; the restatement is torch's own operators on the same seeded tower
    model.feed_data(batches[1])
    model.optimize_parameters(2)
    assert sorted(model.log_dict) == ["l_g_percep", "l_g_pix"]
    plain.feed_data(batches[1])
    plain._correspondence()
    out = plain.net_g(plain.img_in_lq, plain.pre_offset, plain.img_ref_feat)
    plain.optimizer_g.zero_grad()
    vgg = model.cri_perceptual.vgg

    def relu2_1(img):
        f = (img - vgg.mean) / vgg.std
        for name in ("conv1_1", "conv1_2", "pool1", "conv2_1"):
            layer = vgg.vgg_net._modules[name]
            f = F.max_pool2d(f, 2) if name == "pool1" else F.relu(F.conv2d(f, layer.weight, layer.bias, padding=1))
        return f
    l_pix = (out - plain.gt).abs().mean()
    with torch.no_grad():
        f_gt = relu2_1(plain.gt)
    l_percep = torch.norm(relu2_1(out) - f_gt) * 1e-2
    (l_pix + l_percep).backward()
    plain.optimizer_g.step()
    torch.cuda.synchronize()
    print("l_g_pix", float(model.log_dict["l_g_pix"]), float(l_pix.detach()), "l_g_percep", float(model.log_dict["l_g_percep"]),
          float(l_percep.detach()))
    assert float(model.log_dict["l_g_pix"]) == pytest.approx(float(l_pix.detach()), rel=1e-4)
    assert float(model.log_dict["l_g_percep"]) == pytest.approx(float(l_percep.detach()), rel=1e-4)
    _compare_parameters(model, plain, 2)


def test_model_captured_phases_match_the_eager_run(dev, train_kernels):
    eager, graphed = _models([_train_opt(pretrain_steps=3), _train_opt(pretrain_steps=3, hip_graph=True)], seed=22)
    assert graphed._graph_on and not eager._graph_on
    keys = []
    for step in range(1, 9):
        data = _train_batch(seed=4500 + 10 * step)
        for m in (eager, graphed):
            m.feed_data(data)
            m.optimize_parameters(step)
        keys.append(sorted(graphed.log_dict))
        if step in (3, 8):
            assert graphed._graph is not None      # each phase: two eager warm-up steps, then its own captured step
        if step == 4:
            assert graphed._graph is None          # crossing net_g_pretrain_steps dropped the pixel-only graph
    torch.cuda.synchronize()
    assert keys == [["l_pix"]] * 3 + [["l_g_percep", "l_g_pix"]] * 5, keys
    for k in ("l_g_pix", "l_g_percep"):
        assert float(graphed.log_dict[k]) == pytest.approx(float(eager.log_dict[k]), rel=1e-3), k
    _compare_parameters(eager, graphed, 8)
