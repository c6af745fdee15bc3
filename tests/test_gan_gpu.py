"""GPU tests of stage-3 GAN training: the fused WGAN-GP penalty op (csrc/gp_penalty.hip) against the float64 composition,
GradientPenaltyLoss on the device against the float64 fixture of the reference (tests/golden/make_golden_gan.py), and
RefRestorationModel's critic / generator step, eager and under ``hip_graph``.

Bars.  The project's convention (tests/test_perceptual_gpu.py): the hand-written path is allowed four times the gap that the
stock float32 composition shows against float64 on the same device and the same inputs.  Each test prints the stock gap next
to its own figure before it asserts.  Measured on an MI355X:

  op, per shape (OP_CASES holds the stock gaps; both they and the op's figures repeated exactly in every run)
    N x M        value: stock   fused     dG / max |dG|: stock   fused
    2 x 48              5.1e-9  5.1e-9                   1.22e-7  3.9e-8
    3 x 4551            4.4e-8  3.0e-8                   1.68e-7  4.8e-8
    4 x 76800           8.5e-8  1.2e-8                   1.22e-7  9.0e-8
    2 x 4099 (zero row) 6.2e-9  6.2e-9                   6.6e-8   1.59e-7
  loss vs fixture (MIOpen's convolution backward does not repeat its bits; worst stock of five runs sets the bar)
    value       stock (fused=False) 1.2e-7 .. 1.167e-6   bar 4 x 1.167e-6 = 4.7e-6   fused 2.4e-7 .. 1.05e-6
    gradients   stock 3.5e-6 .. 5.559e-6 of the largest recorded entry   bar 4 x 5.559e-6 = 2.2e-5   fused 3.6e-6 .. 5.7e-6"""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_golden_gan as mgg
import make_golden_perceptual as mgp
import synth

pytestmark = pytest.mark.gpu

BAR_LOSS_VALUE = 4 * 1.167e-6
BAR_LOSS_GRAD = 4 * 5.559e-6

NORMS = (0.3, 2.5, 7.0)      # away from the cancellation of (norm - 1) at 1
GOUT = 1.7                   # the op's backward reads its incoming gradient from the device


def _composition(g):
    return ((g.flatten(1).norm(2, dim=1) - 1) ** 2).mean()


def _samples(N, M, seed, norms=NORMS, zero=None):
    """fp32 [N, M] on the host whose rows have (about) the norms given, cycled; row `zero` is all zero."""
    g = synth.gaussish((N, M), seed).astype(np.float64)
    for n in range(N):
        g[n] *= norms[n % len(norms)] / np.linalg.norm(g[n])
    if zero is not None:
        g[zero] = 0.0
    return torch.from_numpy(g.astype(np.float32))


def _value_and_grad(fn, g):
    g = g.detach().clone().requires_grad_(True)
    v = fn(g)
    (v * GOUT).backward()
    return v.detach(), g.grad


# N, M, index of an all-zero sample, the stock composition's measured gap to float64: value, dG
OP_CASES = [(2, 48, None, 5.055e-9, 1.223e-7),          # less than one block
            (3, 4551, None, 4.409e-8, 1.677e-7),        # odd: rows 1, 2 not 16-byte aligned, ragged last group and slice
            (4, 76800, None, 8.503e-8, 1.219e-7),       # the training shape (3 x 160 x 160): 19 slices per sample
            (2, 4099, 1, 6.179e-9, 6.596e-8)]           # one sample all zero


@pytest.mark.parametrize("N,M,zero,gap_value,gap_dg", OP_CASES)
def test_penalty_op_matches_the_float64_composition(dev, N, M, zero, gap_value, gap_dg):
    from c2m_amd import ops
    g = _samples(N, M, 9800 + N + M, zero=zero).to(dev)
    want_v, want_dg = _value_and_grad(_composition, g.double())
    stock_v, stock_dg = _value_and_grad(_composition, g)
    g_in = g.detach().clone().requires_grad_(True)
    got_v, norms = ops.gradient_penalty(g_in, with_norms=True)
    assert got_v.shape == () and got_v.dtype == torch.float32 and norms.shape == (N,) and not norms.requires_grad
    (got_v * GOUT).backward()
    got_dg = g_in.grad
    scale = float(want_dg.abs().max())

    def gaps(v, dg):
        return abs(float(v.detach()) - float(want_v)) / abs(float(want_v)), float((dg.double() - want_dg).abs().max()) / scale
    e_v, e_dg = gaps(got_v, got_dg)
    s_v, s_dg = gaps(stock_v, stock_dg)
    print(f"N {N} M {M}: value rel err fused {e_v:.3e} stock {s_v:.3e}; dG err / max|dG| fused {e_dg:.3e} stock {s_dg:.3e}")
    assert bool(torch.isfinite(got_v)) and bool(torch.isfinite(norms).all()) and bool(torch.isfinite(got_dg).all())
    assert float((norms.double() - g.double().norm(2, dim=1)).abs().max()) <= 1e-6 * max(NORMS)
    if zero is not None:
        assert float(norms[zero]) == 0.0 and float(got_dg[zero].abs().max()) == 0.0
    assert e_v <= 4 * gap_value, (e_v, s_v)
    assert e_dg <= 4 * gap_dg, (e_dg, s_dg)


def test_penalty_op_next_to_norm_one_is_finite_and_of_the_right_sign(dev):
    from c2m_amd import ops
    g = _samples(2, 4099, 9820, norms=(1.0 + 1e-3,)).to(dev).requires_grad_(True)
    v = ops.gradient_penalty(g)
    v.backward()
    assert bool(torch.isfinite(v)) and float(v.detach()) > 0.0 and bool(torch.isfinite(g.grad).all())
    # norm > 1: the penalty pulls every entry towards 0, dG has the sign of G
    assert bool((g.grad * g.detach() >= 0).all()) and float((g.grad * g.detach()).sum()) > 0.0


def test_penalty_op_repeats_its_bits_whatever_the_alignment(dev):
    from c2m_amd import ops
    N, M = 3, 4551
    host = _samples(N, M, 9830)

    def run(t):
        t = t.detach().requires_grad_(True)
        v, norms = ops.gradient_penalty(t, with_norms=True)
        v.backward()
        return v.detach(), norms, t.grad
    g = host.to(dev)
    first, second = run(g), run(g)
    # the same values one element further on: no row is 16-byte aligned any more where row 0 was
    shifted = torch.empty(N * M + 1, device=dev)[1:].view(N, M).copy_(g)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    third = run(shifted)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_penalty_op_takes_views_and_4d_gradients_and_refuses_the_rest(dev):
    import c2m_amd
    ops = c2m_amd.ops
    g = _samples(2, 3 * 8 * 6, 9840).to(dev)
    want = ops.gradient_penalty(g)
    assert torch.equal(ops.gradient_penalty(g.view(2, 3, 8, 6)), want)
    t = g.view(2, 3, 8, 6).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)      # same values, not contiguous
    t = t.detach().requires_grad_(True)
    v = ops.gradient_penalty(t)
    v.backward()
    assert not t.is_contiguous() and torch.equal(v.detach(), want) and t.grad.shape == t.shape
    with pytest.raises(c2m_amd.C2MError):
        ops.gradient_penalty(g.cpu())
    with pytest.raises(c2m_amd.C2MError):
        ops.gradient_penalty(g.double())
    with pytest.raises(c2m_amd.C2MError):
        ops.gradient_penalty(g.half())


# ---- GradientPenaltyLoss on the device against the reference's float64 results ------------------------------------------

@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/gan_golden.npz")


def _loss_gaps(gold, dev, fused):
    from mmsr.models.archs.discriminator_arch import ImageDiscriminator
    from mmsr.models.losses import GradientPenaltyLoss
    net = ImageDiscriminator(3, ndf=mgg.NDF)
    mgg.fill_critic(net)
    net = net.to(dev).train()
    real, fake = (torch.from_numpy(a).to(dev) for a in mgg.gp_inputs())
    alpha = torch.from_numpy(gold["gp.alpha"]).float().to(dev)
    loss = GradientPenaltyLoss(mgg.GP_WEIGHT, fused=fused)(net, real, fake, alpha=alpha)
    loss.backward()
    params = dict(net.named_parameters())
    scale = max(float(np.abs(gold["gp.grad." + name]).max()) for name in mgg.GP_PARAMETERS)
    e_g = max(float(np.abs(params[name].grad[:rows].double().cpu().numpy() - gold["gp.grad." + name]).max())
              for name, rows in mgg.GP_PARAMETERS.items()) / scale
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    return abs(loss.item() - float(gold["gp.value"])) / abs(float(gold["gp.value"])), e_g


@pytest.mark.parametrize("fused", [True, False])
def test_gradient_penalty_loss_on_the_device_matches_the_reference_in_float64(dev, gold, fused):
    e_v, e_g = _loss_gaps(gold, dev, fused)
    print(f"fused {fused}: value rel err {e_v:.3e}, parameter gradients err / largest recorded entry {e_g:.3e}")
    assert e_v <= BAR_LOSS_VALUE, e_v
    assert e_g <= BAR_LOSS_GRAD, e_g


def test_gradient_penalty_loss_draws_alpha_on_the_device(dev):
    from mmsr.models.archs.discriminator_arch import ImageDiscriminator
    from mmsr.models.losses import GradientPenaltyLoss
    net = ImageDiscriminator(3, ndf=mgg.NDF)
    mgg.fill_critic(net)
    net = net.to(dev).train()
    real, fake = (torch.from_numpy(a).to(dev) for a in mgg.gp_inputs())
    cri = GradientPenaltyLoss(mgg.GP_WEIGHT)
    torch.manual_seed(31)
    drawn = cri(net, real, fake)
    torch.manual_seed(31)
    alpha = torch.rand(2, 1, 1, 1, device=dev)
    given = cri(net, real, fake, alpha=alpha)
    assert float(drawn) == pytest.approx(float(given), rel=1e-5)       # (MIOpen's convolutions need not repeat their bits)


# ---- the model ----------------------------------------------------------------------------------------------------------

PERCEPTUAL_OPT = {"layer_weights": {"relu2_1": 1.0}, "criterion": "fro", "norm_img": False, "perceptual_weight": 1e-2}
GAN_WEIGHT, GP_WEIGHT, LR_D = 1e-3, 10, 1e-4
LOG_KEYS = ["l_d_real", "out_d_real", "l_d_fake", "out_d_fake", "l_grad_penalty", "l_g_pix", "l_g_percep", "l_g_gan"]


def _train_opt(pretrain_steps, critic=True, hip_graph=False, **train_extra):
    """The smallest RefRestorationModel of the perceptual tests (tests/test_perceptual_gpu.py), with a critic."""
    train = {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6, "weight_decay_g": 0,
             "beta_g": [0.9, 0.999], "pixel_weight": 1.0, "hip_graph": hip_graph,
             "perceptual_opt": copy.deepcopy(PERCEPTUAL_OPT), "net_g_pretrain_steps": pretrain_steps}
    opt = {"dist": False, "gpu_ids": [0], "is_train": True, "path": {},
           "network_g": {"type": "RestorationNet", "ngf": 64, "n_blocks": 2, "groups": 8},
           "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                           "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
           "network_extractor": {"type": "ContrasExtractorSep"}, "train": train}
    if critic:
        opt["network_d"] = {"type": "ImageDiscriminator", "in_nc": 3, "ndf": 8}
        train.update(gan_type="wgan", gan_weight=GAN_WEIGHT, grad_penalty_weight=GP_WEIGHT, lr_d=LR_D, weight_decay_d=0,
                     beta_d=[0.9, 0.999])
    train.update(train_extra)
    return opt


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


def _compare_parameters(a, b, steps, what):
    """The tolerance of the captured-step test (tests/test_restoration_gpu.py): Adam normalises every gradient entry, so entries
    whose gradient is noise (here also: the critic's convolution biases in front of a BatchNorm, whose gradient is analytically
    zero) can walk apart by up to 2 * lr per step between any two runs; the bulk must coincide."""
    worst, moved, same = 0.0, 0, 0
    for pa, pb in zip(a.parameters(), b.parameters()):
        d = (pa.detach() - pb.detach()).abs()
        worst = max(worst, float(d.max()))
        moved += int((d > 1e-5).sum())
        same += d.numel()
    print(f"{what} after {steps} steps: worst {worst:.3e}, moved {moved} of {same}")
    assert worst <= 2 * steps * 1e-4 + 1e-6, worst
    assert moved < 0.02 * same, (moved, same)


def _snapshot(net):
    return [p.detach().clone() for p in net.parameters()]


def _moved(net, before):
    return any(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))


@pytest.fixture()
def train_kernels():
    """Hand-written (deterministic) convolution kernels in the decoder's training step, as in the captured-step test."""
    import mmsr.models.archs.ref_restoration_arch as arch
    old = arch._TRAIN_KERNELS
    arch._TRAIN_KERNELS = "1"
    yield
    arch._TRAIN_KERNELS = old


def test_model_gan_step_matches_a_torch_restatement(dev, train_kernels):
    model, plain = _models([_train_opt(1), _train_opt(1, critic=False)], seed=41)
    assert len(model.optimizers) == 2 and plain.net_d is None and model.cri_grad_penalty.fused
    critic = copy.deepcopy(model.net_d)                       # the restatement's critic and its Adam
    adam_d = torch.optim.Adam(critic.parameters(), lr=LR_D, weight_decay=0, betas=(0.9, 0.999))
    batches = [_train_batch(seed=4600 + 10 * s) for s in (1, 2)]
    # step 1: the pixel loss alone; the critic is not touched
    d0 = _snapshot(model.net_d)
    for m in (model, plain):
        m.feed_data(batches[0])
        m.optimize_parameters(1)
    assert list(model.log_dict) == ["l_pix"] and not _moved(model.net_d, d0)
    # step 2: the critic's step, then the generator's
    g1 = _snapshot(model.net_g)
    model.feed_data(batches[1])
    torch.manual_seed(77)
    model.optimize_parameters(2)
    assert list(model.log_dict) == LOG_KEYS
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in model.log_dict.values())
    assert _moved(model.net_g, g1) and _moved(model.net_d, d0)
    assert all(p.requires_grad for p in model.net_d.parameters())

    # the restatement: torch operators, the composition penalty, alpha from the same seed
    plain.feed_data(batches[1])
    torch.manual_seed(77)
    plain._correspondence()
    out = plain.net_g(plain.img_in_lq, plain.pre_offset, plain.img_ref_feat)
    gt, fake = plain.gt, out.detach()
    want = {}
    adam_d.zero_grad()
    real_pred, fake_pred = critic(gt), critic(fake)
    want["l_d_real"], want["out_d_real"] = -real_pred.mean(), real_pred.mean()
    want["l_d_fake"], want["out_d_fake"] = fake_pred.mean(), fake_pred.mean()
    alpha = torch.rand(gt.shape[0], 1, 1, 1, device=dev)
    x_hat = (alpha * gt + (1 - alpha) * fake).requires_grad_(True)
    grad = torch.autograd.grad(critic(x_hat).sum(), x_hat, create_graph=True)[0]
    want["l_grad_penalty"] = GP_WEIGHT * ((grad.flatten(1).norm(2, dim=1) - 1) ** 2).mean()
    (want["l_d_real"] + want["l_d_fake"] + want["l_grad_penalty"]).backward()
    adam_d.step()
    plain.optimizer_g.zero_grad()
    vgg = model.cri_perceptual.vgg

    def relu2_1(img):
        f = (img - vgg.mean) / vgg.std
        for name in ("conv1_1", "conv1_2", "pool1", "conv2_1"):
            layer = vgg.vgg_net._modules[name]
            f = F.max_pool2d(f, 2) if name == "pool1" else F.relu(F.conv2d(f, layer.weight, layer.bias, padding=1))
        return f
    want["l_g_pix"] = (out - gt).abs().mean()
    with torch.no_grad():
        f_gt = relu2_1(gt)
    want["l_g_percep"] = torch.norm(relu2_1(out) - f_gt) * 1e-2
    want["l_g_gan"] = -critic(out).mean() * GAN_WEIGHT
    (want["l_g_pix"] + want["l_g_percep"] + want["l_g_gan"]).backward()
    plain.optimizer_g.step()
    torch.cuda.synchronize()
    for k in LOG_KEYS:
        print(k, float(model.log_dict[k]), float(want[k]))
    for k in LOG_KEYS:
        assert float(model.log_dict[k]) == pytest.approx(float(want[k]), rel=1e-4), k
    _compare_parameters(model.net_g, plain.net_g, 2, "net_g")
    _compare_parameters(model.net_d, critic, 1, "net_d")


def test_model_net_d_init_steps_holds_the_generator_back(dev, train_kernels):
    (model,) = _models([_train_opt(1, net_d_init_steps=2)], seed=42)
    moved = {}
    for step in range(1, 5):
        g, d = _snapshot(model.net_g), _snapshot(model.net_d)
        model.feed_data(_train_batch(seed=4700 + 10 * step))
        model.optimize_parameters(step)
        moved[step] = (_moved(model.net_g, g), _moved(model.net_d, d))
        if step in (2, 3):
            assert list(model.log_dict) == LOG_KEYS[:5]
    assert list(model.log_dict) == LOG_KEYS
    assert moved == {1: (True, False), 2: (False, True), 3: (False, True), 4: (True, True)}, moved


def test_model_with_hip_graph_captures_the_pretrain_phase_and_runs_the_gan_phase_eagerly(dev, train_kernels):
    (model,) = _models([_train_opt(3, hip_graph=True)], seed=43)
    assert model._graph_on
    for step in range(1, 6):
        d = _snapshot(model.net_d)
        model.feed_data(_train_batch(seed=4800 + 10 * step))
        model.optimize_parameters(step)
        if step <= 3:
            assert list(model.log_dict) == ["l_pix"] and not _moved(model.net_d, d)
        if step == 3:
            assert model._graph is not None        # two eager warm-up steps, then the captured step
        if step >= 4:
            assert model._graph is None            # crossing net_g_pretrain_steps dropped it; nothing is captured again
            assert list(model.log_dict) == LOG_KEYS and _moved(model.net_d, d)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in model.log_dict.values())
