"""CPU: the stage-3 GAN pieces -- GANLoss, GradientPenaltyLoss and ImageDiscriminator in float64 against the reference's classes
(tests/golden/make_golden_gan.py: seeded weights and inputs, only results are stored), the critic's wiring into
RefRestorationModel, and the C-ABI of include/c2m_gan_hip.h.

Bars: 1e-9 relative for values and gradients.  Both sides are float64 and evaluate the same formulas, so only the order of
the sums differs; anything larger is a formula error.  Gradients are measured against the largest entry of the recorded
tensor (a convolution bias in front of a BatchNorm has an analytically zero gradient: a per-entry relative error means
nothing there)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import make_golden_gan as mgg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(f"{golden_dir}/gan_golden.npz")


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the losses and the critic against the fixture -----------------------------------------------------------------------

@pytest.mark.parametrize("gan_type", mgg.GAN_TYPES)
def test_gan_loss_matches_the_reference_in_float64(gold, gan_type):
    from mmsr.models.losses import GANLoss
    cri = GANLoss(gan_type, loss_weight=mgg.GAN_WEIGHT)
    for is_disc in (True, False):
        for real in (True, False):
            x = torch.from_numpy(mgg.gan_pred()).double().requires_grad_(True)
            v = cri(x, real, is_disc=is_disc)
            v.backward()
            key = f"gan.{gan_type}.{'disc' if is_disc else 'gen'}.{'real' if real else 'fake'}"
            assert v.dim() == 0
            assert _rel(v.item(), gold[key + ".value"]) <= REL, key
            assert _rel(x.grad.numpy(), gold[key + ".grad"]) <= REL, key


def test_gan_loss_weight_applies_to_the_generator_only_and_unknown_types_raise():
    from mmsr.models.losses import GANLoss
    x = torch.from_numpy(mgg.gan_pred())
    for gan_type in mgg.GAN_TYPES:
        a, b = GANLoss(gan_type, loss_weight=1.0), GANLoss(gan_type, loss_weight=0.25)
        assert float(a(x, True, is_disc=True)) == float(b(x, True, is_disc=True))
        assert float(b(x, True)) == pytest.approx(0.25 * float(a(x, True)), rel=1e-6)
    with pytest.raises(NotImplementedError):
        GANLoss('nope')


def _critic(dtype=torch.float64):
    from mmsr.models.archs.discriminator_arch import ImageDiscriminator
    net = ImageDiscriminator(3, ndf=mgg.NDF)
    mgg.fill_critic(net)
    return net.to(dtype).train()


def test_critic_keys_shapes_and_output_match_the_reference(gold):
    net = _critic()
    sd = net.state_dict()
    assert sorted(sd) == [str(k) for k in gold["d.keys"]]
    assert [",".join(str(d) for d in sd[k].shape) for k in sorted(sd)] == [str(s) for s in gold["d.shapes"]]
    with torch.no_grad():
        out = net(torch.from_numpy(mgg.critic_input()).double())
    assert out.shape == (2, 1, 1, 1)
    assert _rel(out.numpy(), gold["d.out"]) <= REL


def test_critic_initialisation_and_registry():
    import mmsr.models.networks as networks
    from mmsr.models.archs.discriminator_arch import ImageDiscriminator
    torch.manual_seed(3)
    net = networks.define_net_d({"network_d": {"type": "ImageDiscriminator", "in_nc": 3, "ndf": 8}})
    assert isinstance(net, ImageDiscriminator)
    # srntt_init_weights(net, 'normal', 0.02): N(0, 0.02) convolution weights, zero biases, BatchNorm weights N(1, 0.02)
    w = net.conv_block4[3].weight
    assert abs(float(w.detach().std()) - 0.02) < 2e-3 and abs(float(w.detach().mean())) < 1e-3
    assert float(net.conv_block2[0].bias.detach().abs().max()) == 0.0 and float(net.out_block[3].bias.detach().abs().max()) == 0.0
    assert abs(float(net.conv_block5[4].weight.detach().mean()) - 1.0) < 0.01 and float(net.conv_block5[4].bias.detach().abs().max()) == 0.0


def test_gradient_penalty_matches_the_reference_in_float64(gold):
    from mmsr.models.losses import GradientPenaltyLoss
    net = _critic()
    real, fake = (torch.from_numpy(a).double() for a in mgg.gp_inputs())
    fake.requires_grad_(True)
    loss = GradientPenaltyLoss(mgg.GP_WEIGHT)(net, real, fake, alpha=torch.from_numpy(gold["gp.alpha"]))
    loss.backward()
    assert _rel(loss.item(), gold["gp.value"]) <= REL
    params = dict(net.named_parameters())
    for name, rows in mgg.GP_PARAMETERS.items():
        assert _rel(params[name].grad[:rows].numpy(), gold["gp.grad." + name]) <= REL, name
    assert fake.grad is None          # x^ is a leaf: nothing reaches the generator through the penalty


def test_gradient_penalty_draws_alpha_from_torchs_generator_and_handles_a_zero_gradient():
    from mmsr.models.losses import GradientPenaltyLoss
    net = _critic(torch.float32)
    real, fake = (torch.from_numpy(a) for a in mgg.gp_inputs())
    cri = GradientPenaltyLoss(2.0)
    torch.manual_seed(11)
    drawn = cri(net, real, fake)
    torch.manual_seed(11)
    alpha = torch.rand(2, 1, 1, 1)
    assert float(drawn) == float(cri(net, real, fake, alpha=alpha))
    # a critic whose output does not depend on its input: gradient 0, penalty (0 - 1)^2, and a finite (zero) backward

    class Flat(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.ones(1))

        def forward(self, x):
            return (x * 0).flatten(1).sum(1) * self.w
    flat = Flat()
    v = cri(flat, real, fake)
    v.backward()
    assert float(v) == 2.0 and bool(torch.isfinite(flat.w.grad).all())


# ---- the model -------------------------------------------------------------------------------------------------------------

class TinyGenerator(nn.Module):
    """Stands in for RestorationNet in the CPU model: the decoder's deformable convolutions exist on the GPU only.  The
    parameter names hit all four optimizer groups."""

    def __init__(self):
        super().__init__()
        self.body = nn.Conv2d(3, 3, 3, padding=1)
        self.large_offset_conv = nn.Conv2d(3, 3, 1)
        self.medium_offset_conv = nn.Conv2d(3, 3, 1)
        self.small_offset_conv = nn.Conv2d(3, 3, 1)

    def forward(self, lq, pre_offset, ref_feat):
        x = F.interpolate(lq, scale_factor=4, mode="bilinear", align_corners=False)
        return x + self.body(x) + self.large_offset_conv(x) + self.medium_offset_conv(x) + self.small_offset_conv(x)


LOG_KEYS = ["l_d_real", "out_d_real", "l_d_fake", "out_d_fake", "l_grad_penalty", "l_g_pix", "l_g_percep", "l_g_gan"]


def _opt(tmp_path=None, **train):
    t = {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6, "weight_decay_g": 0,
         "beta_g": [0.9, 0.999], "pixel_weight": 1.0, "net_g_pretrain_steps": 1,
         "perceptual_opt": {"layer_weights": {"relu1_1": 1.0}, "criterion": "fro", "norm_img": False, "perceptual_weight": 1e-2},
         "gan_type": "wgan", "gan_weight": 1e-3, "grad_penalty_weight": 10, "lr_d": 1e-4, "weight_decay_d": 0,
         "beta_d": [0.9, 0.999]}
    t.update(train)
    path = {} if tmp_path is None else {"models": str(tmp_path), "training_state": str(tmp_path)}
    return {"dist": False, "gpu_ids": None, "is_train": True, "path": path,
            "network_g": {"type": "TinyGenerator"},
            "network_d": {"type": "ImageDiscriminator", "in_nc": 3, "ndf": 4},
            "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                            "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
            "network_extractor": {"type": "ContrasExtractorSep"}, "train": t}


@pytest.fixture()
def cpu_model(monkeypatch):
    """-> make(opt): a RefRestorationModel on the CPU with TinyGenerator registered and the (GPU-only) correspondence search
    replaced by nothing."""
    import warnings
    import mmsr.models.archs.discriminator_arch as registered
    from mmsr.models.ref_restoration_model import RefRestorationModel
    monkeypatch.setattr(registered, "TinyGenerator", TinyGenerator, raising=False)

    def no_correspondence(self):
        self.pre_offset = self.img_ref_feat = None
    monkeypatch.setattr(RefRestorationModel, "_correspondence", no_correspondence)

    def make(opt):
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # random VGG weights
            return RefRestorationModel(opt)
    return make


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(2, 3, 32, 32, generator=g)
    lq = F.interpolate(gt, scale_factor=0.25, mode="bilinear", align_corners=False)
    return {"img_in_lq": lq, "img_ref": torch.rand(2, 3, 32, 32, generator=g), "img_in": gt,
            "img_in_up": F.interpolate(lq, scale_factor=4, mode="bilinear", align_corners=False)}


def _snapshot(net):
    return [p.detach().clone() for p in net.parameters()]


def _moved(net, before):
    return any(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))


def test_cpu_model_runs_a_pretrain_step_then_a_gan_step(cpu_model, tmp_path):
    from mmsr.models.losses import GANLoss, GradientPenaltyLoss
    model = cpu_model(_opt(tmp_path))
    assert len(model.optimizers) == 2 and model.optimizers[1] is model.optimizer_d
    assert isinstance(model.cri_gan, GANLoss) and isinstance(model.cri_grad_penalty, GradientPenaltyLoss)
    assert model.cri_gan.loss_weight == 1e-3 and model.cri_grad_penalty.loss_weight == 10
    assert (model.net_d_steps, model.net_d_init_steps) == (1, 0) and model.net_d.training
    g0, d0 = _snapshot(model.net_g), _snapshot(model.net_d)
    model.feed_data(_batch(1))
    model.optimize_parameters(1)
    assert list(model.log_dict) == ["l_pix"]
    assert _moved(model.net_g, g0) and not _moved(model.net_d, d0)
    g1 = _snapshot(model.net_g)
    model.feed_data(_batch(2))
    model.optimize_parameters(2)
    assert list(model.log_dict) == LOG_KEYS
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for v in model.log_dict.values())
    assert _moved(model.net_g, g1) and _moved(model.net_d, d0)
    assert all(p.requires_grad for p in model.net_d.parameters())       # restored after the generator's step
    assert 0.0 < float(model.log_dict["out_d_fake"]) < 1.0              # the critic ends in a sigmoid
    assert -1e-3 < float(model.log_dict["l_g_gan"]) < 0.0               # wgan, generator side: -gan_weight * mean(D(output))
    assert float(model.log_dict["l_d_fake"]) == float(model.log_dict["out_d_fake"])
    assert float(model.log_dict["l_d_real"]) == -float(model.log_dict["out_d_real"])

    # training state: both optimizers travel; the networks are written by save()
    model.save(0, 2)
    assert sorted(os.listdir(tmp_path)) == ["2.state", "net_d_2.pth", "net_g_2.pth"]
    state = torch.load(tmp_path / "2.state", weights_only=False)
    assert len(state["optimizers"]) == 2
    other = cpu_model(_opt(tmp_path))
    other.resume_training(state)
    for a, b in zip(model.optimizers, other.optimizers):
        sa, sb = a.state_dict()["state"], b.state_dict()["state"]
        assert sorted(sa) == sorted(sb) and len(sa) > 0
        for k in sa:
            assert torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"])
    assert sorted(torch.load(tmp_path / "net_d_2.pth")) == sorted(model.net_d.state_dict())
    other.load_network(other.net_d, str(tmp_path / "net_d_2.pth"))      # (what path.pretrain_model_d does)
    assert all(torch.equal(a, b) for a, b in zip(model.net_d.state_dict().values(), other.net_d.state_dict().values()))


def test_cpu_model_step_gating(cpu_model):
    """net_d_init_steps 2: the critic trains from the first GAN step on, the generator waits until (step - pretrain) > 2;
    net_d_steps 2: afterwards the generator moves on every second step only."""
    model = cpu_model(_opt(net_d_init_steps=2, net_d_steps=2))
    moved = {}
    for step in range(1, 8):
        g, d = _snapshot(model.net_g), _snapshot(model.net_d)
        model.feed_data(_batch(10 + step))
        model.optimize_parameters(step)
        moved[step] = (_moved(model.net_g, g), _moved(model.net_d, d))
        if step in (2, 3):
            assert list(model.log_dict) == LOG_KEYS[:5]
    # (step - 1) % 2 == 0 and (step - 1) > 2: steps 5 and 7
    assert moved == {1: (True, False), 2: (False, True), 3: (False, True), 4: (False, True), 5: (True, True),
                     6: (False, True), 7: (True, True)}, moved


def test_without_network_d_nothing_changes_and_dist_with_it_raises(cpu_model):
    from mmsr.models.ref_restoration_model import RefRestorationModel
    opt = _opt()
    del opt["network_d"]
    model = cpu_model(opt)
    assert model.net_d is None and model.cri_gan is None and len(model.optimizers) == 1
    for step in (1, 2):
        model.feed_data(_batch(step))
        model.optimize_parameters(step)
    assert list(model.log_dict) == ["l_g_pix", "l_g_percep"]
    opt = _opt()
    opt["dist"] = True
    with pytest.raises(NotImplementedError, match="network_d"):
        RefRestorationModel(opt)


# ---- the op's host side and the C-ABI of include/c2m_gan_hip.h ----------------------------------------------------------------

def test_gradient_penalty_op_rejects_cpu_tensors():
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.gradient_penalty(torch.zeros(2, 3, 4, 4))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def _kind(decl):
    if "*" in decl or "c2m_stream_t" in decl:
        return "pointer"
    kind = " ".join(decl.replace("const", " ").split()[:-1])
    assert kind in ("int", "float", "double", "long long", "size_t"), decl
    return kind


def _ctypes_kind(t):
    scalar = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_longlong: "long long",
              ctypes.c_size_t: "size_t"}
    return scalar.get(t, "pointer")


_PROTO = r"^([A-Za-z_][\w \*]*?)\s*\b(c2m_\w+)\s*\(([^()]*)\)\s*;"


def test_gan_header_is_exported_and_mirrored_and_the_main_header_is_unchanged():
    import c2m_amd
    L = c2m_amd._lib.lib()
    protos = re.findall(_PROTO, _header("c2m_gan_hip.h"), flags=re.M)
    assert sorted(n for _, n, _ in protos) == ["c2m_gp_penalty_backward_f32", "c2m_gp_penalty_forward_f32",
                                               "c2m_gp_penalty_workspace_bytes"]
    raw = ctypes.CDLL(c2m_amd.LIB_PATH)
    for ret, name, params in protos:
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(L, name)
        assert _ctypes_kind(fn.restype) == _kind(ret + " _"), name
        want = [_kind(d) for d in " ".join(params.split()).split(",")]
        assert fn.argtypes is not None and [_ctypes_kind(t) for t in fn.argtypes] == want, name
    # purely additive: the main header declares what it declared, at the same ABI version
    main = re.findall(_PROTO, _header("c2m_hip.h"), flags=re.M)
    assert len(main) == 56 and not any("gp_penalty" in n for _, n, _ in main)
    assert L.c2m_abi_version() == 6


def test_penalty_workspace_follows_the_slicing():
    """Pure size arithmetic in the library: one float per slice and sample; slices of at least 4096 elements, at most 256
    of them per sample; invalid sizes give 0."""
    import c2m_amd
    L = c2m_amd._lib.lib()
    ws = L.c2m_gp_penalty_workspace_bytes
    assert ws(2, 48) == 2 * 4 and ws(3, 4551) == 3 * 2 * 4 and ws(4, 76800) == 4 * 19 * 4
    assert ws(1, 4096) == 4 and ws(1, 4097) == 8
    assert ws(1, 256 * 4096) == 256 * 4 and ws(1, 256 * 4096 + 1) == 205 * 4      # slices grow to 5120 elements
    assert ws(0, 10) == 0 and ws(2, 0) == 0 and ws(2, -1) == 0 and ws(70000, 10) == 0
