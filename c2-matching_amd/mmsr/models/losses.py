"""The losses of stage-3 GAN training, written for this project with the semantics of the reference's classes of the same
names: ``PerceptualLoss`` (losses.py:141-238; options/train/stage3_restoration_gan.yml: ``relu5_1`` of VGG19, ``criterion:
fro``, weight 1e-4), ``GANLoss`` (losses.py:275-363; ``gan_type: wgan``) and ``GradientPenaltyLoss`` (losses.py:366-428;
``grad_penalty_weight 10``), the last two at the end of this file.

``PerceptualLoss``:

Two deviations, both deliberate:
* ``criterion='l2'`` builds ``torch.nn.MSELoss()``.  The reference names ``torch.nn.L2loss``, which does not exist, and raises
  on construction.
* Both feature sets come from the same arithmetic: the ground-truth side does not go through the tower's fused no-grad
  inference path (f16 x 2 kernels behind a range check that reads a flag back), so ``loss(x, x)`` is 0 up to what the convolutions
  themselves repeat (exactly 0 on the CPU; MIOpen's kernels need not repeat their bits) and a captured training step never
  reads a value back to the host.

The tower runs on torch's own operators under autograd (``VGGFeatureExtractor.forward_stock``).  A hand-written input-gradient
path for the frozen tower was built and measured, and is not shipped: DESIGN.md section 16 says why.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmsr.models.archs.vgg_arch import VGGFeatureExtractor


class PerceptualLoss(nn.Module):
    """forward(x, gt) -> (perceptual | None, style | None).

    layer_weights: {tap name: weight}; the tower is cut after the last tap.  norm_img: the images are in [-1, 1] and are mapped
    to [0, 1] first; use_input_norm: the tower then applies the ImageNet mean / std.  criterion: 'l1', 'l2' (mean squared
    error) or 'fro' (the Frobenius norm of the feature difference, per layer).  Each layer's term is multiplied by its weight
    and the sum by perceptual_weight; style_weight > 0 adds the same criterion between the Gram matrices f f^T / (c h w) (a style
    term needs 'l1' or 'l2': 'fro' has no criterion module, as in the reference, and is refused at construction).  The features of x carry gradient, those of
    gt are computed without."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, perceptual_weight=1.0, style_weight=0,
                 norm_img=True, criterion='l1'):
        super().__init__()
        self.norm_img = norm_img
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = layer_weights
        self.vgg = VGGFeatureExtractor(list(layer_weights), vgg_type, use_input_norm)
        self.criterion_type = criterion
        if criterion == 'l1':
            self.criterion = nn.L1Loss()
        elif criterion == 'l2':
            self.criterion = nn.MSELoss()
        elif criterion == 'fro':
            self.criterion = None
        else:
            raise NotImplementedError(f'PerceptualLoss: criterion {criterion!r} (one of l1, l2, fro)')
        if style_weight > 0 and self.criterion is None:
            # (the reference fails here too, but only in forward, by calling None)
            raise ValueError("PerceptualLoss: the style term needs criterion 'l1' or 'l2' ('fro' has no criterion module)")

    def _features(self, x, gt):
        with torch.no_grad():
            gt_features = self.vgg.forward_stock(gt.detach())
        return self.vgg.forward_stock(x), gt_features

    @staticmethod
    def _gram(f):
        n, c, h, w = f.shape
        f = f.reshape(n, c, h * w)
        return f.bmm(f.transpose(1, 2)) / (c * h * w)

    def forward(self, x, gt):
        if self.norm_img:
            x, gt = (x + 1.) * 0.5, (gt + 1.) * 0.5
        fx, fg = self._features(x, gt)
        percep = style = None
        if self.perceptual_weight > 0:
            percep = 0
            for k in fx:
                if self.criterion_type == 'fro':
                    term = torch.norm(fx[k] - fg[k], p='fro')
                else:
                    term = self.criterion(fx[k], fg[k])
                percep = percep + term * self.layer_weights[k]
            percep = percep * self.perceptual_weight
        if self.style_weight > 0:
            style = 0
            for k in fx:
                style = style + self.criterion(self._gram(fx[k]), self._gram(fg[k])) * self.layer_weights[k]
            style = style * self.style_weight
        return percep, style


class GANLoss(nn.Module):
    """forward(input, target_is_real, is_disc=False) -> the adversarial loss of a critic prediction.

    gan_type 'vanilla': binary cross-entropy with logits against the label value; 'lsgan': mean squared error against the
    label value; 'wgan': -mean(input) for a real target, +mean(input) for a fake one; 'hinge': mean(relu(1 -/+ input)) for the
    critic, -mean(input) for the generator.  loss_weight scales the generator's loss only (is_disc False); the critic's own
    loss always has weight 1."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        if gan_type not in ('vanilla', 'lsgan', 'wgan', 'hinge'):
            raise NotImplementedError(f'GAN type {gan_type} is not implemented.')
        self.gan_type = gan_type
        self.real_label_val = real_label_val
        self.fake_label_val = fake_label_val
        self.loss_weight = loss_weight

    def forward(self, input, target_is_real, is_disc=False):
        if self.gan_type == 'wgan':
            loss = -input.mean() if target_is_real else input.mean()
        elif self.gan_type == 'hinge':
            if is_disc:
                loss = F.relu(1 - input if target_is_real else 1 + input).mean()
            else:
                loss = -input.mean()
        else:
            label = torch.full_like(input, self.real_label_val if target_is_real else self.fake_label_val)
            loss = F.binary_cross_entropy_with_logits(input, label) if self.gan_type == 'vanilla' else F.mse_loss(input, label)
        return loss if is_disc else loss * self.loss_weight


class GradientPenaltyLoss(nn.Module):
    """The WGAN-GP penalty: forward(discriminator, real_data, fake_data, alpha=None) ->
    loss_weight * mean_n (||d D(x^)/d x^ [n]||_2 - 1)^2 at x^ = alpha * real + (1 - alpha) * fake.detach().

    alpha: [N,1,1,1]; None draws it uniformly in [0, 1) from torch's generator ON the inputs' device (the reference draws on the
    host and copies: a host-to-device copy in every step); a given alpha is used as it is.  No gradient reaches fake_data: the
    reference wraps x^ in ``autograd.Variable(..., requires_grad=True)``, which on current torch makes it a leaf.  The
    reference's inpainting mask is not provided.

    fused (default True): an fp32 gradient on the GPU goes through ``c2m_amd.ops.gradient_penalty`` (two launches forward, one
    backward); anything else -- CPU tensors, other dtypes, fused=False -- takes the torch composition of the same expression."""

    def __init__(self, loss_weight=1.0, fused=True):
        super().__init__()
        self.loss_weight = loss_weight
        self.fused = fused

    @staticmethod
    def penalty_composition(gradients):
        return ((gradients.flatten(1).norm(2, dim=1) - 1) ** 2).mean()

    def forward(self, discriminator, real_data, fake_data, alpha=None):
        if alpha is None:
            alpha = torch.rand(real_data.size(0), 1, 1, 1, dtype=real_data.dtype, device=real_data.device)
        interpolates = (alpha * real_data + (1. - alpha) * fake_data.detach()).detach().requires_grad_(True)
        gradients = torch.autograd.grad(discriminator(interpolates).sum(), interpolates, create_graph=True)[0]
        if self.fused and gradients.is_cuda and gradients.dtype == torch.float32:
            from c2m_amd import ops
            penalty = ops.gradient_penalty(gradients)
        else:
            penalty = self.penalty_composition(gradients)
        return penalty * self.loss_weight
