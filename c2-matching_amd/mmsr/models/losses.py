"""The perceptual (VGG feature) loss of stage-3 GAN training: ``PerceptualLoss`` with the semantics of the reference's class
of that name (losses.py:141-238; options/train/stage3_restoration_gan.yml: ``relu5_1`` of VGG19, ``criterion: fro``, weight
1e-4), written for this project.

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
