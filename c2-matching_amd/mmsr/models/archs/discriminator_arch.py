"""The critic of stage-3 GAN training: ``ImageDiscriminator`` with the layer recipe and ``state_dict`` keys of the reference's
class of that name (archs/discriminator_arch.py:6-43; options/train/stage3_restoration_gan.yml: ``in_nc 3``, ``ndf 32``), so
its ``net_d`` checkpoints load.

It runs on torch's own operators (MIOpen convolutions and BatchNorm on the GPU), by necessity: the WGAN-GP penalty differentiates
the critic's input gradient, and that double backward exists only under autograd.  BatchNorm stays in
train mode during training, as in the reference: every forward of a step normalises by its own batch."""
import torch.nn as nn

from mmsr.models.archs.arch_util import srntt_init_weights

_SLOPE = 0.2


def _conv_block(cin, cout):
    """conv3x3 stride 1 -> BN -> LeakyReLU -> conv3x3 stride 2 -> BN -> LeakyReLU (keys 0, 1, 3, 4 of the block)"""
    layers = []
    for c, stride in ((cin, 1), (cout, 2)):
        layers += [nn.Conv2d(c, cout, 3, stride, 1), nn.BatchNorm2d(cout), nn.LeakyReLU(_SLOPE, inplace=True)]
    return nn.Sequential(*layers)


class ImageDiscriminator(nn.Module):
    """[N, in_nc, H, W] -> [N, 1, 1, 1] in (0, 1): five blocks of widths ndf * {1, 2, 4, 8, 16}, each halving the map, then
    global average pooling, a 1x1 convolution to 1024, LeakyReLU, a 1x1 convolution to 1 and a sigmoid."""

    def __init__(self, in_nc=3, ndf=32):
        super().__init__()
        widths = [in_nc] + [ndf * m for m in (1, 2, 4, 8, 16)]
        for k in range(5):
            setattr(self, f'conv_block{k + 1}', _conv_block(widths[k], widths[k + 1]))
        self.out_block = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(widths[-1], 1024, kernel_size=1),
                                       nn.LeakyReLU(_SLOPE), nn.Conv2d(1024, 1, kernel_size=1), nn.Sigmoid())
        srntt_init_weights(self, init_type='normal', init_gain=0.02)

    def forward(self, x):
        for k in range(5):
            x = getattr(self, f'conv_block{k + 1}')(x)
        return self.out_block(x)
