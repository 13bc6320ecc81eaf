"""The patch discriminator of the stage-1 GAN term: taming's NLayerDiscriminator (the PatchGAN of pix2pix), which the reference's
VQModel is written against (`self.loss(qloss, x, xrec, optimizer_idx, ...)`, VQModel_arch.py:110-160) but does not ship.  Definition,
initialisation and state-dict keys are taming's (taming/modules/discriminator/model.py), so a `_D.pth` loads into either.

HIP path: `train_nhwc` runs every layer with a tape on csrc/conv4x4.hip and csrc/disc_ops.hip (glare_amd.autograd)."""
import torch
import torch.nn as nn

from ._base import HipModule
from .. import autograd as A


def weights_init(m):
    """taming's: conv weights N(0, 0.02); BatchNorm weights N(1, 0.02), biases 0."""
    name = m.__class__.__name__
    if name.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif name.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


def nlayer_sequential(input_nc=3, ndf=64, n_layers=3):
    """The `main` Sequential: Conv(s2, bias) LReLU | n_layers - 1 x [Conv(s2) BN LReLU] | Conv(s1) BN LReLU | Conv(s1, bias) -> 1 channel."""
    seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(0.2, True)]
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2, 1, bias=False), nn.BatchNorm2d(ndf * mult), nn.LeakyReLU(0.2, True)]
    prev, mult = mult, min(2 ** n_layers, 8)
    seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 1, 1, bias=False), nn.BatchNorm2d(ndf * mult), nn.LeakyReLU(0.2, True)]
    seq += [nn.Conv2d(ndf * mult, 1, 4, 1, 1)]
    return nn.Sequential(*seq)


class NLayerDiscriminator(HipModule):
    def __init__(self, input_nc=3, ndf=64, n_layers=3):
        super().__init__()
        self.main = nlayer_sequential(input_nc, ndf, n_layers)
        self.apply(weights_init)

    def train_nhwc(self, x_nhwc_f32, groups=1):
        """x fp32 NHWC [B, H, W, 3] -> logits fp32 NHWC [B, OH, OW, 1], BatchNorm in training mode (batch statistics; the running
        buffers move).  groups: the batch as that many runs of consecutive images with batch statistics of their own -- real and fake
        batches in one pass give what two separate passes give."""
        A.ops.require_cuda(x_nhwc_f32)
        assert x_nhwc_f32.dtype == torch.float32 and x_nhwc_f32.dim() == 4
        layers = list(self.main)
        h, i = x_nhwc_f32, 0
        while i < len(layers):
            conv = layers[i]
            assert isinstance(conv, nn.Conv2d) and conv.kernel_size == (4, 4) and conv.padding == (1, 1)
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            if nxt is None:                                            # the logits: fp32, no activation
                return A.conv4x4(h, conv.weight, conv.bias, stride=conv.stride[0], out_f32=True)
            if isinstance(nxt, nn.LeakyReLU):                          # layer 1: bias + LeakyReLU in the conv's epilogue
                h = A.conv4x4(h, conv.weight, conv.bias, stride=conv.stride[0], lrelu=True)
                i += 2
            else:                                                      # conv -> BatchNorm + LeakyReLU (one set of launches)
                assert isinstance(nxt, nn.BatchNorm2d) and isinstance(layers[i + 2], nn.LeakyReLU)
                h = A.conv4x4(h, conv.weight, conv.bias, stride=conv.stride[0])
                h = A.batchnorm_lrelu(h, nxt.weight, nxt.bias, nxt.running_mean, nxt.running_var, nxt.num_batches_tracked, groups=groups,
                                      lrelu=True, eps=nxt.eps, momentum=nxt.momentum)
                i += 3
        raise AssertionError("the Sequential does not end in a conv")

    def forward(self, x_nchw):
        """NCHW in, NCHW logits out (the module surface taming's has)."""
        return A.nhwc_to_nchw(self.train_nhwc(A.nchw_to_nhwc_f32(x_nchw)))
