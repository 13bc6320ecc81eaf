"""VQGAN prior `net_hq` (mirrors code/models/modules/VQModel_arch.py:14-101): encode / decode as the frozen prior of stages 2 and 3,
and the taped autoencoder `forward(input) -> (dec, diff)` that stage 1 trains (:98-101)."""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import ops
from ._base import HipModule, to_nchw, to_nhwc
from .encoder_decoder import Decoder, Encoder
from .quantize import VectorQuantizer2


class VQModel(HipModule):
    def __init__(self, resolution=256, n_embed=8192, embed_dim=3, ckpt_path=None, double_z=False, z_channels=3,
                 in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 4), num_res_blocks=2, attn_resolutions=(64,), dropout=0.0,
                 **unused):
        super().__init__()
        self.encoder = Encoder(ch, out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                               attn_resolutions=attn_resolutions, in_channels=in_channels, resolution=resolution,
                               z_channels=z_channels, double_z=double_z)
        self.decoder = Decoder(ch, out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                               attn_resolutions=attn_resolutions, in_channels=in_channels, resolution=resolution,
                               z_channels=z_channels)
        self.quantize = VectorQuantizer2(n_embed, embed_dim, beta=0.25)
        self.quant_conv = nn.Conv2d(z_channels, embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, z_channels, 1)
        self.conv_semantic = nn.Sequential(nn.Conv2d(3, 256, 1, 1, 0), nn.ReLU())  # used by train_nhwc(x, vgg_feat) alone

    def _conv1x1_latent(self, conv, z):
        B, H, W, C = z.shape
        return ops.conv2d_smallcin(z, (H * W * C, 1, W * C, C), (B, H, W), conv.weight, conv.bias, out_f32=True)

    def encode_nhwc(self, x_nchw):
        z, _ = self.encoder.forward_nhwc(x_nchw)
        return self._conv1x1_latent(self.quant_conv, z)

    def encode(self, x):  # VQModel_arch.py:74-79
        return to_nchw(self.encode_nhwc(x)), None

    def decode_nhwc(self, z, want_image=False, straight_through=False):
        """z: fp32 NHWC latent [B,h,w,3] -> (indices, image or None, [feat@half, feat@full]).
        straight_through: the codes as `decode` hands them on, z + (z_q - z) in fp32 (quantize.py:298 -- not always z_q to the bit)."""
        B, H, W, C = z.shape
        idx, zq = self.quantize.quantize_tokens(z.view(-1, C))
        if straight_through:
            zq = z.view(-1, C) + (zq - z.view(-1, C))
        quant2 = self._conv1x1_latent(self.post_quant_conv, zq.view(B, H, W, C))
        img, feats = self.decoder.forward_nhwc(quant2, want_image=want_image)
        return idx, img, feats

    def decode(self, h, vgg_feat=None):  # VQModel_arch.py:81-91
        assert vgg_feat is None
        quant, emb_loss, info = self.quantize(h)
        quant2 = self._conv1x1_latent(self.post_quant_conv, to_nhwc(quant, bf16=False))
        dec, feats = self.decoder.forward_nhwc(quant2, want_image=True)
        self.last_indices = info[2]
        return dec, emb_loss, [to_nchw(f) for f in feats]

    semantic_weight = 0.1             # VQModel_arch.py:87: emb_loss += 0.1 * semantic_loss

    def train_nhwc(self, x_nchw, vgg_feat=None):
        """The whole autoencoder with a tape (VQModel_arch.py:98-101, forward = decode(encode(x))): x fp32 NCHW image ->
        (xrec fp32 NHWC, qloss scalar, idx int64 [B*h*w]).  The two 1x1 convs of the 3-channel latent run the thin-input conv with
        weight, bias and data gradients; the codebook layer is autograd.vq_straight_through (csrc/vq_train.hip).
        vgg_feat: None, or the VGG19 relu3_4 map of x (losses.SemanticTarget), 16-bit NHWC [B, h, w, 256] at the latent's size: qloss then
        carries the semantic guidance term of decode() (:85-88), qloss + semantic_weight * mse(conv_semantic(quant), vgg_feat), as one
        fused kernel (autograd.vq_semantic), and `last_semantic` holds the detached mse.  `quant` is the straight-through output, so the
        term's gradient reaches z -- the encoder and quant_conv -- and conv_semantic, never a codebook row (quantize.py:298)."""
        q = self.quantize
        if vgg_feat is not None:      # refused before anything is launched
            f = 2 ** (self.encoder.num_resolutions - 1)
            B, _, H, W = x_nchw.shape
            if H % f or W % f or tuple(vgg_feat.shape) != (B, H // f, W // f, self.conv_semantic[0].out_channels):
                raise ValueError("train_nhwc: a %dx%d input (a multiple of %d is asked) has a %dx%d latent and needs vgg_feat [%d, %d, %d, %d]; "
                                 "got %s" % (H, W, f, H // f, W // f, B, H // f, W // f, self.conv_semantic[0].out_channels, tuple(vgg_feat.shape)))
        h, _ = self.encoder.train_nhwc(x_nchw)
        z = A.conv2d_small(h, self.quant_conv.weight, self.quant_conv.bias, layout="nhwc", out_f32=True)
        w_z, w_e = q.loss_weights()
        zq, qloss, idx = A.vq_straight_through(z, q.embedding.weight, w_z, w_e)
        if vgg_feat is not None:
            sem = A.vq_semantic(zq, self.conv_semantic[0].weight, self.conv_semantic[0].bias, vgg_feat)
            qloss = qloss + self.semantic_weight * sem
            self.last_semantic = sem.detach()
        quant2 = A.conv2d_small(zq, self.post_quant_conv.weight, self.post_quant_conv.bias, layout="nhwc", out_f32=True)
        xrec, _ = self.decoder.train_nhwc(quant2)
        self.last_indices = idx
        self.last_latent = z.detach().reshape(-1, z.shape[-1])        # fp32 [N, 3]: what the codebook layer was fed (Stage1Trainer's restart and EMA update)
        return xrec, qloss, idx

    def forward(self, input):  # VQModel_arch.py:98-101
        """(dec fp32 NCHW, diff): under grad the taped graph above, under no_grad decode(encode(input))."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            xrec, qloss, _ = self.train_nhwc(input)
            return A.nhwc_to_nchw(xrec), qloss
        dec, diff, _ = self.decode(self.encode(input)[0])
        return dec, diff
