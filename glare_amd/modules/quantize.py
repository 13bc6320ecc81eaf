"""Codebook retrieval on the HIP nearest-code kernel, and its training form.

Mirrors VectorQuantizer2 (code/models/modules/quantize.py:213-329): same constructor, same
`forward(z) -> (z_q, loss, (perplexity, min_encodings, min_encoding_indices))` contract with
`sane_index_shape=False` semantics (flat int64 indices), both `legacy` orders of the loss, straight-through z_q.
Without a tape (no_grad, or an input that needs no gradient) the lookup is the inference kernel plus elementwise glue; on an
input that requires a gradient (stage 1, VQModel.train_nhwc) the loss, the straight-through output and the gradients of the
latent and of the codebook come from csrc/vq_train.hip through autograd.vq_straight_through."""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import ops
from ._base import HipModule


class VectorQuantizer2(HipModule):
    def __init__(self, n_e, e_dim, beta, remap=None, unknown_index="random", sane_index_shape=False, legacy=False):
        super().__init__()
        assert remap is None, "index remapping is not used by GLARE (VQModel_arch.py:44-45)"
        self.n_e, self.e_dim, self.beta, self.legacy = n_e, e_dim, beta, legacy
        self.embedding = nn.Embedding(n_e, e_dim)
        self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)
        self.remap, self.re_embed, self.sane_index_shape = None, n_e, sane_index_shape
        self.ema_update = False     # Stage1Trainer(codebook_ema=d): the codebook follows an EMA of the latents, not a gradient

    def loss_weights(self):
        """(w_z, w_e) of loss = w_z mean((z_q.detach() - z)^2) + w_e mean((z_q - z.detach())^2): quantize.py:290-295, and under an EMA
        codebook the commitment term alone, beta mean((z_q.detach() - z)^2) (EMAVectorQuantizer.forward, quantize.py:437)."""
        if self.ema_update:
            return (self.beta, 0.0)
        return (1.0, self.beta) if self.legacy else (self.beta, 1.0)

    def quantize_tokens(self, tokens):
        """tokens fp32 [N, e_dim] (NHWC flattening) -> (idx int64 [N], z_q fp32 [N, e_dim])."""
        return ops.vq_nearest(tokens, self.embedding.weight.detach())

    def forward(self, z, temp=None, rescale_logits=False, return_logits=False):
        assert temp is None or temp == 1.0
        assert not rescale_logits and not return_logits
        ops.require_cuda(z)
        if torch.is_grad_enabled() and z.requires_grad:
            # stage-1 training (VQModel_arch.py:98-101): the same lookup with a tape -- the loss sum, the straight-through output and
            # both gradients are kernels of csrc/vq_train.hip (autograd.VQStraightThroughFn), bitwise reproducible
            w_z, w_e = self.loss_weights()
            zq, loss, idx = A.vq_straight_through(A.nchw_to_nhwc_f32(z), self.embedding.weight, w_z, w_e)
            zq = A.nhwc_to_nchw(zq)
            if self.sane_index_shape:
                idx = idx.reshape(zq.shape[0], zq.shape[2], zq.shape[3])
            return zq, loss, (None, None, idx)
        zp = ops.nchw_to_nhwc(z, bf16=False)  # 'b c h w -> b h w c' (quantize.py:276)
        flat = zp.view(-1, self.e_dim)
        idx, zq = self.quantize_tokens(flat)
        zq = zq.view(zp.shape)
        # losses and the straight-through estimator are cheap elementwise torch ops on device (quantize.py:290-298)
        if not self.legacy:
            loss = self.beta * torch.mean((zq.detach() - zp) ** 2) + torch.mean((zq - zp.detach()) ** 2)
        else:
            loss = torch.mean((zq.detach() - zp) ** 2) + self.beta * torch.mean((zq - zp.detach()) ** 2)
        zq = zp + (zq - zp).detach()
        zq = ops.nhwc_to_nchw(zq.contiguous())
        if self.sane_index_shape:
            idx = idx.reshape(zq.shape[0], zq.shape[2], zq.shape[3])
        return zq, loss, (None, None, idx)

    def get_codebook_entry(self, indices, shape):
        zq = self.embedding(indices)
        if shape is not None:
            zq = zq.view(shape).permute(0, 3, 1, 2).contiguous()
        return zq
