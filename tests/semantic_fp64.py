"""The semantic guidance term of stage 1 restated in fp64 (reference: VQModel_arch.py:85-88, F.mse_loss(conv_semantic(quant), vgg_feat)), the
error bounds of the fused kernel counted from csrc/vq_semantic.hip, and the VGG19 trunk down to relu3_4 as plain torch fp64 ops with
seeded weights (the published file cannot be obtained offline).  A plain module like tolerances.py; no GPU."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # one fp32 rounding, relative
COUT = 256


def semantic(q, W, b, feat):
    """q [N,3], W [256,3], b [256], feat [N,256], any float dtype -> fp64 (loss, dq [N,3], dW [256,3], db [256]): the mse of
    relu(W q + b) against feat and its gradients, ReLU's gradient at exactly 0 being 0."""
    q, W, b, feat = (t.detach().double() for t in (q, W.reshape(COUT, 3), b, feat))
    pre = q @ W.t() + b
    d = pre.clamp_min(0) - feat
    k = 2.0 / d.numel()
    e = d * (pre > 0)
    return 0.5 * k * (d * d).sum(), k * (e @ W), k * (e.t() @ q), k * e.sum(0)


def geometry(n_tokens):
    """(workgroups, tokens per workgroup, tokens per wave at most) of glare_vq_semantic_bf16, as include/glare_hip.h states them."""
    g = min(512, -(-n_tokens // 64))
    chunk = -(-n_tokens // g)
    return -(-n_tokens // chunk), chunk, -(-chunk // 4)


def bounds(q, W, b, feat, pre_roundings=6):
    """Per output element, (roundings on its path) * U * (sum of the magnitudes of its terms), counted beside the source lines of
    csrc/vq_semantic.hip -> fp64 (loss, dq, dW, db).  pre_roundings: 6 (three products, three sums) in general, 0 where every product
    and sum of the pre-activation is exact (the grid inputs of tests/test_gpu_vq_semantic.py).  The error of d = relu(pre) - feat is then
    ed = pre_roundings U (|W| |q| + |b|) + U |d|, carried into every sum; a sum's depth is the longest chain of additions a term passes:
      loss  a lane's chain 4 * tokens per wave, 6 shuffle steps, 3 waves, the workgroups (8 slices of ceil(groups / 8) in order, then the
            slices: ceil(groups / 8) - 1 + 7); + 1 for the square, + 2 for k / 2
      dq    1 for e W, 3 for the lane's four channels, 6 shuffle steps, + 2 for k
      dW    1 for e q, tokens per wave, 3 waves, the workgroups as above, + 2 for k            db: the same without the product
    A ReLU decision that rounding flips (|pre| <= its own error) is covered for the loss, not for the gradients: the gradient tests use
    inputs whose pre-activations are exact."""
    q, W, b, feat = (t.detach().double() for t in (q, W.reshape(COUT, 3), b, feat))
    groups, chunk, per_wave = geometry(q.shape[0])
    pre = q @ W.t() + b
    d = pre.clamp_min(0) - feat
    k = 2.0 / d.numel()
    ed = pre_roundings * U * (q.abs() @ W.abs().t() + b.abs()) + U * d.abs()
    on = (pre > 0).double()
    e, ee = d.abs() * on, ed * on
    tail = 3 + (-(-groups // 8) - 1 + 7) + 2
    loss = 0.5 * k * ((2 * d.abs() * ed).sum() + (1 + 4 * per_wave + 6 + tail) * U * (d * d).sum())
    dq = k * (ee @ W.abs() + (1 + 3 + 6 + 2) * U * (e @ W.abs()))
    dW = k * (ee.t() @ q.abs() + (1 + per_wave + tail) * U * (e.t() @ q.abs()))
    db = k * (ee.sum(0) + (per_wave + tail) * U * e.sum(0))
    return loss, dq, dW, db


def grid_case(n_tokens, seed, dtype16):
    """Inputs whose ReLU mask cannot depend on rounding: q, W, b multiples of 2^-6 in [-2, 2], so every pre-activation is a multiple of
    2^-12 below 16 -- exact in fp32 in any order, FMA included -- and exact zeros occur by themselves.  Channel 5: W = 0, b = 0 (pre is
    0 everywhere); channel 9: b = -8 (dead everywhere); token 0 also q = 0.  feat: random, rounded to the 16-bit format.
    -> fp32 q [N,3], W [256,3], b [256], 16-bit feat [N,256]."""
    g = torch.Generator().manual_seed(seed)
    grid = lambda *shape: torch.randint(-128, 129, shape, generator=g).float() / 64.0
    q, W, b = grid(n_tokens, 3), grid(COUT, 3), grid(COUT)
    W[5], b[5] = 0.0, 0.0
    b[9] = -8.0
    q[0] = 0.0
    feat = (torch.randn(n_tokens, COUT, generator=g).abs() * 1.5).to(dtype16)
    return q, W, b, feat


# ---- VGG19 down to relu3_4 ------------------------------------------------------------------------------------------------------------
VGG19_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (16, 256, 256))
VGG19_POOLS = (4, 9)
VGG19_NAMES = {0: "conv1_1", 2: "conv1_2", 5: "conv2_1", 7: "conv2_2", 10: "conv3_1", 12: "conv3_2", 14: "conv3_3", 16: "conv3_4"}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def seeded_vgg19(seed, form="torchvision", whole=False):
    """A seeded state dict of the trunk, He-scaled (std sqrt(2 / fan_in)) so that relu3_4 is not all zero, biases N(0, 0.05).
    form: "torchvision" (`features.N.weight|bias`) or "vgg_net" (`vgg_net.convX_Y.weight|bias`, the reference extractor's).
    whole: also what the trunk has no use for -- the next conv (features.19) and a classifier tensor, as zeros."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in VGG19_CONVS:
        stem = "features.%d" % idx if form == "torchvision" else "vgg_net." + VGG19_NAMES[idx]
        sd[stem + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd[stem + ".bias"] = torch.randn(cout, generator=g) * 0.05
    if whole:
        stem = "features.19" if form == "torchvision" else "vgg_net.conv4_1"
        sd[stem + ".weight"], sd[stem + ".bias"] = torch.zeros(512, 256, 3, 3), torch.zeros(512)
        sd["classifier.6.bias"] = torch.zeros(1000)
    return sd


def vgg16_shaped():
    """torchvision's vgg16.features keys down to its conv4_1, zeros: index 16 is a pool there, so `features.16.*` does not exist."""
    sd = {}
    for idx, cin, cout in VGG19_CONVS[:7] + ((17, 256, 512),):
        sd["features.%d.weight" % idx], sd["features.%d.bias" % idx] = torch.zeros(cout, cin, 3, 3), torch.zeros(cout)
    return sd


def vgg19_relu3_4(x_nchw, sd):
    """fp64: (x - mean) / std with the float32 statistics of the reference's extractor (vgg_arch.py:134-152), then conv / relu / maxpool
    of vgg19.features[:18] under torchvision's keys -> [B, 256, H/4, W/4]."""
    h = (x_nchw.double() - torch.tensor(MEAN).double().view(1, 3, 1, 1)) / torch.tensor(STD).double().view(1, 3, 1, 1)
    for idx in range(17):
        if idx in VGG19_POOLS:
            h = F.max_pool2d(h, 2, 2)
        elif "features.%d.weight" % idx in sd:
            h = F.relu(F.conv2d(h, sd["features.%d.weight" % idx].double(), sd["features.%d.bias" % idx].double(), padding=1))
    return h
