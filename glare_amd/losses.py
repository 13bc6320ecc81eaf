"""Stage-3 loss terms on the HIP path: MS-SSIM and the VGG16-feature perceptual loss that
VQLLFLOWDModel.optimize_parameters adds to the L1 term (code/models/VQLLFLOWD_model.py:217-223).

Mirrors code/models/modules/pytorch_msssim/__init__.py:8-98 (`gaussian`, `create_window`, `ssim`, `msssim`) and
code/models/modules/losses.py:12-40 (`PerceptualNetwork`).  Images are NHWC fp32 on the device; the ten SSIM level scalars
and the VGG features come from kernels (csrc/loss_ops.hip, csrc/conv_igemm.hip); the few scalar combinations below are
torch ops on 5-element tensors.
"""
from math import exp

import functools
import os
import re

import torch
import torch.nn as nn

from . import autograd as A
from . import ops
from .modules._base import HipModule

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # pytorch_msssim/__init__.py:73
_WEIGHTS = {}


@functools.lru_cache(maxsize=None)      # five windows per MS-SSIM call, the same every step: built once (was ~15 small CPU tensor ops per step)
def gaussian(window_size, sigma=1.5):
    """The 1-D window of create_window() (:8-17) with the same float32 rounding: its outer product is the 2-D window."""
    g = torch.Tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    return tuple((g / g.sum()).tolist())     # immutable: the cached object is shared by every caller


def msssim(sr, gt, window_size=11, normalize=False):
    """sr, gt: NHWC fp32 device tensors in [0, 1] (value range 1).  Returns the scalar of msssim() (:71-98), including its
    `prod(pow1[:-1] * pow2[-1])` combination."""
    B, H, W, C = sr.shape
    windows, h, w = [], H, W
    for _ in range(5):
        windows.append(gaussian(min(window_size, h, w)))     # real_size = min(window_size, height, width), :40-42
        h, w = h // 2, w // 2
    sims, css = A.msssim_terms(sr, gt, windows)
    weights = _WEIGHTS.get(sr.device)
    if weights is None:   # uploaded once per device (a pageable H2D copy is not allowed inside a captured step)
        weights = _WEIGHTS[sr.device] = torch.tensor(MSSSIM_WEIGHTS, dtype=torch.float32, device=sr.device)
    if normalize:                                             # :86-88
        sims, css = (sims + 1) / 2, (css + 1) / 2
    pow1, pow2 = css ** weights, sims ** weights
    x = pow1[:-1] * pow2[-1]                                  # :92 torch.prod(...), written out: prod's backward inspects
    return x[0] * x[1] * x[2] * x[3]                          # its input for zeros on the host (a sync; not graph-capturable)


class PerceptualNetwork(HipModule):
    """vgg16.features[:16] with taps after relu1_2 / relu2_2 / relu3_3 and the mean of the three feature MSEs
    (losses.py:12-40).  Parameter names are torchvision's (`vgg_model.<index>.weight`), so the pretrained file the reference
    downloads (`vgg16(pretrained=True)`) loads unchanged; offline the weights are whatever the caller initialises."""

    TAPS = (3, 8, 15)

    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in (64, 64, "M", 128, 128, "M", 256, 256, 256):     # torchvision cfg 'D', first 16 modules
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.vgg_model = nn.Sequential(*layers)
        for p in self.vgg_model.parameters():
            p.requires_grad = False

    def output_features(self, x):
        """x: NHWC fp32 image -> [relu1_2, relu2_2, relu3_3] as NHWC bf16."""
        feats, h, i, mods = [], x, 0, list(self.vgg_model)
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Conv2d):                              # conv + the ReLU that follows it, fused
                if m.in_channels == 3:
                    h = A.conv2d_small(h, m.weight, m.bias, layout="nhwc", act="relu")
                else:
                    h = A.conv2d(h, m.weight, m.bias, act="relu")
                i += 2
            else:
                h = A.maxpool2(h)
                i += 1
            if i - 1 in self.TAPS:
                feats.append(h)
        return feats

    def forward(self, dehaze, gt):
        f_sr = self.output_features(dehaze)
        with torch.no_grad():
            f_gt = self.output_features(gt)
        losses = [A.mse_loss(a, b) for a, b in zip(f_sr, f_gt)]
        return sum(losses) / len(losses)


# torchvision's vgg16 cfg 'D': the conv indices of `features` per LPIPS slice (taps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
LPIPS_SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
LPIPS_CHANNELS = (64, 128, 256, 512, 512)
LPIPS_SHIFT = (-.030, -.088, -.188)      # ScalingLayer (lpips / taming): applied to 2 x - 1
LPIPS_SCALE = (.458, .448, .450)


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(LPIPS_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(LPIPS_SCALE)[None, :, None, None])


class _NetLinLayer(nn.Module):
    """`lin`: a 1x1 conv without bias behind a Dropout (the identity in eval mode)."""

    def __init__(self, chn):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn, 1, 1, stride=1, padding=0, bias=False))


class LPIPSLoss(HipModule):
    """LPIPS (Zhang et al. 2018) on VGG16, the perceptual part of taming's VQLPIPSWithDiscriminator that VQModel.training_step calls as
    `self.loss` (VQModel_arch.py:110-160), differentiable for the reconstruction: the scaling layer, vgg16.features down to relu5_3 on
    the taped HIP convs as PerceptualNetwork runs them, and per tap the LPIPS head (autograd.lpips_head, csrc/lpips_ops.hip) on the
    16-bit NHWC feature maps.  Module layout and parameter names are taming's / the lpips package's (`scaling_layer.shift|scale`,
    `net.slice<k>.<torchvision index>.weight|bias`, `lin<k>.model.1.weight`), so the published files load unchanged (load_vgg16).
    Every parameter is frozen and the module stays in eval mode.  One deviation from autograd of the published forward: a pixel of a
    reconstruction-side feature map that is all zero gets gradient 0 from the head (autograd: NaN)."""

    def __init__(self):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = nn.Module()
        cin, nxt = 3, 0
        for k, (idx, cout) in enumerate(zip(LPIPS_SLICES, LPIPS_CHANNELS)):
            sl = nn.Sequential()
            if k:
                sl.add_module(str(nxt), nn.MaxPool2d(kernel_size=2, stride=2))
            for i in idx:
                sl.add_module(str(i), nn.Conv2d(cin, cout, 3, padding=1))
                sl.add_module(str(i + 1), nn.ReLU(inplace=True))
                cin = cout
            nxt = idx[-1] + 2
            setattr(self.net, "slice%d" % (k + 1), sl)
            setattr(self, "lin%d" % k, _NetLinLayer(cout))
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def train(self, mode=True):
        return super().train(False)       # a frozen loss network: eval mode whatever the caller's .train() says

    def _frozen_packs(self):
        """The trunk's filters are packed ONCE per precision and direction (ops.FrozenPacks), not once per step."""
        cache = self.__dict__.setdefault("_hip_cache", {})
        if "frozen" not in cache:
            cache["frozen"] = ops.FrozenPacks(list(self.net.parameters()))
        return cache["frozen"]

    def _affine(self):
        def build():      # (y - shift) / scale on y = 2 x - 1 as x * mul + add, the two vectors formed in fp64
            shift, scale = self.scaling_layer.shift.detach().double().reshape(-1), self.scaling_layer.scale.detach().double().reshape(-1)
            return (2.0 / scale).float().contiguous(), ((-1.0 - shift) / scale).float().contiguous()
        return self._packed("affine", build)

    def _head(self, k):
        return self._packed(("lin", k), lambda: getattr(self, "lin%d" % k).model[1].weight.detach().float().reshape(-1).contiguous())

    def output_features(self, img):
        """img: NHWC fp32 in [0, 1] -> the five taps as 16-bit NHWC."""
        mul, add = self._affine()
        h, feats = A.image_affine(img, mul, add), []
        for k in range(5):
            for m in getattr(self.net, "slice%d" % (k + 1)):
                if isinstance(m, nn.Conv2d):                              # conv + the ReLU that follows it, fused
                    if m.in_channels == 3:
                        h = A.conv2d_small(h, m.weight, m.bias, layout="nhwc", act="relu")
                    else:
                        h = A.conv2d(h, m.weight, m.bias, act="relu")
                elif isinstance(m, nn.MaxPool2d):
                    h = A.maxpool2(h)
            feats.append(h)
        return feats

    def forward(self, xrec, x):
        """xrec, x: NHWC fp32 in [0, 1]; only xrec is differentiated.  Returns the batch mean of the per-image sum of the five taps:
        `mean(p_loss)` of taming's nll_loss (the caller multiplies by perceptual_weight)."""
        self._frozen_packs()
        fa = self.output_features(xrec)
        with torch.no_grad():
            fb = self.output_features(x)
        total = None
        for k, (a, b) in enumerate(zip(fa, fb)):
            v = A.lpips_head(a, b, self._head(k))
            total = v if total is None else total + v
        return total.mean()


VGG19_RELU3_4 = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256)      # torchvision cfg 'E' down to relu3_4: convs 0 2 5 7 10 12 14 16, pools 4 9
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # vgg_arch.py:134-137, for an image in [0, 1]


class SemanticTarget(HipModule):
    """The target of stage 1's semantic guidance term: VGG19 down to relu3_4 on the input image, as the reference's
    VGGFeatureExtractor(['relu3_4']) that VQModel builds (VQModel_arch.py:56-61) computes it with use_input_norm=True: (x - mean) / std with
    ImageNet's statistics on a [0, 1] image (vgg_arch.py:134-152), then `features[:18]` of torchvision's vgg19 -- two 2x2 pools, so the map is
    H/4 x W/4 with 256 channels: the f4 latent's size.  `features.<torchvision index>.weight|bias` are the parameter names, so
    vgg19-dcbb9e9d.pth loads unchanged (load_vgg19).  The trunk runs on the taped HIP convs used as plain forwards; every parameter is
    frozen and the module stays in eval mode; the filters are packed once per precision (ops.FrozenPacks)."""

    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in VGG19_RELU3_4:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        self.register_buffer("mean", torch.tensor(IMAGENET_MEAN)[None, :, None, None])
        self.register_buffer("std", torch.tensor(IMAGENET_STD)[None, :, None, None])
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def train(self, mode=True):
        return super().train(False)       # a frozen loss network: eval mode whatever the caller's .train() says

    def _frozen_packs(self):
        cache = self.__dict__.setdefault("_hip_cache", {})
        if "frozen" not in cache:
            cache["frozen"] = ops.FrozenPacks(list(self.features.parameters()))
        return cache["frozen"]

    def _affine(self):
        def build():      # (x - mean) / std as x * mul + add, the two vectors formed in fp64
            mean, std = self.mean.detach().double().reshape(-1), self.std.detach().double().reshape(-1)
            return (1.0 / std).float().contiguous(), (-mean / std).float().contiguous()
        return self._packed("affine", build)

    def forward(self, img):
        """img: NHWC fp32 in [0, 1], H and W multiples of 4 -> relu3_4 as 16-bit NHWC [B, H/4, W/4, 256], no tape."""
        B, H, W, C = img.shape
        if C != 3 or H % 4 or W % 4:
            raise ValueError("SemanticTarget: an NHWC 3-channel image with H and W multiples of 4 is asked (two 2x2 pools down to the "
                             "latent's size); got %s" % (tuple(img.shape),))
        self._frozen_packs()
        with torch.no_grad():
            mul, add = self._affine()
            h = A.image_affine(img.float().contiguous(), mul, add)
            for m in self.features:
                if isinstance(m, nn.Conv2d):                              # conv + the ReLU that follows it, fused
                    if m.in_channels == 3:
                        h = A.conv2d_small(h, m.weight, m.bias, layout="nhwc", act="relu")
                    else:
                        h = A.conv2d(h, m.weight, m.bias, act="relu")
                elif isinstance(m, nn.MaxPool2d):
                    h = A.maxpool2(h)
        return h


_BACKBONE_KEY = re.compile(r"^(?:features|vgg_model|net\.slice[1-5])\.(\d+)\.(weight|bias)$")


def _state_dict_of(file):
    sd = torch.load(file, map_location="cpu", weights_only=True) if isinstance(file, (str, bytes, os.PathLike)) else file
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError("%r does not hold a plain state dict of tensors" % (file,))
    return sd


def load_vgg16(module, vgg16_file, heads_file=None):
    """The one strict loader of the VGG16 loss networks: fills a PerceptualNetwork or an LPIPSLoss from files (paths, or state dicts).
    vgg16_file: the backbone under torchvision's keys (`features.N.*`), PerceptualNetwork's (`vgg_model.N.*`) or LPIPS's
    (`net.sliceK.N.*`); keys the target has no use for (the classifier, deeper convs) are ignored.  heads_file: taming's / the lpips
    package's `vgg.pth` (`linK.model.1.weight`), needed by an LPIPSLoss and refused by a PerceptualNetwork.  Every backbone and head
    tensor of the target must be found with its shape, else ValueError names the missing / mismatched keys: nothing is left at its
    initialisation silently.  Returns the list of the target's keys that were loaded."""
    if vgg16_file is None:
        raise ValueError("load_vgg16: the VGG16 backbone file is required (a heads file alone loads nothing the heads could read)")
    want_heads = [n for n, _ in module.named_parameters() if n.startswith("lin")]
    if heads_file is not None and not want_heads:
        raise ValueError("load_vgg16: %s has no LPIPS heads; a heads file makes no sense for it" % type(module).__name__)
    src = {}
    for key, v in _state_dict_of(vgg16_file).items():
        m = _BACKBONE_KEY.match(key)
        if m:
            src[(int(m.group(1)), m.group(2))] = (key, v)
    heads = _state_dict_of(heads_file) if heads_file is not None else {}
    targets = dict(module.named_parameters())
    plan, missing, wrong = [], [], []
    for name, p in targets.items():
        m = _BACKBONE_KEY.match(name)
        if m:
            hit = src.get((int(m.group(1)), m.group(2)))
            found = None if hit is None else hit[1]
            shown = "features.%s.%s (as %s)" % (m.group(1), m.group(2), name)
        else:
            found = heads.get(name)
            shown = name
        if found is None:
            missing.append(shown)
        elif tuple(found.shape) != tuple(p.shape):
            wrong.append("%s: %s in the file, %s expected" % (shown, tuple(found.shape), tuple(p.shape)))
        else:
            plan.append((name, p, found))
    if missing or wrong:
        raise ValueError("load_vgg16(%s): missing %s; wrong shape %s" % (type(module).__name__, missing or "none", wrong or "none"))
    with torch.no_grad():
        for _, p, v in plan:
            p.copy_(v.to(p.dtype))
    if hasattr(module, "invalidate"):
        module.invalidate()
    return [name for name, _, _ in plan]


def _vgg19_conv_names():
    """{'convB_I': torchvision index} of vgg19.features, the names the reference's extractor gives its layers (vgg_arch.py NAMES['vgg19'])."""
    names, idx, block, conv = {}, 0, 1, 1
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"):     # cfg 'E'
        if v == "M":
            idx, block, conv = idx + 1, block + 1, 1
        else:
            names["conv%d_%d" % (block, conv)] = idx
            idx, conv = idx + 2, conv + 1
    return names


_VGG_NET_KEY = re.compile(r"^vgg_net\.(conv\d_\d)\.(weight|bias)$")
_FEATURES_KEY = re.compile(r"^features\.(\d+)\.(weight|bias)$")


def load_vgg19(module, vgg19_file):
    """The strict loader of a SemanticTarget, in the manner of load_vgg16: fills it from a file (a path, or a state dict) under torchvision's
    keys (`features.N.weight|bias`, what vgg19-dcbb9e9d.pth holds) or the reference extractor's (`vgg_net.conv3_4.weight`, ...).  The
    classifier and the deeper convs are ignored.  Every tensor of the trunk must be found with its shape, else ValueError names the
    missing / mismatched keys (a VGG16 file has no conv at `features.16`: its index 16 is a pool).  Returns the list of the keys loaded."""
    if vgg19_file is None:
        raise ValueError("load_vgg19: the VGG19 file is required")
    by_name, src = _vgg19_conv_names(), {}
    for key, v in _state_dict_of(vgg19_file).items():
        m, n = _FEATURES_KEY.match(key), _VGG_NET_KEY.match(key)
        if m:
            src[(int(m.group(1)), m.group(2))] = v
        elif n and n.group(1) in by_name:
            src[(by_name[n.group(1)], n.group(2))] = v
    plan, missing, wrong = [], [], []
    for name, p in module.named_parameters():
        m = _FEATURES_KEY.match(name)
        found = src.get((int(m.group(1)), m.group(2)))
        if found is None:
            missing.append(name)
        elif tuple(found.shape) != tuple(p.shape):
            wrong.append("%s: %s in the file, %s expected" % (name, tuple(found.shape), tuple(p.shape)))
        else:
            plan.append((name, p, found))
    if missing or wrong:
        raise ValueError("load_vgg19(%s): missing %s; wrong shape %s" % (type(module).__name__, missing or "none", wrong or "none"))
    with torch.no_grad():
        for _, p, v in plan:
            p.copy_(v.to(p.dtype))
    module.invalidate()
    return [name for name, _, _ in plan]
