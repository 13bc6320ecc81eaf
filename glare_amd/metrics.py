"""Evaluation metrics of the reference's dataset loops on the device: LPIPS (AlexNet) as `Measure.lpips` computes it
(code/Measure.py:17-30, called from infer_dataset_lol.py:153 / infer_dataset_lolv2-real.py:150 / test_stage3.py:205).  PSNR and the
MATLAB-style SSIM (utils2.py:32-36, 42-89) live in glare_amd.harness.

The reference builds `lpips.LPIPS(net='alex')` from the third-party `lpips` package (Zhang et al., "The Unreasonable Effectiveness of Deep
Features as a Perceptual Metric", CVPR 2018; PyPI lpips 0.1.x -- unpinned by the reference, absent from this image together with the
torchvision AlexNet weights and the package's linear heads it downloads).  `LPIPS` below mirrors that module's SURFACE -- constructor
default, `forward(in0, in1, normalize=False)` -> [N, 1, 1, 1], and its state-dict keys (`scaling_layer.shift / .scale`,
`net.slice{1..5}.{0,3,6,8,10}.weight / .bias` = torchvision alexnet.features indices, `lin{0..4}.model.1.weight` and their `lins.{k}` aliases)
so that a checkpoint saved from the package loads with `load_state_dict`; offline the weights are whatever the caller initialises
(glare_amd.synthetic.seeded_init_ in the tests).  Compute: csrc/metrics.hip through the C ABI (fp32 as the package; no CPU path).
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .modules._base import HipModule

ALEX_CHNS = (64, 192, 384, 256, 256)                                    # lpips: self.chns for net='alex'
# (index in torchvision's alexnet.features, cin, cout, kernel, stride, padding) of the conv that ENDS each slice (ReLU follows; slices
# 2 and 3 start with MaxPool2d(3, 2))
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))


def conv2d_direct(x, weight, bias=None, stride=1, padding=0, relu=False, in_shift=None, in_scale=None):
    """fp32 NCHW direct convolution (glare_conv2d_direct_f32): any kernel <= 16, stride, zero padding; optional per-channel input
    affine (x - shift) / scale applied before the padding."""
    _lib.require_cuda(x, weight, bias, in_shift, in_scale)
    x, weight = x.float().contiguous(), weight.detach().float().contiguous()
    B, Cin, H, W = x.shape
    Cout, cin2, k, k2 = weight.shape
    assert cin2 == Cin and k == k2
    OH, OW = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    out = torch.empty(B, Cout, OH, OW, dtype=torch.float32, device=x.device)
    b = None if bias is None else bias.detach().float().contiguous()
    sh = None if in_shift is None else in_shift.detach().float().reshape(-1).contiguous()
    sc = None if in_scale is None else in_scale.detach().float().reshape(-1).contiguous()
    _lib.check(_lib.main_lib().glare_conv2d_direct_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(b), _lib.ptr(out), B, Cin, H, W, Cout, k,
                                                       stride, padding, int(relu), _lib.ptr(sh), _lib.ptr(sc),
                                                       _lib.stream_handle()), "glare_conv2d_direct_f32")
    return out


def maxpool2d(x, kernel_size, stride):
    _lib.require_cuda(x)
    x = x.float().contiguous()
    B, C, H, W = x.shape
    out = torch.empty(B, C, (H - kernel_size) // stride + 1, (W - kernel_size) // stride + 1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.main_lib().glare_maxpool2d_f32(_lib.ptr(x), _lib.ptr(out), B, C, H, W, kernel_size, stride,
                                                   _lib.stream_handle()), "glare_maxpool2d_f32")
    return out


class ScalingLayer(nn.Module):
    """lpips.ScalingLayer: (inp - shift) / scale with the package's constants (applied inside the first conv's loader here)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([.458, .448, .450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """lpips.NetLinLayer: Dropout (identity in eval) + 1x1 conv C -> 1 without bias; the conv is `model.1`."""

    def __init__(self, chn_in, chn_out=1, use_dropout=True):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)


class _AlexSlices(nn.Module):
    """lpips.pretrained_networks.alexnet: torchvision's alexnet.features cut into five slices, modules keyed by their index there."""

    def __init__(self):
        super().__init__()
        for s, (idx, cin, cout, k, st, pd) in enumerate(ALEX_CONVS):
            seq = nn.Sequential()
            if s in (1, 2):
                seq.add_module(str(idx - 1), nn.MaxPool2d(kernel_size=3, stride=2))
            seq.add_module(str(idx), nn.Conv2d(cin, cout, kernel_size=k, stride=st, padding=pd))
            seq.add_module(str(idx + 1), nn.ReLU(inplace=True))
            setattr(self, "slice%d" % (s + 1), seq)


class LPIPS(HipModule):
    """`lpips.LPIPS(net='alex', version='0.1', lpips=True, spatial=False)` on the HIP kernels."""

    def __init__(self, net="alex", version="0.1", use_dropout=True):
        super().__init__()
        if net not in ("alex", "alexnet") or version != "0.1":
            raise NotImplementedError("glare_amd.metrics.LPIPS implements net='alex', version='0.1' (Measure.py:20)")
        self.pnet_type, self.version, self.chns, self.L = net, version, list(ALEX_CHNS), len(ALEX_CHNS)
        self.scaling_layer = ScalingLayer()
        self.net = _AlexSlices()
        for k, c in enumerate(ALEX_CHNS):
            setattr(self, "lin%d" % k, NetLinLayer(c, use_dropout=use_dropout))
        self.lins = nn.ModuleList([getattr(self, "lin%d" % k) for k in range(self.L)])     # the package registers both names
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def features(self, x):
        """The five ReLU taps of one batch (fp32 NCHW in [-1, 1] after `normalize`)."""
        feats, h = [], x
        for s, (idx, cin, cout, k, st, pd) in enumerate(ALEX_CONVS):
            conv = getattr(getattr(self.net, "slice%d" % (s + 1)), str(idx))
            if s in (1, 2):
                h = maxpool2d(h, 3, 2)
            if s == 0:
                h = conv2d_direct(h, conv.weight, conv.bias, st, pd, relu=True, in_shift=self.scaling_layer.shift, in_scale=self.scaling_layer.scale)
            else:
                h = conv2d_direct(h, conv.weight, conv.bias, st, pd, relu=True)
            feats.append(h)
        return feats

    @torch.no_grad()
    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        _lib.require_cuda(in0, in1)
        if normalize:                      # images in [0, 1] -> [-1, 1]
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        f0, f1 = self.features(in0.float()), self.features(in1.float())
        B = in0.shape[0]
        lib = _lib.main_lib()
        total = torch.empty(B, dtype=torch.float64, device=in0.device)
        per_layer = []
        for k in range(self.L):
            a, b = f0[k], f1[k]
            C, HW = a.shape[1], a.shape[2] * a.shape[3]
            nws = lib.glare_lpips_tap_workspace_bytes(B, HW)
            ws = torch.empty(nws, dtype=torch.uint8, device=a.device)
            lin = self.lins[k].model[-1].weight.detach().float().reshape(-1).contiguous()
            dst = torch.empty(B, dtype=torch.float64, device=a.device) if retPerLayer else total
            _lib.check(lib.glare_lpips_tap_f32(_lib.ptr(a), _lib.ptr(b), _lib.ptr(lin), B, C, HW, 1e-10, int(k > 0 and not retPerLayer),
                                               _lib.ptr(dst), _lib.ptr(ws), nws, _lib.stream_handle()), "glare_lpips_tap_f32")
            if retPerLayer:
                per_layer.append(dst.float().view(B, 1, 1, 1))
        if retPerLayer:
            val = sum(per_layer)
            return val, per_layer
        return total.float().view(B, 1, 1, 1)


def build_lpips_alex(weights=None, device=None):
    """The LPIPS-alex metric net on `device`: from `weights`, a state dict saved from `lpips.LPIPS(net='alex')`, or -- its AlexNet and
    linear heads cannot be downloaded here -- name-seeded, so that the column only exercises the path."""
    from .synthetic import seeded_init_

    net = LPIPS(net="alex")
    if weights:
        net.load_state_dict(torch.load(weights, map_location="cpu"), strict=False)   # the package's own files hold the heads only
    else:
        seeded_init_(net, 7)
        with torch.no_grad():
            for lin in net.lins:                  # the package's trained heads are non-negative: keep the stand-in a valid distance
                lin.model[-1].weight.abs_()
    return net.to(device)


def to_lpips_input(imgs_u8):
    """Measure.t (Measure.py:48-64): uint8 HWC image(s) on the device -> fp32 NCHW in [-1, 1] (x / 127.5 - 1)."""
    if imgs_u8.dim() == 3:
        imgs_u8 = imgs_u8[None]
    assert imgs_u8.dtype == torch.uint8 and imgs_u8.shape[-1] == 3
    return imgs_u8.permute(0, 3, 1, 2).float() / 127.5 - 1


class CodebookUsage:
    """Running use of the codebook over a split (basicsr/active_codebook.py's count; the perplexity of quantize.py:83-85 over every token
    seen): `update(idx, groups)` adds one batch's indices to an int64 [n_codes] total on the device -- kernel launches only, no host
    synchronisation -- and returns that batch's per-group counts; `stats()` reads the totals back."""

    def __init__(self, n_codes, device):
        self.n_codes = int(n_codes)
        self._total = torch.zeros(self.n_codes, dtype=torch.int64, device=device)
        self._oor = torch.zeros((), dtype=torch.int64, device=device)

    def update(self, idx, groups=1):
        """-> (counts int64 [groups, n_codes], out_of_range int64 [groups]) of this batch (device tensors)."""
        from . import ops

        counts, oor, _ = ops.vq_usage(idx, self.n_codes, groups, total=self._total)
        self._oor += oor.sum()
        return counts, oor

    def discard(self, counts_row):
        """Takes one group's counts (a row update() returned) out of the total again: an image that is scored a second time."""
        self._total -= counts_row

    def counts(self):
        """The int64 [n_codes] total (the device tensor itself)."""
        return self._total

    def reset(self):
        self._total.zero_()
        self._oor.zero_()

    def stats(self):
        from . import ops

        tokens, active, _, perplexity = ops.vq_usage_stats(self._total)
        return usage_block(int(tokens), int(active), float(perplexity), self.n_codes, int(self._oor))


def usage_block(tokens, active, perplexity, n_codes, out_of_range=None):
    """The `codebook` block of a record: host numbers."""
    block = {"tokens": int(tokens), "active": int(active), "active_fraction": int(active) / int(n_codes), "perplexity": float(perplexity)}
    if out_of_range is not None:
        block["out_of_range"] = int(out_of_range)
    return block


def usage_block_host(counts):
    """usage_block of a host int64 [K] histogram, in float64 (a resumed sweep reads `<name>.codes.npy` back; no device involved)."""
    counts = np.asarray(counts, dtype=np.int64)
    n = int(counts.sum())
    p = counts[counts > 0].astype(np.float64) / max(n, 1)
    return usage_block(n, int((counts > 0).sum()), float(np.exp(-np.sum(p * np.log(p + 1e-10)))), counts.size)


# ---- NIQE: the no-reference score of unpaired results ------------------------------------------------------------------------------
# Mittal, Soundararajan, Bovik, "Making a 'Completely Blind' Image Quality Analyzer" (IEEE SPL 2013) as basicsr's calculate_niqe evaluates
# it -- the number the paper reports on MEF / LIME / DICM / NPE / VV (driver: defor_cuda_ext/basicsr/metrics/calculate_niqe.py, called with
# crop_border = 0, convert_to = 'y').  The pixel work runs on the device (csrc/niqe.hip: luma, the normalised image n at two scales, the
# half-size filter, per-block moments of n and of its four neighbour products); the host turns n_blocks x 25 fp64 moments per scale into
# the 36 features per block and the score, in fp64 numpy.  The pristine model is the user's file (basicsr's niqe_pris_params.npz), as
# the VGG weights are.  DESIGN.md "NIQE" says what is pinned against what.
NIQE_BLOCK = _lib.constants()["GLARE_NIQE_BLOCK"]
_NIQE_SHAPES = (("mu_pris_param", ((36,), (1, 36))), ("cov_pris_param", ((36, 36),)), ("gaussian_window", ((7, 7),)))
_NIQE_TABLE = None


def _niqe_params(arrays, where):
    """The three arrays of a pristine model, checked by name and shape -> fp64 dict (mu flattened to [36])."""
    out = {}
    for key, shapes in _NIQE_SHAPES:
        if key not in arrays:
            raise ValueError("%s: no array %r (a NIQE pristine model holds %s)" % (where, key, ", ".join(k for k, _ in _NIQE_SHAPES)))
        a = np.asarray(arrays[key])
        if a.shape not in shapes or not np.issubdtype(a.dtype, np.number) or np.iscomplexobj(a):
            raise ValueError("%s: %s has shape %s and dtype %s, expected a real array of shape %s"
                             % (where, key, tuple(a.shape), a.dtype, " or ".join(str(s) for s in shapes)))
        a = a.astype(np.float64)
        if not np.isfinite(a).all():
            raise ValueError("%s: %s holds inf or NaN" % (where, key))
        out[key] = a.reshape(shapes[0])
    return out


def load_niqe_params(path):
    """The pristine model of a `.npz` file: mu_pris_param (36,) or (1, 36), cov_pris_param (36, 36), gaussian_window (7, 7).  A file
    that lacks one of them, or holds it in another shape, is refused with the array's name."""
    with np.load(path, allow_pickle=False) as f:
        return _niqe_params({k: f[k] for k in f.files}, str(path))


def _niqe_table():
    """(grid g = 0.2, 0.201, ..., 10.000; rho(g) = Gamma(2/g)^2 / (Gamma(1/g) Gamma(3/g))), rho increasing."""
    global _NIQE_TABLE
    if _NIQE_TABLE is None:
        import math

        g = 0.2 + 0.001 * np.arange(9801)
        rho = np.array([math.exp(2 * math.lgamma(2 / x) - math.lgamma(1 / x) - math.lgamma(3 / x)) for x in g])
        assert np.all(np.diff(rho) > 0)          # what lets the nearest grid point be found by bisection
        lg = np.array([[math.lgamma(1 / x), math.lgamma(2 / x), math.lgamma(3 / x)] for x in g])
        _NIQE_TABLE = (g, rho, lg)
    return _NIQE_TABLE


def niqe_grid_index(R):
    """argmin_k (rho_k - R)^2 over the grid, the first on ties, for an array of R; a NaN or an infinity selects index 0, as numpy's
    argmin of a row of equal values does.  rho increases, so the minimum is one of the two grid points around R."""
    _, rho, _ = _niqe_table()
    R = np.asarray(R, dtype=np.float64)
    hi = np.clip(np.searchsorted(rho, R), 0, rho.size - 1)
    lo = np.clip(hi - 1, 0, rho.size - 1)
    with np.errstate(invalid="ignore"):
        k = np.where((rho[lo] - R) ** 2 <= (rho[hi] - R) ** 2, lo, hi)
    return np.where(np.isfinite(R), k, 0)


def niqe_features(moments, count):
    """Block moments of one scale [..., 5, 5] (glare_niqe_block_moments_f32: per map count(v<0), count(v>0), sum_{v<0} v^2, sum_{v>0} v^2,
    sum |v|) of blocks of `count` elements -> ([..., 18] features, [..., 5] grid indices).  Per map the asymmetric generalised Gaussian
    fit by moment matching: alpha from the grid, beta_l / beta_r from the one-sided deviations; [alpha, (beta_l + beta_r) / 2] for n itself
    and [alpha, (beta_r - beta_l) Gamma(2/alpha) / Gamma(1/alpha), beta_l, beta_r] for each product.  A side without a value gives NaN."""
    g, _, lg = _niqe_table()
    m = np.asarray(moments, dtype=np.float64)
    cn, cp, sn, sp, sa = (m[..., i] for i in range(5))
    with np.errstate(all="ignore"):
        left, right = np.sqrt(sn / cn), np.sqrt(sp / cp)
        gamma = left / right
        rhat = (sa / count) ** 2 / ((sn + sp) / count)
        k = niqe_grid_index(rhat * (gamma ** 3 + 1) * (gamma + 1) / (gamma ** 2 + 1) ** 2)
        alpha = g[k]
        scale = np.sqrt(np.exp(lg[k, 0] - lg[k, 2]))
        bl, br = left * scale, right * scale
        mean = (br - bl) * np.exp(lg[k, 1] - lg[k, 0])
    cols = [alpha[..., 0], (bl[..., 0] + br[..., 0]) / 2]
    for j in range(1, 5):
        cols += [alpha[..., j], mean[..., j], bl[..., j], br[..., j]]
    return np.stack(cols, axis=-1), k


def niqe_score(features36, params):
    """[n_blocks, 36] features -> (score, None) or (None, reason): sqrt(d pinv((cov_pris + cov_d) / 2) d^T), d = mu_pris - nanmean(features),
    cov_d over the rows without NaN (n - 1 divisor); fewer than 2 such rows has no score."""
    f = np.asarray(features36, dtype=np.float64)
    good = f[~np.isnan(f).any(axis=1)]
    if good.shape[0] < 2:
        return None, "fewer than 2 blocks with finite features (%d of %d)" % (good.shape[0], f.shape[0])
    with np.errstate(all="ignore"):
        mu_d = np.nanmean(f, axis=0)
    d = params["mu_pris_param"].reshape(36) - mu_d
    inv = np.linalg.pinv((params["cov_pris_param"] + np.cov(good, rowvar=False)) / 2)
    return float(np.sqrt(d @ inv @ d)), None


def niqe_from_moments(moments1, moments2, params, block=NIQE_BLOCK):
    """The host part: the block moments of the two scales of ONE image ([n_blocks, 5, 5] each, blocks of block^2 and (block / 2)^2
    elements) -> (score, None) or (None, reason)."""
    f1, _ = niqe_features(np.asarray(moments1).reshape(-1, 5, 5), block * block)
    f2, _ = niqe_features(np.asarray(moments2).reshape(-1, 5, 5), (block // 2) * (block // 2))
    return niqe_score(np.concatenate([f1, f2], axis=1), params)


def niqe_window_sums(window):
    """(s0, 1 - s0) of the fp64 window, as glare_niqe_mscn_f32 takes them.  A window normalised in fp64 sums to 1 only to within its own
    rounding (49 weights of 2^-53 relative each): a sum within 2^-50 of 1 IS 1, and a constant image then normalises to exactly 0."""
    import math

    s0 = math.fsum(np.asarray(window, dtype=np.float64).reshape(-1).tolist())
    oms0 = 1.0 - s0
    return (1.0, 0.0) if abs(oms0) <= 2.0 ** -50 else (s0, oms0)


def niqe_luma(imgs_u8):
    """uint8 RGB [B,h,w,3] on the device -> fp32 [B,H,W]: the integer luma of the top-left whole 96 x 96 blocks."""
    _lib.require_cuda(imgs_u8)
    assert imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4 and imgs_u8.shape[-1] == 3, (imgs_u8.dtype, tuple(imgs_u8.shape))
    imgs_u8 = imgs_u8.contiguous()
    B, h, w, _ = imgs_u8.shape
    y = torch.empty(B, h // NIQE_BLOCK * NIQE_BLOCK, w // NIQE_BLOCK * NIQE_BLOCK, dtype=torch.float32, device=imgs_u8.device)
    _lib.check(_lib.main_lib().glare_niqe_luma_u8(_lib.ptr(imgs_u8), B, h, w, _lib.ptr(y), _lib.stream_handle()), "glare_niqe_luma_u8")
    return y


def niqe_mscn(y, window):
    """fp32 [B,H,W] -> n = (y - mu) / (sigma + 1) with the 7 x 7 fp64 `window` (numpy)."""
    _lib.require_cuda(y)
    y = y.float().contiguous()
    B, H, W = y.shape
    s0, oms0 = niqe_window_sums(window)
    n = torch.empty_like(y)
    _lib.check(_lib.main_lib().glare_niqe_mscn_f32(_lib.ptr(y), B, H, W, _lib.host_f32(np.asarray(window).reshape(-1), 49), s0, oms0,
                                                   _lib.ptr(n), _lib.stream_handle()), "glare_niqe_mscn_f32")
    return n


def niqe_block_moments(n, bh=NIQE_BLOCK, bw=NIQE_BLOCK):
    """fp32 [B,H,W] -> fp64 [B, W / bw, H / bh, 5, 5] (blocks column-major; maps; moments)."""
    _lib.require_cuda(n)
    n = n.float().contiguous()
    B, H, W = n.shape
    out = torch.empty(B, W // max(bw, 1), H // max(bh, 1), 5, 5, dtype=torch.float64, device=n.device)
    _lib.check(_lib.main_lib().glare_niqe_block_moments_f32(_lib.ptr(n), B, H, W, bh, bw, _lib.ptr(out), _lib.stream_handle()),
               "glare_niqe_block_moments_f32")
    return out


def niqe_halve(y):
    """fp32 [B,H,W], H and W even and >= 4 -> [B, H / 2, W / 2]: MATLAB's antialiased bicubic imresize(., 0.5)."""
    _lib.require_cuda(y)
    y = y.float().contiguous()
    B, H, W = y.shape
    out = torch.empty(B, H // 2, W // 2, dtype=torch.float32, device=y.device)
    _lib.check(_lib.main_lib().glare_niqe_halve_f32(_lib.ptr(y), B, H, W, _lib.ptr(out), _lib.stream_handle()), "glare_niqe_halve_f32")
    return out


def niqe_moments_device(imgs_u8, window):
    """uint8 [B,h,w,3] on the device, at least 2 whole blocks -> the block moments of both scales, host fp64 [B, n_blocks, 5, 5] each:
    six launches, and n_blocks x 25 numbers per scale and image cross PCIe."""
    y = niqe_luma(imgs_u8)
    m1 = niqe_block_moments(niqe_mscn(y, window))
    m2 = niqe_block_moments(niqe_mscn(niqe_halve(y), window), NIQE_BLOCK // 2, NIQE_BLOCK // 2)
    B = y.shape[0]
    return m1.reshape(B, -1, 5, 5).cpu().numpy(), m2.reshape(B, -1, 5, 5).cpu().numpy()


def niqe_scores(images_u8, params, device=None):
    """As niqe(), but -> a list of (score, None) or (None, reason)."""
    if not torch.cuda.is_available():
        raise NotImplementedError("glare_amd metrics run on MI355X only (HIP kernels, no CPU path)")
    params = _niqe_params(params, "params") if isinstance(params, dict) else load_niqe_params(params)
    device = device or torch.device("cuda", torch.cuda.current_device())
    if isinstance(images_u8, (torch.Tensor, np.ndarray)) and images_u8.ndim == 4:
        images_u8 = list(images_u8)
    imgs = [im if isinstance(im, torch.Tensor) else torch.from_numpy(im if im.flags.writeable and im.flags.c_contiguous else np.array(im))
            for im in images_u8]                      # an array read from a file is read-only: torch wants a writable one
    results, groups = [None] * len(imgs), {}
    for i, im in enumerate(imgs):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[-1] != 3:
            raise ValueError("niqe: image %d is %s %s, expected uint8 [h, w, 3]" % (i, im.dtype, tuple(im.shape)))
        h, w = int(im.shape[0]), int(im.shape[1])
        if (h // NIQE_BLOCK) * (w // NIQE_BLOCK) < 2:
            results[i] = (None, "%dx%d holds fewer than 2 whole %dx%d blocks" % (h, w, NIQE_BLOCK, NIQE_BLOCK))
        else:
            groups.setdefault((h, w), []).append(i)
    for idx in groups.values():
        m1, m2 = niqe_moments_device(torch.stack([imgs[i].to(device) for i in idx]), params["gaussian_window"])
        for j, i in enumerate(idx):
            results[i] = niqe_from_moments(m1[j], m2[j], params)
    return results


def niqe(images_u8, params):
    """NIQE of uint8 RGB images: a device or host tensor / array [B,h,w,3], or a list of [h,w,3] images of mixed sizes -> a list with a
    float per image, or None where an image has no score (fewer than 2 whole 96 x 96 blocks, or fewer than 2 blocks with finite
    features).  params: load_niqe_params(path), or a dict with the same three arrays.  Lower is better."""
    return [s for s, _ in niqe_scores(images_u8, params)]


def niqe_mean(scores):
    """Mean over the scored images (None left out); None when nothing was scored."""
    vals = [s for s in scores if s is not None]
    return float(np.mean(vals)) if vals else None


def main(argv=None):
    """python -m glare_amd.metrics niqe PATH... --params PARAMS.npz: scores existing files and folders (a folder: <dir>/*.* in natural
    order), e.g. another method's outputs, and prints one JSON line."""
    import argparse
    import json
    import os
    import time

    from . import enhance

    ap = argparse.ArgumentParser(prog="python -m glare_amd.metrics", description="No-reference scores of existing images.")
    sub = ap.add_subparsers(dest="metric", required=True)
    nq = sub.add_parser("niqe", help="NIQE (lower is better)")
    nq.add_argument("paths", nargs="+", help="image files and / or folders")
    nq.add_argument("--params", required=True, help="the pristine model: basicsr's niqe_pris_params.npz")
    args = ap.parse_args(argv)
    params = load_niqe_params(args.params)
    assert torch.cuda.is_available(), "glare_amd.metrics needs an MI355X: the HIP kernels are the only implementation"
    imgs, names, skipped = [], [], []
    for f in enhance.list_inputs(args.paths):
        img, why = enhance.read_image(f)
        if img is None:
            skipped.append({"name": os.path.basename(f), "reason": why})
        else:
            imgs.append(img)
            names.append(os.path.basename(f))
    t0 = time.perf_counter()
    scored = niqe_scores(imgs, params)        # ends in the copies of the moments to the host: synchronous
    secs = time.perf_counter() - t0
    res = {"images": [dict({"name": n, "size": [int(a.shape[0]), int(a.shape[1])], "niqe": s}, **({} if why is None else {"niqe_reason": why}))
                      for n, a, (s, why) in zip(names, imgs, scored)],
           "skipped": skipped, "niqe_mean": niqe_mean([s for s, _ in scored]), "scored": sum(s is not None for s, _ in scored),
           "niqe_seconds": round(secs, 4)}
    print(json.dumps(res))
    return res


class Measure:
    """Measure (Measure.py:17-30), the LPIPS leg: `lpips(imgA, imgB)` on uint8 HWC images (numpy or device tensors) -> float."""

    def __init__(self, net="alex", use_gpu=True, model=None):
        if not use_gpu:
            raise NotImplementedError("glare_amd metrics run on MI355X only (HIP kernels, no CPU path)")
        self.device = "cuda"
        self.model = (model if model is not None else LPIPS(net=net)).to(self.device)

    def lpips(self, imgA, imgB, model=None):
        tA, tB = (to_lpips_input(torch.as_tensor(np.ascontiguousarray(im) if isinstance(im, np.ndarray) else im).to(self.device)) for im in (imgA, imgB))
        return self.model.forward(tA, tB).item()


if __name__ == "__main__":
    main()
