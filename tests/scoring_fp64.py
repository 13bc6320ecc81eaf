"""The kernels behind every PSNR, SSIM and LPIPS the project prints -- csrc/harness.hip (paired and unpaired pre / post-processing, the "adjust"
protocol) and csrc/metrics.hip (the LPIPS convolution, pool and tap) -- restated in fp64 for test_gpu_scoring_edges.py, with their input
families.  A plain module like tolerances.py; held to independent references and shown sensitive on the CPU by test_vq_scoring_fp64_host.py.

Bounds are counted from the kernels' own expressions, U = 2^-24 one fp32 rounding, gamma(k) = k U / (1 - k U) k of them in a row; each count
stands next to the function that returns it.  Every function that takes `mutation` computes, under a name of MUTATIONS, what a subtly wrong
kernel would: the CPU test shows each one moves the expected result beyond the bound (or flips a byte), so the GPU comparison can see it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import loss_fp64

U = 2.0 ** -24
PAD = 20


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(v):
    """a Python number as the C `float` a kernel holds, back as a double"""
    return float(np.float32(v))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the network-output generator of the unpaired / adjust tests (test_gpu_evaluate.py imports it back) -------------------------------------
def output_and_gt(B, Hp, Wp, special=True):
    """fp32 [B,3,Hp,Wp] below 0, above 1, on k/255 and one ulp either side; special: NaN, +inf and -inf sprinkled in."""
    g = torch.Generator().manual_seed(Hp * Wp + B)
    x = torch.rand(B, 3, Hp, Wp, generator=g, dtype=torch.float64).mul(1.4).sub(0.2).float()
    k = torch.randint(0, 256, x.shape, generator=g).float() / 255
    sel = torch.rand(x.shape, generator=g)
    x = torch.where(sel < 0.3, k, x)
    x = torch.where((sel >= 0.3) & (sel < 0.4), torch.nextafter(k, torch.tensor(2.0)), x)
    x = torch.where((sel >= 0.4) & (sel < 0.5), torch.nextafter(k, torch.tensor(-1.0)), x)
    if special:
        flat = x.view(-1)
        spec = torch.randint(0, flat.numel(), (max(6, flat.numel() // 50),), generator=g)
        for j, i in enumerate(spec.tolist()):
            flat[i] = (float("nan"), float("inf"), float("-inf"))[j % 3]
    gt = torch.randint(0, 256, (B, Hp, Wp, 3), generator=g, dtype=torch.uint8)
    return x, gt


# ---- pre-processing: one expression of one byte, and an index map ----------------------------------------------------------------------------
def pre_table64():
    """fp64 log(max(fl32(v / 255) + fl32(1e-3), fl32(1e-3))) for v = 0 .. 255: the value pre_kernel, pre_pad_kernel and tile_gather_kernel share"""
    v = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float64)
    return np.log(np.maximum(v + f32(1e-3), f32(1e-3)))


def fold(i, n, mode, mutation=None):
    """source index of padded coordinate i (may be negative or beyond n): numpy 'reflect' folds with period 2n - 2, 'symmetric' with 2n"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    if mode == "symmetric":
        p = np.mod(i, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)
    per = 2 * n if mutation == "fold_period_2n" else 2 * n - 2
    p = np.mod(i, per)
    return np.where(p < n, p, per - p if mutation != "fold_period_2n" else 2 * n - 1 - p)


def pad_indices(n, before, after, mode):
    """the same map from numpy itself: np.pad of an index array"""
    return np.pad(np.arange(n), (before, after), mode)


def pre_expected(table32, img, ys, xs):
    """table[img[b, ys, xs, c]] as [B, 3, Hp, Wp]"""
    return np.ascontiguousarray(table32[img[:, ys][:, :, xs]].transpose(0, 3, 1, 2))


PAIRED_SHAPES = ((2, 2, 2), (3, 7, 33), (1, 21, 20), (1, 20, 21), (2, 3, 40))          # (B, H, W): pad 20 at the bottom and on the left
# (H, W, (top, bottom, left, right)): a side of one pixel; a pad longer than twice the side on each of the four sides in turn; all at once
PAD_CASES = ((1, 5, (3, 2, 1, 4)), (5, 1, (1, 4, 3, 2)), (1, 1, (2, 3, 4, 5)), (3, 4, (7, 0, 0, 0)), (3, 4, (0, 7, 0, 0)), (3, 4, (0, 0, 9, 0)),
             (3, 4, (0, 0, 0, 9)), (3, 4, (7, 8, 9, 10)), (2, 2, (5, 5, 5, 5)))


# ---- paired post-processing -----------------------------------------------------------------------------------------------------------------
GRAY32 = tuple(f32(w) for w in (0.114, 0.587, 0.299))          # the weights as post_crop_kernel holds them (0.114f ...), on channels 0, 1, 2
GRAY64 = (0.114, 0.587, 0.299)                                  # ... and as it applies them, in double, to the ground truth
POST_SHAPES = ((65, 5, 7), (2, 127, 129), (2, 128, 128), (2, 129, 128))          # (B, h, w): 16 383 / 16 384 / 16 512 pixels against a trip of 16 384


def post_crop(out, h, w, pad=PAD):
    """-> (clamped crop fp32 [B,h,w,3], a NaN kept; non-finite values inside the crop before the clamp, int [B])"""
    v = np.ascontiguousarray(np.asarray(out, dtype=np.float32)[:, :, :h, pad:pad + w].transpose(0, 2, 3, 1))
    with np.errstate(invalid="ignore"):
        r = np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)
    return r, (~np.isfinite(v)).reshape(v.shape[0], -1).sum(1)


def post_fp64(out, gt, h, w, pad=PAD, mutation=None):
    """postprocess_device with ground truth in fp64 -> dict(restored, bound, gain, psnr, psnr_bound, nonfinite).
    restored = clip(r gain), r the clamped crop, gain = sum gray(gt / 255) / sum gray(r).  Roundings of the kernels on |r gain|:
      post_crop_kernel   gray(r) = 0.114f r0 + 0.587f r1 + 0.299f r2: a product and two additions on the first term's path, all terms
                         non-negative -> 3 on the sum; the sums over pixels and the ratio are fp64
      post_gain_kernel   (float) of the ratio 1, r * gain 1; the clamps are 1-Lipschitz
    = gamma(5) |r gain|.  PSNR: the kernel's d = gt / 255 - r and its sums are fp64, so its error is the restored bound e carried through
    mse = mean d^2: (10 / ln 10) 2 mean(|d| e) / mse, plus the fp64 summation of n + 74 terms."""
    r, bad = post_crop(out, h, w, pad)
    B = r.shape[0]
    r64, g = r.astype(np.float64), np.asarray(gt).astype(np.float64)
    wr = GRAY32[::-1] if mutation == "gray_weights_bgr" else GRAY32
    wg = GRAY64[::-1] if mutation == "gray_weights_bgr" else GRAY64
    with np.errstate(invalid="ignore", divide="ignore"):
        sr = (wr[0] * r64[..., 0] + wr[1] * r64[..., 1] + wr[2] * r64[..., 2]).reshape(B, -1).sum(1)
        sg = (wg[0] * (g[..., 0] / 255.0) + wg[1] * (g[..., 1] / 255.0) + wg[2] * (g[..., 2] / 255.0)).reshape(B, -1).sum(1)
        gain = sg / sr
        raw = r64 * gain[:, None, None, None]
        restored = np.where(raw < 0, 0.0, np.where(raw > 1, 1.0, raw))
        bound = gamma(5) * np.abs(raw) + 1e-300
        d = g / 255.0 - restored
        n = d[0].size
        mse = (d * d).reshape(B, -1).mean(1)
        psnr = np.where(mse == 0, 100.0, 10.0 * np.log10(1.0 / mse))
        psnr_bound = (10.0 / math.log(10.0)) * (2.0 * (np.abs(d) * bound).reshape(B, -1).mean(1) / mse + (n + 74) * 2.0 ** -53)
    return dict(restored=restored, bound=bound, gain=gain, psnr=psnr, psnr_bound=psnr_bound, nonfinite=bad, crop=r)


def post_inputs(B, h, w, seed, below=5, right=3):
    """network output fp32 [B,3,h+below,w+20+right] around 0.45 +- 0.4 (values below 0 and above 1), uint8 ground truth [B,h,w,3]"""
    rng = np.random.default_rng(seed)
    out = rng.normal(0.45, 0.4, size=(B, 3, h + below, w + PAD + right)).astype(np.float32)
    gt = rng.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    return out, gt


def plant_specials(out, h, w, inside, outside, pad=PAD):
    """a copy of `out` with NaN / +inf / -inf inside the crop of the images `inside` ({image: kinds}) and outside the crop of `outside`"""
    out = out.copy()
    vals = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
    for b, kinds in inside.items():
        for j, kind in enumerate(kinds):
            out[b, j % 3, (h - 1) if j == 0 else (j * 2) % h, pad + ((w - 1) if j == 0 else j % w)] = vals[kind]          # j = 0: the crop's last pixel
    for b in outside:
        out[b, 0, 0, pad - 1] = np.nan          # left of the crop
        out[b, 1, h, pad] = np.inf              # below it
        out[b, 2, 0, pad + w] = -np.inf         # right of it
    return out


# ---- rint(clip(x) * 255): to_ubyte_kernel and ubyte_planes_kernel ----------------------------------------------------------------------------
def to_ubyte_expected(x32, mutation=None):
    """rint(fl32(clip(x, 0, 1) * 255)) as doubles in [0, 255]: the product is exact in fp64, rounds once to fp32, then ties go to even.
    A NaN gives 0 (fmaxf(NaN, 0) = 0, the kernel's documented behaviour)."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    c = np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 1.0))
    p = (c * 255.0).astype(np.float32).astype(np.float64)
    if mutation == "round_half_up":
        return np.floor(p + 0.5)
    if mutation == "truncate":
        return np.floor(p)
    return np.rint(p)


def half_products():
    """fp32 x in [0, 1] whose fp32 product x * 255 is EXACTLY k + 0.5 -> {k: x}, searched among the neighbours of (k + 0.5) / 255"""
    found = {}
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        cand = [x]
        for _ in range(6):
            cand = [np.nextafter(cand[0], np.float32(-1))] + cand + [np.nextafter(cand[-1], np.float32(2))]
        for c in cand:
            if np.float32(np.float64(c) * 255.0) == np.float32(k + 0.5):
                found[k] = c
                break
    return found


def ubyte_pool():
    """the ties first (both parities of k), then -0.0, values below 0 and above 1, NaN, infinities, then every k / 255 with its two neighbours"""
    ties = half_products()
    head = [ties[k] for k in sorted(ties)]
    head += [-0.0, 0.0, -1e-8, -0.3, -1e30, 1.0, 1.0000001, 1.7, 1e30, np.nan, np.inf, -np.inf, 2.0 ** -149, 0.5 / 255]
    k = (np.arange(256, dtype=np.float32) / np.float32(255))
    body = np.stack([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))], 1).reshape(-1)
    return np.concatenate([np.asarray(head, dtype=np.float32), body]).astype(np.float32)


UBYTE_N = (1, 255, 257, 4099)


def ubyte_inputs(n):
    """n values: the pool's head (n = 4099 holds all of it, then uniform values in [-0.1, 1.1])"""
    pool = ubyte_pool()
    if n <= pool.size:
        return pool[:n].copy()
    rest = np.random.RandomState(n).uniform(-0.1, 1.1, n - pool.size).astype(np.float32)
    return np.concatenate([pool, rest])


# ---- the evaluation loop's SSIM -----------------------------------------------------------------------------------------------------------
def metric_window():
    """cv2.getGaussianKernel(11, 1.5) normalised in fp64, as the floats the kernel receives"""
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return tuple(f32(v) for v in (g / g.sum()).tolist())


METRIC_C1, METRIC_C2 = f32((0.01 * 255) ** 2), f32((0.03 * 255) ** 2)          # 6.5025, 58.5225 as the kernel's floats
SSIM_SHAPES = ((3, 11, 11), (2, 12, 27), (1, 40, 23))                           # (B, h, w): one valid position; ragged; taller than wide
SSIM_FAMILIES = ("natural", "dark", "bright_flat", "identical")


def ssim_inputs(shape, family, seed):
    """-> (restored fp32 [B,h,w,3] in about [0, 1], ground truth uint8 [B,h,w,3])"""
    B, h, w = shape
    rng = np.random.RandomState(seed)
    if family == "dark":
        gt = rng.randint(0, 9, size=(B, h, w, 3))
        res = (gt + rng.randn(B, h, w, 3) * 2.0) / 255.0
    elif family == "bright_flat":
        gt = rng.randint(248, 253, size=(B, h, w, 3))
        res = (250.0 + rng.randn(B, h, w, 3) * 2.0) / 255.0
    else:
        gt = rng.randint(0, 256, size=(B, h, w, 3))
        res = gt / 255.0 + (0.0 if family == "identical" else rng.randn(B, h, w, 3) * 0.1)
    return res.astype(np.float32), gt.astype(np.uint8)


def ssim_metric_fp64(x255, y255):
    """fp64 SSIM of two [B,h,w,3] planes in [0, 255], the utils2 form (11-tap window at the valid positions, C1 = 6.5025, C2 = 58.5225, mean
    of the map over positions and channels) per image -> ([B] values, [B] lists of moments), through loss_fp64.ssim_forward"""
    x, y = torch.as_tensor(x255, dtype=torch.float64), torch.as_tensor(y255, dtype=torch.float64)
    outs = [loss_fp64.ssim_forward(x[b:b + 1], y[b:b + 1], metric_window(), METRIC_C1, METRIC_C2) for b in range(x.shape[0])]
    return torch.stack([o[1] for o in outs]), [o[0] for o in outs]


# ---- the word-owning byte kernels' two-level sums (post_u8_kernel / score_u8_kernel and their finish kernels) ---------------------------------
def word_sums(values, mutation=None):
    """values int [B, n] (one per output byte: a non-finite flag, a squared difference) -> int64 [B] as the kernels add them: the output is
    one flat array of 4-byte words, a word belongs to the image of its FIRST byte, what it carries of the next image goes to a second
    (`spill`) partial, and the finish kernel adds own[b] + spill[b - 1], one thread per image in blocks of 64"""
    v = np.asarray(values, dtype=np.int64)
    B, n = v.shape
    flat = v.reshape(-1)
    own, spill = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        lo, hi = (n * b + 3) // 4 * 4, min((n * (b + 1) + 3) // 4 * 4, n * B)
        own[b] = flat[lo:min(hi, n * (b + 1))].sum()
        spill[b] = flat[n * (b + 1):hi].sum()
    tot = np.zeros(B, dtype=np.int64)
    for b in range(B):
        src = b % 64 if mutation == "second_block_dropped" else b
        tot[b] = own[src] + (spill[src] if mutation == "spill_to_wrong_image" else (spill[src - 1] if src > 0 else 0))
    return tot


TINY_IMAGES = (65, 5, 6, (1, 2, 3, 3))           # (B, Hp, Wp, (top, left, h, w)): 27 bytes per image, most images start mid-word
SECOND_TRIP = (2, 185, 250, (2, 4, 181, 243))    # 131 949 bytes, 43 983 pixels per image: a second, ragged trip of the 131 072-byte / 32 768-pixel loops


def tiny_outputs(special=True):
    """the many-tiny-images case: output_and_gt's values, with specials (when asked) in images 0, 63 and 64 and in the first bytes of images
    1, 2, 3, 62 and 64 -- the bytes the previous image's last word carries"""
    B, Hp, Wp, (top, left, h, w) = TINY_IMAGES
    x, gt = output_and_gt(B, Hp, Wp, special=False)
    if special:
        kinds = (float("nan"), float("inf"), float("-inf"))
        for j, b in enumerate((0, 63, 64)):
            x[b, 1, top + 1, left + 1] = kinds[j]
            x[b, 2, top + 2, left + 2] = kinds[(j + 1) % 3]
        x[64, 0, top + 2, left + 0] = float("nan")          # image 64 differs from image 0 in its count
        for j, b in enumerate((1, 2, 3, 62, 64)):            # pixel 0, channels 0 .. 2: bytes 0 .. 2 of the image
            for c in range(1 + j % 3):
                x[b, c, top, left] = kinds[(j + c) % 3]
    return x, gt[:, :h, :w].contiguous()


def window_nonfinite(x, window):
    top, left, h, w = window
    v = np.asarray(x)[:, :, top:top + h, left:left + w].transpose(0, 2, 3, 1)
    return (~np.isfinite(v)).reshape(v.shape[0], -1)


def adjust_gain_fp64(out, gt, window, mutation=None):
    """glare_amd.harness.adjust_gain (the existing host restatement), with the two ways a gain kernel goes wrong"""
    from glare_amd import harness

    out = np.asarray(out, dtype=np.float32)
    if mutation == "gain_from_clamped_means":
        out = np.clip(out, 0, 1)
    gt = np.asarray(gt)
    if mutation == "gray_weights_bgr":
        gt = gt[..., ::-1]
    return harness.adjust_gain(out, gt, window)


# ---- LPIPS: the direct convolution, the pool, the tap -----------------------------------------------------------------------------------------
ALEX = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))          # (k, stride, pad) of the five AlexNet convolutions
CONV_COUT = (1, 7, 33, 40)                                               # a ragged group of 8, a ragged block of 32
CONV_OHW = ((1, 1), (7, 9), (5, 13))                                     # 1, 63 and 65 output pixels against a block of 64
# (k, stride, pad, Cin): Cin across a ragged last chunk of the filter staging (chunk = 8192 / (32 k k) channels: 28, 10, 2, 1)
CONV_CIN = ((3, 1, 1, 29), (3, 1, 1, 57), (5, 1, 2, 64), (11, 4, 2, 3), (16, 4, 2, 3))


def conv_input_size(o, k, stride, pad):
    """the smallest input side that gives o outputs"""
    return (o - 1) * stride + k - 2 * pad


def conv_fp64(x, w, bias=None, stride=1, pad=0, relu=False, shift=None, scale=None, mutation=None):
    """conv_direct_f32_kernel in fp64 (F.conv2d on the CPU) -> (exact, bound).  x' = (x - shift) / scale where the affine is on, the padding
    applied AFTER it (padding taps contribute exactly 0).  Counted from metrics.hip:57-72: one fma per tap on the running sum, taps = Cin k k
    links, each below U sum |w| |x'|; the bias addition one more on sum |w| |x'| + |bias|; where the affine is on, x' carries the subtraction's
    and the division's rounding, two more per tap: (taps + 2 [+ 2]) U sum |w| |x'| + U |bias|.  ReLU is 1-Lipschitz."""
    x, w = x.double(), w.double()
    xp = x
    if shift is not None:
        sh, sc = shift.double().view(1, -1, 1, 1), scale.double().view(1, -1, 1, 1)
        if mutation == "pad_before_affine":
            xp = (F.pad(x, (pad, pad, pad, pad)) - sh) / sc
            pad = 0
        else:
            xp = (x - sh) / sc
    b = None if bias is None else bias.double()
    exact = F.conv2d(xp, w, b, stride, pad)
    taps = w.shape[1] * w.shape[2] * w.shape[3]
    mag = F.conv2d(xp.abs(), w.abs(), None, stride, pad)
    bound = (taps + 2 + (2 if shift is not None else 0)) * U * mag + (0.0 if b is None else U * b.abs().view(1, -1, 1, 1)) + 2.0 ** -149
    if relu:
        exact = torch.where(exact < 0, torch.zeros_like(exact), exact)          # a NaN stays, as torch.relu keeps it
    return exact, bound


LPIPS_EPS = f32(1e-10)
TAP_HW = (1, 255, 257, 600)
TAP_C = (1, 64, 384)
TAP_SMALL = 1e-5          # the scale of the second image's features where a test wants eps to matter


def lpips_tap_fp64(f0, f1, lin, eps=LPIPS_EPS, mutation=None):
    """sum_p sum_c lin[c] (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2 / HW per image, fp64; f: [B, C, HW]"""
    f0, f1, lin = f0.double(), f1.double(), lin.double()

    def unit(f):
        n = (f * f).sum(1, keepdim=True)
        return f / (torch.sqrt(n + eps) if mutation == "eps_inside_sqrt" else torch.sqrt(n) + eps)

    d = unit(f0) - unit(f1)
    return ((d * d) * lin.view(1, -1, 1)).sum(1).mean(1)


def tap_inputs(B, C, HW, seed, zero_pixels=True):
    """features after a ReLU (non-negative, a third of them 0), two images' worth; pixel 0 all zero in f0 only and pixel 1 in both (where
    they exist): 0 / (0 + eps) = 0, so the first contributes sum_c lin[c] n1[c]^2 and the second exactly 0"""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.relu(torch.randn(B, C, HW, generator=g) + 0.4)
    f1 = torch.relu(f0 + torch.randn(B, C, HW, generator=g) * 0.5)
    lin = torch.rand(C, generator=g) * 0.1
    if zero_pixels and HW > 2:
        f0[:, :, 0] = 0
        f0[:, :, 1] = 0
        f1[:, :, 1] = 0
    return f0, f1, lin


MUTATIONS = {
    "gain": ("gain_from_clamped_means", "gray_weights_bgr"),
    "rounding": ("round_half_up", "truncate"),
    "padding": ("fold_period_2n", "pad_before_affine"),
    "finish": ("spill_to_wrong_image", "second_block_dropped"),
    "lpips": ("eps_inside_sqrt",),
}
