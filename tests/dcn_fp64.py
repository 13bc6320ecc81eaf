"""Modulated deformable convolution (DCNv2) forward restated in plain fp64 torch for any kernel size, stride, padding, dilation and
deformable group count: the reference of test_gpu_dcn_edges.py (csrc/dcn.hip: dcn_fwd_kernel, dcn_fwd_fast_kernel; csrc/dcn_generic.hip),
checked against the C oracle and F.conv2d in test_dcn_fp64_host.py.  Written from the header of dcn.hip:
    out[p, co] = bias[co] + sum_{g, t, c} W[co, g cpg + c, t] mask[g, t, p] bilinear(x[., g cpg + c], pos(p, g, t))
    a sample is 0 unless -1 < h < H and -1 < w < W; each of the 4 corners is dropped on its own when it lies outside the image.
The sampling POSITION is the kernels' one fp32 addition, float(ho s - p + t d) + offset, done here in fp32 as well: floor, the in-image
test and the choice of corners are then the same decisions, and no element sits on a disagreement about floor.  Everything after the
position is fp64: the fractions, 1 - l, the four weights, (w1 v1 + w2 v2 + w3 v3 + w4 v4) mask, the optional sigmoid of the mask logit,
the contraction, the bias.  A plain module like tolerances.py.

Rounding points of the output forms (what a kernel may do to the fp64 value `out`):
    fp32 NHWC, fp32 NCHW planar     none of their own: the fp32 accumulator + bias
    16-bit NHWC (fused form)        rounded ONCE from accumulator + bias
    tile sums (fused form)          the fp32 values BEFORE that rounding, summed per tile of 64 (128) pixels x Co; tiles are cut per image

SLACK of the random family (slack(); U = 2^-24, S = (sum_i w_i |v_i|) |mask| the magnitude of a sample, mag = sum |W| S):
    weights   l = h - floor(h) is exact; 1 - l rounds, twice per weight, and the product: 3 U
    blend     lean kernel: one product and three fmaf, 4 U; general and generic kernels as written, uncontracted: four products and three
              additions, 7 U -- the looser is counted (how the compiler contracts them is not looked at); the product with the mask: U
    sigmoid   1 / (1 + expf(-a)): conv_fp64.sigmoid_rel's count, (sigmoid(-a) (4 + 2 |a|) + 2) U, bounded by (6 + 2 max |a|) U
    split     v = hi + lo + r with |r| <= 2^-18 |v| (two bf16 roundings), the same for the filter; the contraction drops lo lo:
              3 x 2^-18 mag.  Single-pass form instead: sample and filter rounded once to the 16-bit format, 2 u16 (1 + u16) mag
    MFMA      fp32 accumulation of n = dg K cpg products, n U mag; the split form accumulates 3 n, the lo products at most 2^-8 of the hi
              ones: 3 n (1 + 2^-7) U mag
    generic   dcn_generic.hip: no split, one fmaf per product: C / groups K U mag
    bias      U (mag + |bias|)
    sums      against the fp64 sum of the fp32 values written.  A lane chains the 16 MT NT values it owns: 16 MT NT U sum_lane |v|; summed over
              the lanes that is 16 MT NT U sum_tile |v| -- the per-lane count and the per-tile count are the same number -- then the lane tree
              (6) and the four waves: (16 MT NT + 10) U sum |value|

EXACT FAMILY (exact_operands): x and the filter hold small integers, offsets multiples of 1/4, masks multiples of 1/4 (mask_is_logit = 0):
positions are multiples of 1/4 (exact in fp32), the four weights multiples of 1/16, a sample n / 64 with |n| <= 128 -- 8 significant bits,
held by `hi` alone.  The filter holds 8 non-zeros of +-1 per output channel, so sum |terms| <= 16 per output and <= 2^18 per tile of
128 x 128 or 64 x 256 values: every partial sum of every order is a multiple of 1/64 below 2^24 / 64, exact in fp32, tile sums included.
`narrow` (the single-pass form): offsets in halves, masks in {1/2, 1}, |x| <= 3: samples n / 8, |n| <= 24, exact in bf16 and fp16 too."""
import math

import torch
import torch.nn.functional as F

from conv_fp64 import U, fmt


def out_size(H, W, k, s, p, d):
    return (H + 2 * p - (d * (k - 1) + 1)) // s + 1, (W + 2 * p - (d * (k - 1) + 1)) // s + 1


def positions(Ho, Wo, k, s, p, d, offset):
    """offset [B, dg 2K, Ho Wo] fp32 -> (h, w) [B, dg, K, Ho, Wo] fp32: ONE fp32 addition each, as every kernel does it"""
    B, K = offset.shape[0], k * k
    dg = offset.shape[1] // (2 * K)
    off = offset.float().view(B, dg, K, 2, Ho, Wo)
    t = torch.arange(K, device=offset.device)
    bh = (torch.arange(Ho, device=offset.device).view(1, Ho, 1) * s - p + (t // k).view(K, 1, 1) * d).float()
    bw = (torch.arange(Wo, device=offset.device).view(1, 1, Wo) * s - p + (t % k).view(K, 1, 1) * d).float()
    return bh + off[:, :, :, 0], bw + off[:, :, :, 1]


def dcn_fp64(x, offset, mask, w, bias, k, s, p, d, dg, groups=1, mutate=None):
    """x [B, H, W, C] fp64, offset [B, dg 2K, Ho Wo] fp32, mask [B, dg K, Ho Wo] fp64 VALUES (the caller applies the sigmoid), w [Co, C / groups, k, k]
    fp64, bias [Co] or None -> (out [B, Ho, Wo, Co], mag, smag): mag = sum |W| S, smag [B, Ho, Wo] the largest S of a pixel (for reports)"""
    B, H, W, C = x.shape
    Co, K, cpg = w.shape[0], k * k, C // dg
    Ho, Wo = out_size(H, W, k, s, p, d)
    hp, wp = positions(Ho, Wo, k, s, p, d, offset)
    mk = mask.view(B, dg, K, Ho, Wo)
    cols = torch.zeros(B, Ho, Wo, C, K, dtype=torch.float64, device=x.device)
    acol = torch.zeros_like(cols)
    bi = torch.arange(B, device=x.device).view(B, 1, 1)
    for g in range(dg):
        for t in range(K):
            h, ww_ = hp[:, g, t], wp[:, g, t]
            if mutate == "offsets_swapped" and g == 0 and t == 0:          # offset_w read for h and offset_h for w: the bases stay
                oh = offset.float().view(B, dg, K, 2, Ho, Wo)[:, 0, 0]
                h, ww_ = (h - oh[:, 0]) + oh[:, 1], (ww_ - oh[:, 1]) + oh[:, 0]
            h, ww_ = h.double(), ww_.double()
            m = mk[:, g, (t + 1) % K if (mutate == "mask_of_next_tap" and t == 0) else t]
            lo_ok = (h >= -1) if mutate == "ge_at_minus_one" else (h > -1)
            hi_ok = (h <= H) if mutate == "le_at_h" else (h < H)
            inside = lo_ok & hi_ok & (ww_ > -1) & (ww_ < W)
            hl, wl = torch.floor(h), torch.floor(ww_)
            lh, lw = h - hl, ww_ - wl
            gs = (g + 1) % dg if mutate == "group_of_next" and g == 0 else g
            xs = x[..., gs * cpg:(gs + 1) * cpg]
            val = torch.zeros(B, Ho, Wo, cpg, dtype=torch.float64, device=x.device)
            aval = torch.zeros_like(val)
            for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                yy, xx = hl + dy, wl + dx
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                if mutate == "corner_kept" and dy == 1:          # the row below the image is read (clamped) instead of dropped
                    ok = inside & (yy >= 0) & (yy <= H) & (xx >= 0) & (xx <= W - 1)
                v = xs[bi, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()] * ok.unsqueeze(-1)
                val += wt.unsqueeze(-1) * v
                aval += wt.unsqueeze(-1) * v.abs()
            if mutate == "tap_dropped" and g == 0 and t == K - 1:
                continue
            cols[..., g * cpg:(g + 1) * cpg, t] = val * m.unsqueeze(-1)
            acol[..., g * cpg:(g + 1) * cpg, t] = aval * m.abs().unsqueeze(-1)
    Cg, Cog = C // groups, Co // groups
    out = torch.empty(B, Ho, Wo, Co, dtype=torch.float64, device=x.device)
    mag = torch.empty_like(out)
    for gr in range(groups):
        wg = w[gr * Cog:(gr + 1) * Cog].reshape(Cog, Cg * K)
        out[..., gr * Cog:(gr + 1) * Cog] = cols[..., gr * Cg:(gr + 1) * Cg, :].reshape(B, Ho, Wo, Cg * K) @ wg.t()
        mag[..., gr * Cog:(gr + 1) * Cog] = acol[..., gr * Cg:(gr + 1) * Cg, :].reshape(B, Ho, Wo, Cg * K) @ wg.abs().t()
    if bias is not None:
        out = out + (bias.roll(-1) if mutate == "bias_of_next" else bias)
    if mutate == "pixel_of_next_image":
        out = out.clone()
        out[:, Ho - 1, Wo - 1] = out.roll(-1, 0)[:, 0, 0]
    return out, mag, acol.amax((-1, -2))


MUTATIONS = ("ge_at_minus_one", "le_at_h", "corner_kept", "offsets_swapped", "mask_of_next_tap", "group_of_next", "pixel_of_next_image",
             "tap_dropped", "bias_of_next")
# With per-corner dropping the in-image rule decides nothing of its own AT its two limits: at h = -1 the only row that exists (row 0) has the
# weight l = 0, at h = H both rows are outside.  These two mutations must therefore change NOTHING -- asserted, so that a kernel is free to
# take either comparison; inside the limits ((-1, 0) and (H - 1, H)) the corner rules carry the semantics, and `corner_kept` guards them.
SILENT = ("ge_at_minus_one", "le_at_h")


def mask_values(mask, is_logit):
    return torch.sigmoid(mask.double()) if is_logit else mask.double()


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 9), (9, 1), (5, 7), (8, 8), (5, 13))
BS = (1, 3)
# launch_dcn_fast restated: (kernel, NT, NCH, MT, WN)
LEAN = [dict(name="wn4-co128-cpg32", C=128, Co=128, dg=4, single=False), dict(name="wn4-co256-cpg32", C=64, Co=256, dg=2, single=False),
        dict(name="wn4-co128-cpg64", C=64, Co=128, dg=1, single=False), dict(name="wn4-co256-cpg64", C=128, Co=256, dg=2, single=False),
        dict(name="split-co64-cpg32", C=32, Co=64, dg=1, single=False), dict(name="split-co64-cpg64", C=64, Co=64, dg=1, single=False),
        dict(name="single-co64-cpg32", C=32, Co=64, dg=1, single=True), dict(name="single-mt2-co128-cpg32", C=128, Co=128, dg=4, single=True),
        dict(name="single-co256-cpg32", C=32, Co=256, dg=1, single=True), dict(name="single-co64-cpg64", C=64, Co=64, dg=1, single=True),
        dict(name="single-co128-cpg64", C=64, Co=128, dg=1, single=True), dict(name="single-co256-cpg64", C=128, Co=256, dg=2, single=True)]


def lean_dispatch(C, Co, dg, single):
    """-> ("fast", NT, NCH, MT, single, WN) as launch_dcn_fast picks it, None where it has no instantiation (Co = 192)"""
    nt, nch = Co // 64, (C // dg) // 8
    if single and nt == 2 and nch == 4:
        return ("fast", 2, 4, 2, True, 2)
    if not single and nch % 2 == 0 and Co in (128, 256):
        return ("fast", Co // 128, nch, 2, False, 4)
    if nt in (1, 2, 4) and nch in (4, 8):
        return ("fast", nt, nch, 1, single, 2)
    return None


def tile_pixels(C, Co, dg, single):
    d = lean_dispatch(C, Co, dg, single)
    return 32 * d[3] * (4 // d[5])


def general_dispatch(C, Co, dg):
    """launch_dcn: (NT, ITEMS) of dcn_fwd_kernel, None without an instantiation"""
    nt, items = Co // 64, 64 * ((C // dg) // 8) // 256
    return (nt, items) if nt in (1, 2, 4) and items in (1, 2) else None


def dcn_check(C, Co, dg, groups=1):
    """dcn.hip's dcn_check: does the drop-in take the MFMA kernels (True) or dcn_generic.hip (False)"""
    return groups == 1 and C % dg == 0 and C // dg in (32, 64) and Co % 64 == 0 and Co <= 256


# three of test_gpu_dcn.py's GENERIC_CASES (B, C, H, W, Co, k, stride, pad, dil, groups, dg): the 1x1, a grouped one (conv AND deformable groups),
# and one whose channels per deformable group are neither 32 nor 64 (stride 2, dilation 2, four conv groups)
GENERIC = [(1, 8, 10, 6, 6, 1, 1, 0, 1, 1, 2), (2, 12, 7, 9, 8, 3, 1, 1, 1, 2, 3), (1, 16, 9, 11, 24, 3, 2, 2, 2, 4, 1)]
# the MFMA geometries of the drop-in test (the MFMA kernel with planar output) and of the general-kernel test
DROP_IN = [dict(name="cpg32-co64", C=64, Co=64, dg=2, k=3, s=1, p=1, d=1, bias=True), dict(name="cpg64-co128-s2", C=64, Co=128, dg=1, k=3, s=2, p=1, d=1, bias=False),
           dict(name="cpg32-co256-d2", C=32, Co=256, dg=1, k=3, s=1, p=2, d=2, bias=True)]
DROP_IN += [dict(name="generic-%s" % n, C=c[1], Co=c[4], dg=c[10], k=c[5], s=c[6], p=c[7], d=c[8], groups=c[9], bias=b, own=(c[2], c[3], c[0]))
            for n, b, c in zip(("1x1", "grouped", "s2-d2-groups4"), (True, False, True), GENERIC)]
GENERAL = [dict(C=64, Co=128, dg=2, want=(2, 1)), dict(C=64, Co=64, dg=1, want=(1, 2)), dict(C=128, Co=256, dg=2, want=(4, 2))]
PLANAR = (5, 5, 4)          # H, W, B of the planar test: a 64-pixel tile spans three images


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def fixed_offsets(H, W, narrow=False):
    """[n] pairs (target h, target w) a case plants so that positions hit the limits of the sampling rule: exactly -1, inside (-1, 0), exactly
    H - 1, inside (H - 1, H), exactly H -- for h, and the same five for w -- and far outside"""
    hs = [-1.0, -0.5 if narrow else -0.25, H - 1.0, H - (0.5 if narrow else 0.25), float(H)]
    ws = [-1.0, -0.5 if narrow else -0.75, W - 1.0, W - 0.5, float(W)]
    pairs = [(h, 0.5 * (W - 1)) for h in hs] + [(0.5 * (H - 1), w) for w in ws] + [(h, w) for h, w in zip(hs, ws)]
    pairs += [(1e4, 0.0), (0.0, -1e4), (-1e4, 1e4), (3e9, 0.0), (0.0, -3e9)]
    return pairs


def operands(C, Co, dg, H, W, B, fam, k=3, s=1, p=1, d=1, groups=1, narrow=False, seed=0, scale=None):
    """-> dict x [B, H, W, C], offset [B, dg 2K, Ho Wo] fp32, mask [B, dg K, Ho Wo] fp32, w, bias (fp64), is_logit.
    fam "exact": the module's exact family (mask values, is_logit = 0); "random": normal x / filter, offsets of `scale` (0.3 or 4) with the
    fixed positions of fixed_offsets planted tap by tap, mask LOGITS."""
    g = torch.Generator().manual_seed(1000 * C + 10 * Co + 100000 * H + 1000000 * W + B + seed)
    K = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    n = Ho * Wo
    if fam == "exact":
        q = 2.0 if narrow else 4.0
        x = torch.randint(-3 if narrow else -2, (3 if narrow else 2) + 1, (B, H, W, C), generator=g).double()
        offset = torch.randint(-8, 9, (B, dg * 2 * K, n), generator=g).float() / q
        mask = (torch.randint(1, 3, (B, dg * K, n), generator=g).float() / 2.0) if narrow else (torch.randint(1, 5, (B, dg * K, n), generator=g).float() / 4.0)
        w = torch.zeros(Co, (C // groups) * K, dtype=torch.float64)
        co = torch.arange(Co).view(Co, 1)
        j = torch.arange(8).view(1, 8)
        pos = (co * 37 + j * ((C // groups) * K // 8) + j * j * 5) % ((C // groups) * K)
        w.scatter_(1, pos, (1.0 - 2.0 * ((co + j) % 2)).double().expand(Co, 8).clone())
        w = w.view(Co, C // groups, k, k)
        bias = (torch.arange(Co) % 7 - 3).double()
        is_logit = False
    else:
        x = torch.randn(B, H, W, C, generator=g).double()
        offset = (torch.randn(B, dg * 2 * K, n, generator=g) * (scale or 0.3)).float()
        mask = torch.randn(B, dg * K, n, generator=g).float() * 2.0
        w = (torch.randn(Co, C // groups, k, k, generator=g) / math.sqrt(C // groups * K)).float().double()
        bias = torch.randn(Co, generator=g).float().double()
        is_logit = True
    # the fixed positions, each on a slot (image, group, tap, pixel) of its own, as the offset that reaches the target from that slot's base: spread
    # evenly over the slots; where a case has fewer slots than positions (1x1 images), the first ones of the list -- the limits of h, then of w
    ov = offset.view(B, dg, K, 2, n)
    pairs = fixed_offsets(H, W, narrow)
    total = B * dg * K * n
    planted = []
    for i, (th, tw) in enumerate(pairs[:total]):
        idx = (i * total) // len(pairs) if total >= len(pairs) else i
        px, t_, g_, b_ = idx % n, (idx // n) % K, (idx // (n * K)) % dg, idx // (n * K * dg)
        bh, bw = (px // Wo) * s - p + (t_ // k) * d, (px % Wo) * s - p + (t_ % k) * d
        ov[b_, g_, t_, 0, px], ov[b_, g_, t_, 1, px] = th - bh, tw - bw
        planted.append((b_, g_, t_, px, th, tw))
    return dict(x=x, offset=offset, mask=mask, w=w, bias=bias, is_logit=is_logit, geom=(k, s, p, d, dg, groups), planted=planted)


def reference(o, mutate=None, bias=True):
    k, s, p, d, dg, groups = o["geom"]
    return dcn_fp64(o["x"], o["offset"], mask_values(o["mask"], o["is_logit"]), o["w"], o["bias"] if bias else None, k, s, p, d, dg, groups, mutate)


def slack(o, mag, form, dtype=None, bias=True):
    """form: "split" (both MFMA kernels, fp32-class), "single" (16-bit sample and filter; dtype), "generic" (dcn_generic.hip)"""
    k, s, p, d, dg, groups = o["geom"]
    C = o["x"].shape[-1]
    n = (C // groups) * k * k
    elem = (3 + 7 + 1) * U + ((6.0 + 2.0 * float(o["mask"].abs().max())) * U if o["is_logit"] else 0.0)          # sigmoid_rel's count at the largest |logit|
    if form == "split":
        terms = 3 * 2.0 ** -18 + 3 * n * (1 + 2.0 ** -7) * U
    elif form == "single":
        u16 = 2.0 ** -(fmt(dtype)[0] + 1)
        terms = 2 * u16 * (1 + u16) + n * U
    else:
        terms = n * U
    b = o["bias"].abs().to(mag.device) if (bias and o["bias"] is not None) else 0.0
    return (elem + terms) * mag + U * (mag + b) + 2.0 ** -149          # no sample inside the image and no bias: the bound is an exact 0 (the floor keeps 0 / 0 out)


def tile_sums(values, tile):
    """values [B, Ho, Wo, Co] -> (sums [B, ceil(Ho Wo / tile)], sum |values| per tile): tiles cut per image"""
    B, Ho, Wo, Co = values.shape
    n = Ho * Wo
    nt = -(-n // tile)
    v = torch.zeros(B, nt * tile, Co, dtype=values.dtype, device=values.device)
    v[:, :n] = values.reshape(B, n, Co)
    v = v.view(B, nt, tile * Co)
    return v.sum(-1), v.abs().sum(-1)


def conv2d_reference(x, w, bias, k, s, p, d, groups=1):
    """F.conv2d on NHWC fp64 operands -> NHWC"""
    return F.conv2d(x.permute(0, 3, 1, 2), w, bias, s, p, d, groups).permute(0, 2, 3, 1)
