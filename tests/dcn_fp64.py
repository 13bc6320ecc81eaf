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
`narrow` (the single-pass form): offsets in halves, masks in {1/2, 1}, |x| <= 3: samples n / 8, |n| <= 24, exact in bf16 and fp16 too.

Geometry is per axis throughout: k, s, p, d are an int or a pair (along h, along w).  The second half of the module (BACKWARD, below) restates
the five gradients of csrc/dcn_bwd.hip and of dcn_generic.hip's backward kernels: the reference of test_gpu_dcn_bwd_edges.py, with its own header
(formulas, the count behind slack_bwd, the backward's exact family)."""
import math

import torch
import torch.nn.functional as F

from conv_fp64 import U, fmt


def pair(v):
    """a geometry argument per axis: an int stands for (v, v), a pair is (along h, along w)"""
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_size(H, W, k, s, p, d):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def positions(Ho, Wo, k, s, p, d, offset, taps_per_row=None):
    """offset [B, dg 2K, Ho Wo] fp32 -> (h, w) [B, dg, K, Ho, Wo] fp32: ONE fp32 addition each, as every kernel does it.  Tap t sits in filter
    row t // kw, column t % kw (taps_per_row: a mutation's other divisor)"""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    B, K = offset.shape[0], kh * kw
    dg = offset.shape[1] // (2 * K)
    off = offset.float().view(B, dg, K, 2, Ho, Wo)
    t = torch.arange(K, device=offset.device)
    div = kw if taps_per_row is None else taps_per_row
    bh = (torch.arange(Ho, device=offset.device).view(1, Ho, 1) * sh - ph + (t // div).view(K, 1, 1) * dh).float()
    bw = (torch.arange(Wo, device=offset.device).view(1, 1, Wo) * sw - pw + (t % div).view(K, 1, 1) * dw).float()
    return bh + off[:, :, :, 0], bw + off[:, :, :, 1]


def dcn_fp64(x, offset, mask, w, bias, k, s, p, d, dg, groups=1, mutate=None):
    """x [B, H, W, C] fp64, offset [B, dg 2K, Ho Wo] fp32, mask [B, dg K, Ho Wo] fp64 VALUES (the caller applies the sigmoid), w [Co, C / groups, k, k]
    fp64, bias [Co] or None -> (out [B, Ho, Wo, Co], mag, smag): mag = sum |W| S, smag [B, Ho, Wo] the largest S of a pixel (for reports)"""
    B, H, W, C = x.shape
    Co, K, cpg = w.shape[0], pair(k)[0] * pair(k)[1], C // dg
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
    (kh, kw) = pair(k)
    K = kh * kw
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
        w = w.view(Co, C // groups, kh, kw)
        bias = (torch.arange(Co) % 7 - 3).double()
        is_logit = False
    else:
        x = torch.randn(B, H, W, C, generator=g).double()
        offset = (torch.randn(B, dg * 2 * K, n, generator=g) * (scale or 0.3)).float()
        mask = torch.randn(B, dg * K, n, generator=g).float() * 2.0
        w = (torch.randn(Co, C // groups, kh, kw, generator=g) / math.sqrt(C // groups * K)).float().double()
        bias = torch.randn(Co, generator=g).float().double()
        is_logit = True
    planted = plant(offset, H, W, Wo, k, s, p, d, dg, narrow)
    return dict(x=x, offset=offset, mask=mask, w=w, bias=bias, is_logit=is_logit, geom=(k, s, p, d, dg, groups), planted=planted)


def plant(offset, H, W, Wo, k, s, p, d, dg, narrow=False, share=1):
    """the fixed positions, each on a slot (image, group, tap, pixel) of its own, as the offset that reaches the target from that slot's base: spread
    evenly over the slots; where a case has fewer slots than positions (1x1 images), the first ones of the list -- the limits of h, then of w"""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    B, K = offset.shape[0], kh * kw
    n = offset.shape[-1]
    ov = offset.view(B, dg, K, 2, n)
    pairs = fixed_offsets(H, W, narrow)
    total = B * dg * K * n
    planted = []
    for i, (th, tw) in enumerate(pairs[:total // share]):          # share: at most one slot in `share` is planted
        idx = (i * total) // len(pairs) if total >= len(pairs) else i
        px, t_, g_, b_ = idx % n, (idx // n) % K, (idx // (n * K)) % dg, idx // (n * K * dg)
        bh, bw = (px // Wo) * sh - ph + (t_ // kw) * dh, (px % Wo) * sw - pw + (t_ % kw) * dw
        ov[b_, g_, t_, 0, px], ov[b_, g_, t_, 1, px] = th - bh, tw - bw
        planted.append((b_, g_, t_, px, th, tw))
    return planted


def reference(o, mutate=None, bias=True):
    k, s, p, d, dg, groups = o["geom"]
    return dcn_fp64(o["x"], o["offset"], mask_values(o["mask"], o["is_logit"]), o["w"], o["bias"] if bias else None, k, s, p, d, dg, groups, mutate)


def slack(o, mag, form, dtype=None, bias=True):
    """form: "split" (both MFMA kernels, fp32-class), "single" (16-bit sample and filter; dtype), "generic" (dcn_generic.hip)"""
    k, s, p, d, dg, groups = o["geom"]
    C = o["x"].shape[-1]
    n = (C // groups) * pair(k)[0] * pair(k)[1]
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
    return F.conv2d(x.permute(0, 3, 1, 2), w, bias, pair(s), pair(p), pair(d), groups).permute(0, 2, 3, 1)


# ==== backward =============================================================================================================================
# The five gradients of csrc/dcn_bwd.hip (dcn_bwd_data_kernel, dcn_bwd_weight_kernel, dcn_bwd_reduce_kernel, dcn_bwd_bias_kernel) and of the three
# backward kernels of csrc/dcn_generic.hip: the reference of test_gpu_dcn_bwd_edges.py, checked in test_dcn_bwd_fp64_host.py against the C
# oracle, against autograd of forward_from_positions (below) and against F.conv2d's gradients.  Written from the header of dcn_bwd.hip:
#     cg[p, c, t]      = sum_co gO[p, co] W[co, c, t]
#     g_mask[g, t, p]  = sum_c cg bilinear(x[., g cpg + c], pos(p, g, t))
#     g_offset[.., p]  = sum_c cg mask d bilinear / d(h | w)
#     g_input         += cg mask (corner weight)                       scattered to the (up to) four corners of every sample
#     g_weight[co,c,t] = sum_p gO[p, co] mask bilinear(x[., c], pos)   ACCUMULATED into the caller's buffer, like g_bias[co] = sum_p gO[p, co]
# The position is the forward's one fp32 addition; everything after it is fp64.  d bilinear / d h is ONE-SIDED, as the kernels have it: the
# corners are those of floor(h), the derivative of the weights (1 - lh, lh) is (-1, +1), a dropped corner contributes 0 and lh = 0 is an
# ordinary value (the right-hand derivative) -- which is what autograd of the forward gives with the positions as leaves (floor has gradient 0).
#
# SLACK of the random family (slack_bwd(); U = 2^-24; every count multiplies the gradient's own sum of magnitudes, returned next to it:
# cgm = sum_co |gO| |W| stands for |cg|, sum_i w_i |v_i| for a sample, sum_i |dw_i| |v_i| = hw (|v3| + |v1|) + lw (|v4| + |v2|) for its derivative):
#   MFMA path (dcn_bwd.hip)
#     cg        the fp32 MFMA chain over Co products, one rounding of the partial sum per product: ncg = Co.  KSPLIT = 2 (cpg 32): two chains of
#               Co / 2, each against the magnitudes of its OWN half, so together Co / 2 x the whole, and the halves added at the read:
#               ncg = Co / 2 + 1
#     g_mask    weights 3 (1 - l rounds, twice per weight, and the product), blend w1 v1 + .. + w4 v4 as written 7, cg * (.) 1, the lane's chain
#               over its 8 channels 8, the shuffle tree over the cpg / 8 chunks log2(cpg / 8):              ncg + 11 + 8 + log2(cpg / 8)
#     g_offset  top = cg m 1; hw = 1 - lw 1, v3 - v1 1, the product 1, the sum 1; (.) * top 1; chain 8; tree:  ncg + 6 + 8 + log2(cpg / 8)
#     g_input   per contribution: weight 3, * m 1, * cg 1; the atomics add in ANY order, each addition rounds a partial sum that sum |terms|
#               bounds: cnt, the number of contributions the element receives (counted by the reference):   ncg + 5 + cnt
#     g_weight  column = (blend) m: 3 + 7 + 1; the MFMA chain over the pixels of a split, `per` of them (one rounding per product, summed over
#               the splits against the split's own magnitudes: per x the whole); the 32-term split sum 32; += into the caller's buffer 1
#               (that one also on the buffer's content `init`):                                             11 + min(per, pixels) + 32 + 1
#     g_bias    a thread chains B ceil(n / 256) values, wave tree 6, four waves 2, += 1:                    B ceil(n / 256) + 9
#   generic path (dcn_generic.hip; one fmaf per product)
#     cv        Co / groups fmaf
#     g_mask    bilinear 3 + 7, cv * (.) 1, the thread's chain over cpg channels cpg:                        Co / groups + 11 + cpg
#     g_offset  coordinate_weight: 1 - f 1, four products 1, three additions 3; * cv * m 2; chain cpg:       Co / groups + 7 + cpg
#     g_input   top = cv m 1, wy wx 1, * top 1, atomics cnt:                                                Co / groups + 3 + cnt
#               plus the weights themselves: wy = ah + 1 - y rounds ah + 1 (at most U (H + 1), absolute; the subtraction and y + 1 - ah are
#               exact), the same for wx: 2 U (max(H, W) + 1) x the contributions' magnitudes WITHOUT the weights (`gx_flat`)
#     g_weight  sample 3 + 7 + 1, a thread's fmaf chain ceil(B n / 256), wave tree 6, four waves 2, += 1:    ceil(B n / 256) + 20
#     g_bias    ceil(B n / 256) + 9
# The numbers are read from the two sources, not fitted to a run.
#
# EXACT FAMILY (operands_bwd "exact"): x and grad_out non-zero integers in [-2, 2], the filter DENSE integers in [-1, 1] (the forward's 8 taps per
# row would leave most cg at 0), sampling positions multiples of 1/4 drawn over (-1, H) x (-1, W) (so offsets are multiples of 1/4 and the drawn
# samples land inside whatever the image size and the geometry, a quarter of them with a corner beyond the border; the planted positions are
# the ones on the limits and outside), masks in {1/4 .. 1}, mask_is_logit = 0.  Then cg is an integer, weights are
# multiples of 1/16, g_mask and g_offset multiples of 1/16, g_input and g_weight of 1/64, g_bias an integer: with every sum of magnitudes
# times its denominator below 2^24 (asserted on the CPU for every size the GPU test runs) every partial sum of every order is exact in fp32,
# the atomics of g_input included.
BWD_NAMES = ("gx", "goff", "gmask", "gw", "gb")
BWD_DENOM = dict(gx=64.0, goff=16.0, gmask=16.0, gw=64.0, gb=1.0)
DB_PIX, DB_SPLITS = 64, 32

# launcher of dcn_bwd.hip restated: (NTILE, ITEMS) of dcn_bwd_data_kernel, MT of dcn_bwd_weight_kernel<false, MT, NTILE, ITEMS>
BWD = [dict(name="cpg32-co128", C=128, Co=128, dg=4, want=("mfma", 1, 1, 4, 2)), dict(name="cpg64-co256", C=128, Co=256, dg=2, want=("mfma", 2, 2, 8, 1)),
       dict(name="cpg32-co256", C=64, Co=256, dg=2, want=("mfma", 1, 1, 8, 2)), dict(name="cpg64-co128", C=64, Co=128, dg=1, want=("mfma", 2, 2, 4, 1))]
BWD_GEOMS = [dict(name="3x3", k=3, s=1, p=1, d=1), dict(name="s2", k=3, s=2, p=1, d=1), dict(name="d2", k=3, s=1, p=2, d=2), dict(name="1x1", k=1, s=1, p=0, d=1),
             dict(name="aniso", k=(1, 3), s=(2, 1), p=(0, 1), d=(1, 2))]
# (H, W, B): a 64-pixel tile spans three images; 11 tiles, where the XCD remap moves tiles; 2116 pixels, where a split holds two tiles
BWD_SPECIAL = ((5, 5, 4), (15, 15, 3), (46, 46, 1))


def bwd_dispatch(C, Co, dg, groups=1):
    """-> ("mfma", NTILE, ITEMS, MT, KSPLIT) as glare_mdcn_backward_f32 picks its two MFMA kernels, ("generic",) for dcn_generic.hip"""
    if C % dg or groups != 1 or C // dg not in (32, 64) or Co % 128 or Co > 256:
        return ("generic",)
    nt = (C // dg) // 32
    return ("mfma", nt, nt, Co // 32, 2 if nt == 1 else 1)


def bwd_split(total):
    """the weight pass's split of `total` output pixels -> (per, tiles per split, non-empty splits); per is rounded up to whole 64-pixel tiles"""
    per = -(-(-(-total // DB_SPLITS)) // DB_PIX) * DB_PIX
    return per, per // DB_PIX, -(-total // per)


def bwd_tile_of_block(block, n):
    """dcn_bwd_data_kernel's XCD remap: the pixel tile workgroup `block` of `n` takes"""
    q, r, xcd, k = n // 8, n % 8, block % 8, block // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


def bwd_workspace_bytes(B, C, H, W, Co, kh, kw):
    return (2 * B * C * H * W + Co * C * kh * kw * (1 + DB_SPLITS)) * 4 + 256


def _corners(h, w_, H, W):
    """h, w_ fp64 positions -> inside, and per corner (yy, xx, weight, d weight / dh, d weight / dw, ok): the corners of floor()"""
    inside = (h > -1) & (h < H) & (w_ > -1) & (w_ < W)
    hl, wl = torch.floor(h).detach(), torch.floor(w_).detach()
    lh, lw = h - hl, w_ - wl
    one = torch.ones_like(lh)
    out = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        fy, fx = (lh if dy else 1 - lh), (lw if dx else 1 - lw)
        sy, sx = (one if dy else -one), (one if dx else -one)
        yy, xx = hl + dy, wl + dx
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        out.append((yy, xx, fy * fx, sy * fx, fy * sx, ok))
    return inside, out


def forward_from_positions(x, hp, wp, mask, w, bias, dg, groups=1):
    """the forward as a differentiable function of x, the POSITIONS hp / wp [B, dg, K, Ho, Wo] (fp64 leaves), the mask values, the filter
    and the bias: the same value as dcn_fp64 (asserted on the host) and the function whose autograd the backward restatement must equal"""
    B, H, W, C = x.shape
    Co, K, cpg = w.shape[0], w.shape[2] * w.shape[3], C // dg
    Ho, Wo = hp.shape[-2:]
    mk = mask.view(B, dg, K, Ho, Wo)
    bi = torch.arange(B, device=x.device).view(B, 1, 1)
    cols = []
    for g in range(dg):
        per_tap = []
        for t in range(K):
            _, cs = _corners(hp[:, g, t], wp[:, g, t], H, W)
            val = 0.0
            for yy, xx, wt, _, _, ok in cs:
                v = x[..., g * cpg:(g + 1) * cpg][bi, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()] * ok.unsqueeze(-1)
                val = val + wt.unsqueeze(-1) * v
            per_tap.append(val * mk[:, g, t].unsqueeze(-1))
        cols.append(torch.stack(per_tap, -1))          # [B, Ho, Wo, cpg, K]
    cols = torch.cat(cols, 3)
    Cg, Cog = C // groups, Co // groups
    outs = [cols[..., gr * Cg:(gr + 1) * Cg, :].reshape(B, Ho, Wo, Cg * K) @ w[gr * Cog:(gr + 1) * Cog].reshape(Cog, Cg * K).t() for gr in range(groups)]
    out = torch.cat(outs, -1)
    return out if bias is None else out + bias


def dcn_bwd_fp64(x, offset, mask, w, gout, k, s, p, d, dg, groups=1, mutate=None):
    """x [B, H, W, C] fp64, offset [B, dg 2K, Ho Wo] fp32, mask [B, dg K, Ho Wo] fp64 VALUES, w [Co, C / groups, kh, kw] fp64, gout [B, Ho, Wo, Co]
    fp64 -> dict: gx [B, H, W, C], goff [B, dg 2K, Ho Wo], gmask [B, dg K, Ho Wo], gw like w, gb [Co]; "mag": the sum of magnitudes of each;
    "cnt": how many contributions an element of gx receives; "gx_flat": gx's magnitudes without the corner weights"""
    B, H, W, C = x.shape
    (kh, kw) = pair(k)
    Co, K, cpg = w.shape[0], kh * kw, C // dg
    Ho, Wo = out_size(H, W, k, s, p, d)
    n = Ho * Wo
    hp, wp = positions(Ho, Wo, k, s, p, d, offset, kh if mutate == "khkw_swapped" else None)
    mk = mask.view(B, dg, K, Ho, Wo)
    Cg, Cog = C // groups, Co // groups
    f64 = dict(dtype=torch.float64, device=x.device)
    cg, cgm = torch.empty(B, Ho, Wo, C, K, **f64), torch.empty(B, Ho, Wo, C, K, **f64)
    for gr in range(groups):
        wg, go = w[gr * Cog:(gr + 1) * Cog].reshape(Cog, Cg * K), gout[..., gr * Cog:(gr + 1) * Cog]
        cgm[..., gr * Cg:(gr + 1) * Cg, :] = (go.abs() @ wg.abs()).view(B, Ho, Wo, Cg, K)
        if mutate == "cg_second_half_missing":          # the KSPLIT half: only the first Co / 2 output channels are contracted
            wg, go = wg[:Cog // 2], go[..., :Cog // 2]
        cg[..., gr * Cg:(gr + 1) * Cg, :] = (go @ wg).view(B, Ho, Wo, Cg, K)
    gx, agx, fgx = (torch.zeros(B * H * W, C, **f64) for _ in range(3))
    cnt = torch.zeros(B * H * W, dg, **f64)
    goff, agoff = torch.zeros(B, dg, K, 2, Ho, Wo, **f64), torch.zeros(B, dg, K, 2, Ho, Wo, **f64)
    gmask, agmask = torch.zeros(B, dg, K, Ho, Wo, **f64), torch.zeros(B, dg, K, Ho, Wo, **f64)
    cols, acol = torch.zeros(B, Ho, Wo, C, K, **f64), torch.zeros(B, Ho, Wo, C, K, **f64)
    bi = torch.arange(B, device=x.device).view(B, 1, 1)
    for g in range(dg):
        gs = (g + 1) % dg if mutate == "group_of_next" and g == 0 else g
        xs = x[..., gs * cpg:(gs + 1) * cpg]
        ch = slice(g * cpg, (g + 1) * cpg)
        for t in range(K):
            m = mk[:, g, t]
            inside, cs = _corners(hp[:, g, t].double(), wp[:, g, t].double(), H, W)
            c_, cm_ = cg[..., ch, t], cgm[..., ch, t]
            val, aval, dvh, advh, dvw, advw = (torch.zeros(B, Ho, Wo, cpg, **f64) for _ in range(6))
            for ci, (yy, xx, wt, th, tw, ok) in enumerate(cs):
                yc, xc = yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()
                v = xs[bi, yc, xc] * ok.unsqueeze(-1)
                val += wt.unsqueeze(-1) * v
                aval += wt.unsqueeze(-1) * v.abs()
                dvh += th.unsqueeze(-1) * v
                advh += th.abs().unsqueeze(-1) * v.abs()
                dvw += tw.unsqueeze(-1) * v
                advw += tw.abs().unsqueeze(-1) * v.abs()
                if mutate == "gx_tap_dropped" and g == 0 and t == K - 1:
                    continue
                sc = ok
                if mutate == "corner_kept_in_scatter" and ci >= 2:          # the lower corners: the row below the image is scattered to (clamped)
                    sc = inside & (yy >= 0) & (yy <= H) & (xx >= 0) & (xx <= W - 1)
                idx = ((bi * H + yc) * W + xc).reshape(-1)
                scf = sc.double()
                gx[:, ch].index_add_(0, idx, ((wt * m * scf).unsqueeze(-1) * c_).reshape(-1, cpg))
                agx[:, ch].index_add_(0, idx, ((wt * m.abs() * scf).unsqueeze(-1) * cm_).reshape(-1, cpg))
                fgx[:, ch].index_add_(0, idx, ((m.abs() * scf).unsqueeze(-1) * cm_).reshape(-1, cpg))
                cnt[:, g].index_add_(0, idx, scf.reshape(-1))
            gmask[:, g, t], agmask[:, g, t] = (c_ * val).sum(-1), (cm_ * aval).sum(-1)
            mo = torch.ones_like(m) if mutate == "goff_without_mask" else m
            goff[:, g, t, 0], agoff[:, g, t, 0] = (c_ * dvh).sum(-1) * mo, (cm_ * advh).sum(-1) * mo.abs()
            goff[:, g, t, 1], agoff[:, g, t, 1] = (c_ * dvw).sum(-1) * mo, (cm_ * advw).sum(-1) * mo.abs()
            mw = torch.ones_like(m) if mutate == "gw_without_mask" else m
            cols[..., ch, t], acol[..., ch, t] = val * mw.unsqueeze(-1), aval * mw.abs().unsqueeze(-1)
    if mutate == "gw_past_64_missing":          # of every split of the weight pass only its first 64-pixel tile
        per = bwd_split(B * n)[0]
        keep = ((torch.arange(B * n, device=x.device) % per) < DB_PIX).double().view(B, Ho, Wo, 1, 1)
        cols = cols * keep
    gw, agw = torch.empty_like(w), torch.empty_like(w)
    for gr in range(groups):
        go = gout[..., gr * Cog:(gr + 1) * Cog].reshape(B * n, Cog)
        gw[gr * Cog:(gr + 1) * Cog] = (go.t() @ cols[..., gr * Cg:(gr + 1) * Cg, :].reshape(B * n, Cg * K)).view(Cog, Cg, kh, kw)
        agw[gr * Cog:(gr + 1) * Cog] = (go.abs().t() @ acol[..., gr * Cg:(gr + 1) * Cg, :].reshape(B * n, Cg * K)).view(Cog, Cg, kh, kw)
    gb = (gout[:B - 1] if mutate == "gb_image_missing" else gout).sum((0, 1, 2))
    agb = gout.abs().sum((0, 1, 2))
    if mutate == "goff_hw_swapped":
        goff[:, 0, 0] = goff[:, 0, 0].flip(1)
    if mutate == "gmask_of_next_tap":
        gmask[:, :, 0] = gmask[:, :, 1 % K].clone()
    if mutate == "pixel_of_next_image":          # the last pixel of an image from the first pixel of the next one (a ragged tile's neighbour)
        goff[..., Ho - 1, Wo - 1] = goff.roll(-1, 0)[..., 0, 0]
        gmask[..., Ho - 1, Wo - 1] = gmask.roll(-1, 0)[..., 0, 0]
    out = dict(gx=gx.view(B, H, W, C), goff=goff.view(B, dg * 2 * K, n), gmask=gmask.view(B, dg * K, n), gw=gw, gb=gb)
    out = {name: v + 0.0 for name, v in out.items()}          # no -0: the kernels' sums start from +0
    out["mag"] = dict(gx=agx.view(B, H, W, C), goff=agoff.view(B, dg * 2 * K, n), gmask=agmask.view(B, dg * K, n), gw=agw, gb=agb)
    out["cnt"] = cnt.repeat_interleave(cpg, 1).view(B, H, W, C)
    out["gx_flat"] = fgx.view(B, H, W, C)
    return out


MUTATIONS_BWD = ("goff_hw_swapped", "gmask_of_next_tap", "goff_without_mask", "gw_without_mask", "corner_kept_in_scatter", "gx_tap_dropped", "group_of_next",
                 "cg_second_half_missing", "gw_past_64_missing", "gb_image_missing", "pixel_of_next_image", "khkw_swapped")


def operands_bwd(C, Co, dg, H, W, B, fam, k=3, s=1, p=1, d=1, groups=1, scale=None, seed=0):
    """the forward's operands plus gout [B, Ho, Wo, Co]; mask VALUES (the backward takes no logits).  "random": operands() with its planted
    positions, x / filter / mask values numbers of fp32.  "exact": the backward's exact family (the header above), the same positions planted"""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    K = kh * kw
    Ho, Wo = out_size(H, W, k, s, p, d)
    n = Ho * Wo
    g = torch.Generator().manual_seed(77 + 1000 * C + 10 * Co + 100000 * H + 1000000 * W + B + 13 * kh + 17 * sw + 19 * dh + seed)
    if fam == "exact":
        def nonzero(shape):          # +-1, +-2
            return (torch.randint(1, 3, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).double()
        x = nonzero((B, H, W, C))
        w = torch.randint(-1, 2, (Co, C // groups, kh, kw), generator=g).double()
        gout = nonzero((B, Ho, Wo, Co))
        mask = torch.randint(1, 5, (B, dg * K, n), generator=g).float() / 4.0
        th = torch.randint(-3, 4 * H, (B, dg, K, n), generator=g).float() / 4.0
        tw = torch.randint(-3, 4 * W, (B, dg, K, n), generator=g).float() / 4.0
        t = torch.arange(K)
        px = torch.arange(n)
        bh = ((px // Wo).view(1, n) * sh - ph + (t // kw).view(K, 1) * dh).float()
        bw = ((px % Wo).view(1, n) * sw - pw + (t % kw).view(K, 1) * dw).float()
        offset = torch.stack((th - bh, tw - bw), 3).reshape(B, dg * 2 * K, n).contiguous()
        planted = plant(offset, H, W, Wo, k, s, p, d, dg, share=4)          # a quarter of the slots at most: the smallest cases must not be all limits
        o = dict(x=x, offset=offset, mask=mask, w=w, bias=None, is_logit=False, geom=(k, s, p, d, dg, groups), planted=planted)
    else:
        o = operands(C, Co, dg, H, W, B, "random", k=k, s=s, p=p, d=d, groups=groups, seed=seed, scale=scale)
        o["x"], o["w"] = o["x"].float().double(), o["w"].float().double()
        o["mask"], o["is_logit"] = torch.sigmoid(o["mask"]), False
        gout = torch.randn(B, Ho, Wo, Co, generator=g).float().double()
    o["gout"] = gout
    return o


def reference_bwd(o, mutate=None):
    k, s, p, d, dg, groups = o["geom"]
    return dcn_bwd_fp64(o["x"], o["offset"], o["mask"].double(), o["w"], o["gout"], k, s, p, d, dg, groups, mutate)


def slack_bwd(o, ref, path, init=0.0):
    """-> dict gradient -> bound per element; path "mfma" (dcn_bwd.hip) or "generic" (dcn_generic.hip); init: what grad_weight / grad_bias held"""
    k, s, p, d, dg, groups = o["geom"]
    B, H, W, C = o["x"].shape
    Co, cpg = o["w"].shape[0], C // dg
    Ho, Wo = out_size(H, W, k, s, p, d)
    n, total = Ho * Wo, B * Ho * Wo
    mag = ref["mag"]
    if path == "mfma":
        ncg, tree = (Co // 2 + 1 if bwd_dispatch(C, Co, dg, groups)[4] == 2 else Co), math.log2(cpg // 8)
        c = dict(gmask=ncg + 11 + 8 + tree, goff=ncg + 6 + 8 + tree, gx=ncg + 5 + ref["cnt"], gw=11 + min(bwd_split(total)[0], total) + DB_SPLITS + 1,
                 gb=B * -(-n // 256) + 9)
        extra = 0.0
    else:
        ncg, chain = Co // groups, -(-total // 256)
        c = dict(gmask=ncg + 11 + cpg, goff=ncg + 7 + cpg, gx=ncg + 3 + ref["cnt"], gw=chain + 20, gb=chain + 9)
        extra = 2 * U * (max(H, W) + 1) * ref["gx_flat"]
    out = {name: c[name] * U * mag[name] + 2.0 ** -149 for name in BWD_NAMES}          # nothing sampled inside: an exact 0 (the floor keeps 0 / 0 out)
    out["gx"] = out["gx"] + extra
    out["gw"], out["gb"] = out["gw"] + U * abs(init), out["gb"] + U * abs(init)
    return out
