"""The loss kernels (csrc/loss_ops.hip, the pixel losses of csrc/train_ops.hip), Adam and the grad scaler restated in plain torch for
fp64 operands: the references of test_gpu_loss_update_edges.py.  Each is written from the operation's definition (the torch
expression the reference model evaluates, the published SSIM / Adam formulas, ATen's scaler update), not from the kernels' loops,
and test_loss_fp64_host.py checks every one against an independent CPU reference -- fp64 autograd, torch.optim.Adam,
torch._amp_update_scale_, the reference's own MS-SSIM vectors -- so that the GPU test's reference is not a copy of the code under
test.  Images keep the kernels' layouts (NHWC; the ground truth of the pixel losses NCHW).  The second half builds the INPUTS the
host and the GPU file share (planted specials, tie patterns, the SSIM families, the scaler table), so that the conditions the host
file asserts about them hold for what the GPU sees.  A plain module like tolerances.py."""
import math

import numpy as np
import torch

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ---- clamp to [0, 1] with NaN -> 0 -----------------------------------------------------------------------------------------------
def clamp01(x):
    return torch.where(torch.isnan(x), torch.zeros_like(x), x.clamp(0.0, 1.0))


def clamp01_pass(x):
    """where d clamp01 / dx = 1: the CLOSED interval (torch.clamp's backward); a NaN was overwritten, its gradient is 0"""
    return (x >= 0.0) & (x <= 1.0)


def clamp01_backward(x, g):
    return torch.where(clamp01_pass(x), g, torch.zeros_like(g))


# ---- pixel losses: rec NHWC, gt NCHW ---------------------------------------------------------------------------------------------
def l1_clamp(rec, gt):
    """mean over ALL elements of |clamp01(rec) - gt| with the NaN positions of rec masked to 0.
    -> (terms [B, H, W, C], loss, sign of the gradient in {-1, 0, 1}): gradient = sign / n"""
    t = gt.permute(0, 2, 3, 1)
    ok = ~torch.isnan(rec)
    d = torch.where(ok, clamp01(rec) - t, torch.zeros_like(rec))
    sign = torch.where(clamp01_pass(rec), torch.sign(d), torch.zeros_like(d))
    return d.abs(), d.abs().sum() / rec.numel(), sign


def l1_plain(rec, gt):
    """mean |rec - gt|; a NaN goes through to the loss and to its own gradient.  -> (terms, loss, sign): gradient = sign / n"""
    d = rec - gt.permute(0, 2, 3, 1)
    return d.abs(), d.abs().sum() / rec.numel(), torch.where(torch.isnan(d), d, torch.sign(d))          # torch.sign(NaN) is 0


def sigmoid(x):
    return torch.sigmoid(x)


# ---- 2x2 pools on NHWC -----------------------------------------------------------------------------------------------------------
def _windows(x):
    """[B, H, W, C] -> [B, H//2, W//2, C, 4]: the four values of each 2x2 window in scan order (0,0) (0,1) (1,0) (1,1)"""
    B, H, W, C = x.shape
    x = x[:, :H // 2 * 2, :W // 2 * 2]
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], -1)


def avgpool2(x):
    return _windows(x).sum(-1) * 0.25


def maxpool2(x):
    return _windows(x).amax(-1)


def maxpool2_first(x):
    """[B, OH, OW, C, 4] bool: the FIRST position in scan order that holds the window's maximum (where its gradient goes)"""
    w = _windows(x)
    is_max = w == w.amax(-1, keepdim=True)
    return is_max & (is_max.cumsum(-1) == 1)


def maxpool2_backward(x, g):
    """g [B, OH, OW, C] -> gx like x: g at the first maximum of each window, 0 elsewhere and in an odd last row / column"""
    B, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    r = torch.where(maxpool2_first(x), g.unsqueeze(-1), torch.zeros_like(g).unsqueeze(-1))          # +0, not 0 * g
    gx = torch.zeros_like(x)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gx[:, dy:2 * OH:2, dx:2 * OW:2] = r[..., k]
    return gx


def mse(a, b):
    return ((a - b) ** 2).sum() / a.numel()


def mse_backward(a, b, g):
    return 2.0 * (a - b) / a.numel() * g


# ---- SSIM, one level -------------------------------------------------------------------------------------------------------------
def window2d(w1):
    """the 2-D window: the outer product of the 1-D one"""
    w1 = torch.as_tensor(w1, dtype=torch.float64)
    return w1[:, None] * w1[None, :]


def windowed(img, w1):
    """sum over the window of w[dy][dx] img[oy + dy][ox + dx] at the VALID positions: [B, H, W, C] -> [B, OH, OW, C]"""
    w2 = window2d(w1).to(img.device)
    ws = w2.shape[0]
    B, H, W, C = img.shape
    OH, OW = H - ws + 1, W - ws + 1
    out = torch.zeros(B, OH, OW, C, dtype=img.dtype, device=img.device)
    for dy in range(ws):
        for dx in range(ws):
            out += w2[dy, dx] * img[:, dy:dy + OH, dx:dx + OW]
    return out


def windowed_adjoint(m, w1, H, W):
    """the adjoint of windowed(): [B, OH, OW, C] -> [B, H, W, C], out[p] = sum over o of w[p - o] m[o]"""
    w2 = window2d(w1).to(m.device)
    ws = w2.shape[0]
    B, OH, OW, C = m.shape
    out = torch.zeros(B, H, W, C, dtype=m.dtype, device=m.device)
    for dy in range(ws):
        for dx in range(ws):
            out[:, dy:dy + OH, dx:dx + OW] += w2[dy, dx] * m
    return out


def ssim_moments(x, y, w1):
    """-> [B, OH, OW, C, 5]: mu1, mu2, E[xx], E[yy], E[xy]"""
    return torch.stack([windowed(x, w1), windowed(y, w1), windowed(x * x, w1), windowed(y * y, w1), windowed(x * y, w1)], -1)


def ssim_maps(mom, C1, C2):
    """-> (cs map, ssim map) = (v1 / v2, lum * cs), v1 = 2 sigma12 + C2, v2 = sigma1^2 + sigma2^2 + C2, lum = (2 mu1 mu2 + C1) /
    (mu1^2 + mu2^2 + C1)"""
    m1, m2, e11, e22, e12 = mom.unbind(-1)
    v1 = 2.0 * (e12 - m1 * m2) + C2
    v2 = (e11 - m1 * m1) + (e22 - m2 * m2) + C2
    cs = v1 / v2
    return cs, (2.0 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs


def ssim_forward(x, y, w1, C1, C2):
    """-> (moments, mean ssim map, mean cs map)"""
    mom = ssim_moments(x, y, w1)
    cs, ss = ssim_maps(mom, C1, C2)
    return mom, ss.mean(), cs.mean()


def ssim_adjoints(mom, C1, C2, g_sim, g_cs):
    """d/d mu1, d/d E[xx], d/d E[xy] of (g_sim ssim + g_cs cs) / n per output pixel, n = the number of output pixels:
    [B, OH, OW, C, 3].  With F = cs (alpha lum + beta):
        d cs / d E[xy] = 2 / v2,  d cs / d E[xx] = -v1 / v2^2,  d cs / d mu1 = (-2 mu2 v2 + 2 mu1 v1) / v2^2,
        d lum / d mu1 = (2 mu2 a2 - 2 mu1 a1) / a2^2"""
    m1, m2, e11, e22, e12 = mom.unbind(-1)
    n = m1.numel()
    alpha, beta = g_sim / n, g_cs / n
    v1 = 2.0 * (e12 - m1 * m2) + C2
    v2 = (e11 - m1 * m1) + (e22 - m2 * m2) + C2
    a1, a2 = 2.0 * m1 * m2 + C1, m1 * m1 + m2 * m2 + C1
    cs, lum = v1 / v2, a1 / a2
    k = alpha * lum + beta
    d_m1 = k * (-2.0 * m2 * v2 + 2.0 * m1 * v1) / (v2 * v2) + alpha * cs * (2.0 * m2 * a2 - 2.0 * m1 * a1) / (a2 * a2)
    return torch.stack([d_m1, k * (-v1) / (v2 * v2), k * 2.0 / v2], -1)


def ssim_backward(x, y, adj, w1, g_next=None):
    """gx = W^T a0 + 2 x W^T a1 + y W^T a2 (mu1 = W x, E[xx] = W x^2, E[xy] = W xy), plus the gradient of the next, 2x2-average-
    pooled level: 0.25 g_next[py >> 1][px >> 1] wherever that pooled pixel exists"""
    B, H, W, C = x.shape
    a0, a1, a2 = (windowed_adjoint(adj[..., k], w1, H, W) for k in range(3))
    gx = a0 + 2.0 * x * a1 + y * a2
    if g_next is not None:
        nH, nW = H // 2, W // 2
        gx[:, :2 * nH, :2 * nW] += 0.25 * g_next.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return gx


def msssim_chain(x, y, windows, C1, C2, normalize):
    """MS-SSIM and d / dx from the per-level restatements above: five levels, 2x2 average pools in between, the combination
    prod_{l<4} (cs_l^w_l * sim_4^w_4) of the reference's msssim(); -> (value, gx)"""
    xs, ys, moms = [x], [y], []
    sims, css = [], []
    for lv in range(5):
        mom, s, c = ssim_forward(xs[-1], ys[-1], windows[lv], C1, C2)
        moms.append(mom)
        sims.append(s)
        css.append(c)
        if lv < 4:
            xs.append(avgpool2(xs[-1]))
            ys.append(avgpool2(ys[-1]))
    sims = torch.stack(sims).detach().requires_grad_(True)
    css = torch.stack(css).detach().requires_grad_(True)
    w = torch.tensor(MSSSIM_WEIGHTS, dtype=torch.float64, device=x.device)
    s2, c2 = ((sims + 1) / 2, (css + 1) / 2) if normalize else (sims, css)
    val = torch.prod((c2 ** w)[:-1] * (s2 ** w)[-1])
    g_sim, g_cs = torch.autograd.grad(val, (sims, css))
    g_next = None
    for lv in range(4, -1, -1):
        adj = ssim_adjoints(moms[lv], C1, C2, g_sim[lv], g_cs[lv])
        g_next = ssim_backward(xs[lv], ys[lv], adj, windows[lv], g_next)
    return val.detach(), g_next


def gaussian_window(ws, sigma=1.5):
    """the reference's 1-D window (pytorch_msssim gaussian()): normalised in float32; returned as the doubles of those floats"""
    g = torch.tensor([math.exp(-(i - ws // 2) ** 2 / float(2 * sigma ** 2)) for i in range(ws)], dtype=torch.float32)
    return tuple((g / g.sum()).tolist())


# ---- Adam and the grad scaler ----------------------------------------------------------------------------------------------------
def adam_bias(beta1, beta2, step):
    """what adam_prepare leaves in state3[0:2]: (1 - beta1^t, sqrt(1 - beta2^t))"""
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def adam_step(w, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, loss_scale=None, lr_mul=1.0):
    """torch.optim.Adam's step (L2 weight decay added to the gradient, eps added AFTER the division by sqrt(bias_correction2)) on a
    gradient that is first multiplied by grad_scale and divided by the loss scale; -> (w, m, v)"""
    bc1, bc2s = adam_bias(beta1, beta2, step)
    gi = g * (grad_scale / loss_scale if loss_scale is not None else grad_scale) + weight_decay * w
    m = beta1 * m + (1.0 - beta1) * gi
    v = beta2 * v + (1.0 - beta2) * gi * gi
    return w - (lr * lr_mul / bc1) * (m / (v.sqrt() / bc2s + eps)), m, v


def f32_bits(v):
    """the bit pattern of v as an fp32, an int in [0, 2^32)"""
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def nonfinite_bits(bits):
    """inf or NaN: the exponent field of the fp32 pattern is all ones"""
    return (int(bits) & 0x7f800000) == 0x7f800000


def scaler_update(scale, tracker, found, growth, backoff, interval):
    """ATen's _amp_update_scale_ in fp32: a step that found inf / NaN (any non-zero flag) backs the scale off and resets the
    tracker; otherwise the tracker counts, and when it REACHES the interval the scale grows -- unless the grown scale is not
    finite, then it is kept -- and the tracker resets either way.  -> (scale as np.float32, tracker)"""
    s = np.float32(scale)
    with np.errstate(over="ignore", under="ignore"):
        if found != 0:
            return s * np.float32(backoff), 0
        t = tracker + 1
        if t != interval:
            return s, t
        ns = s * np.float32(growth)
    return (s if nonfinite_bits(f32_bits(ns)) else ns), 0


# (scale, tracker, found, growth, backoff, interval)
SCALER_TABLE = (
    (65536.0, 1999, 0, 2.0, 0.5, 2000),          # growth at tracker == interval - 1
    (65536.0, 1998, 0, 2.0, 0.5, 2000),          # one short of it: the tracker counts
    (1024.0, 0, 0, 2.0, 0.5, 1),                 # interval 1: grows every clean step
    (1024.0, 0, 0, 1.5, 0.25, 1),
    (1024.0, 5, 0, 2.0, 0.5, 3),                 # tracker >= interval (a checkpoint with a larger count): no growth, keeps counting
    (1024.0, 3, 0, 2.0, 0.5, 3),
    (1024.0, 7, 1, 2.0, 0.5, 2000),              # found, tracker > 0
    (1024.0, 7, 2, 2.0, 0.5, 2000),
    (1024.0, 7, -1, 2.0, 0.5, 2000),
    (1024.0, 1999, 1, 2.0, 0.25, 2000),          # found wins over a due growth
    (2.0 ** -126, 3, 1, 2.0, 0.5, 2000),         # backoff into the subnormals
    (2.0 ** -148, 3, 1, 2.0, 0.25, 2000),        # ... to the smallest one's half-way: 2^-150 ties to even, 0
    (2.0 ** -149, 3, 1, 2.0, 0.5, 2000),         # ... to 0
    (0.0, 3, 1, 2.0, 0.5, 2000),
    (3e38, 1, 0, 2.0, 0.5, 2),                   # the grown scale is inf: kept, tracker reset
    (2.0 ** 127, 1999, 0, 2.0, 0.5, 2000),
    (2.0 ** 127, 0, 0, 1.5, 0.5, 1),             # 1.5 x 2^127 is finite: grows
    (2.0 ** 126, 0, 0, 2.0, 0.5, 1),             # the last growth that fits
)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
F32_TINY = 2.0 ** -149
CLAMP_SPECIALS = (-math.inf, -1.0, -3 * F32_TINY, -0.0, 0.0, F32_TINY, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, math.inf,
                  math.nan, -math.nan)
L1_SPECIALS = ("zero", "negzero", "one", "below", "above", "equal", "pinf", "ninf", "nan")
L1_SHAPES = ((1, 1, 1, 1), (2, 5, 7, 3), (3, 9, 13, 3), (2, 3, 5, 4), (1, 419, 419, 3))


def neg_nan32():
    return torch.tensor([-0x400000], dtype=torch.int32).view(torch.float32)          # 0xffc00000: a NaN with the sign bit set


def clamp_inputs(n, seed):
    """fp32 [n]: N(0.5, 1) with CLAMP_SPECIALS planted from the front (as many as fit), the negative NaN with its sign bit"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) + 0.5
    k = min(n, len(CLAMP_SPECIALS))
    x[:k] = torch.tensor(CLAMP_SPECIALS[:k], dtype=torch.float32)
    if n >= len(CLAMP_SPECIALS):
        x[len(CLAMP_SPECIALS) - 1] = neg_nan32()[0]
    return x


def l1_plant(rec, gt, b, flat_index, name):
    """plant one special at element `flat_index` of sample b of rec (NHWC); "equal" copies gt's value (inside the range)"""
    B, H, W, C = rec.shape
    c, px, py = flat_index % C, flat_index // C % W, flat_index // (C * W)
    v = {"zero": 0.0, "negzero": -0.0, "one": 1.0, "below": -F32_TINY, "above": 1.0 + 2.0 ** -23, "pinf": math.inf,
         "ninf": -math.inf, "nan": math.nan, "equal": float(gt[b, c, py, px])}[name]
    rec[b, py, px, c] = v


def l1_inputs(shape, seed, specials=L1_SPECIALS):
    """-> (rec NHWC fp32, gt NCHW fp32): gt uniform in (0, 1), rec = gt + 0.3 N(0, 1) (about a fifth outside the range), every
    special of `specials` planted once per sample, spread over the sample"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, C, H, W, generator=g) * 0.98 + 0.01
    rec = gt.permute(0, 2, 3, 1).contiguous() + 0.3 * torch.randn(B, H, W, C, generator=g)
    per = H * W * C
    if per >= len(specials):
        for b in range(B):
            for k, name in enumerate(specials):
                l1_plant(rec, gt, b, (k * per) // len(specials) + b, name)          # + b: another block lane per sample
    return rec, gt


def l1_has(rec, gt, b, name):
    """does sample b of rec hold the planted special?"""
    r, t = rec[b], gt[b].permute(1, 2, 0)
    bits = r.contiguous().view(torch.int32)
    return bool({"zero": bits == 0, "negzero": bits == -2 ** 31, "one": r == 1.0, "below": r == -F32_TINY,
                 "above": r == 1.0 + 2.0 ** -23, "pinf": r == math.inf, "ninf": r == -math.inf, "nan": torch.isnan(r),
                 "equal": (r == t) & (r > 0) & (r < 1)}[name].any())


MAXPOOL_SHAPES = ((1, 2, 2, 1), (1, 3, 2, 8), (2, 5, 7, 3), (1, 6, 4, 64))
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def maxpool_inputs(shape, big, seed):
    """fp32 [B, H, W, C] drawn from {-2, -1, -0.0, 0.0, 1, 2, +-inf, big} (big: the largest finite value of the 16-bit format).  In two
    of every three windows the maximum is then copied onto one of the six position pairs in turn, so that it ties; the others keep
    whatever ties the draw gave them (-0.0 against 0.0 among them)."""
    B, H, W, C = shape
    vals = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, math.inf, -math.inf, big])
    g = torch.Generator().manual_seed(seed)
    x = vals[torch.randint(0, len(vals), (B, H, W, C), generator=g)]
    OH, OW = H // 2, W // 2
    k = 0
    for b in range(B):
        for oy in range(OH):
            for ox in range(OW):
                for c in range(C):
                    if k % 3 != 2:
                        win = x[b, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2, c]
                        top = win.max()
                        for p in PAIRS[(k // 3 * 2 + k % 3) % 6]:
                            win[p // 2, p % 2] = top
                    k += 1
    return x


SSIM_SHAPES = ((1, 11, 11, 3, 11), (2, 12, 17, 3, 11), (1, 5, 7, 3, 5), (1, 3, 3, 1, 3), (1, 1, 4, 2, 1), (1, 158, 158, 3, 11))
SSIM_FAMILIES = ("random", "bright1e-1", "bright1e-2", "bright1e-3", "flat0", "flat1", "flat.25/.75")


def ssim_inputs(shape, family, seed):
    """-> (x, y) fp32 NHWC in [0, 1].  random: y uniform, x = clamp(y + 0.2 noise); bright: 0.98 + c noise (low contrast at a high
    mean, clamped); flat: constant images"""
    B, H, W, C = shape[:4]
    g = torch.Generator().manual_seed(seed)
    if family == "random":
        y = torch.rand(B, H, W, C, generator=g)
        return (y + 0.2 * torch.randn(B, H, W, C, generator=g)).clamp(0, 1), y
    if family.startswith("bright"):
        c = float(family[6:])
        return tuple((0.98 + c * torch.randn(B, H, W, C, generator=g)).clamp(0, 1) for _ in range(2))
    a, b = {"flat0": (0.0, 0.0), "flat1": (1.0, 1.0), "flat.25/.75": (0.25, 0.75)}[family]
    return torch.full((B, H, W, C), a), torch.full((B, H, W, C), b)


def window_spread(img, ws):
    """the weighted second moment of every window about the window's own first pixel, [B, OH, OW, C]: exactly 0 iff the window is
    constant (E[xx] - mu^2 of a constant c is c^2 sum(w) (1 - sum(w)): 0 only for a window that sums to exactly 1)"""
    B, H, W, C = img.shape
    OH, OW = H - ws + 1, W - ws + 1
    w2 = window2d(gaussian_window(ws))
    out = torch.zeros(B, OH, OW, C, dtype=torch.float64)
    for dy in range(ws):
        for dx in range(ws):
            out += w2[dy, dx] * (img[:, dy:dy + OH, dx:dx + OW].double() - img[:, :OH, :OW].double()) ** 2
    return out
