"""The LPIPS head (csrc/lpips_ops.hip) and the image affine map in fp64, with the error bounds the per-element tests hold the kernels to.
NHWC, as the kernels read it.  A plain module like backward_fp64.py.

    na = sqrt(sum_c a_c^2)   nb = sqrt(sum_c b_c^2)   ah = a / (na + eps)   bh = b / (nb + eps)
    out[i] = (1 / HW) sum_pixels sum_c w_c (ah_c - bh_c)^2
    e_c = 2 w_c (ah_c - bh_c)    s = sum_c e_c a_c
    da_c = (g[i] / HW) (e_c / (na + eps) - a_c s / (na (na + eps)^2));   a pixel of `a` that is all zero: da = 0   (autograd: NaN)

Slack, counted from the kernel's expression (U = 2^-24, one fp32 rounding; a division or a square root is counted as a whole ulp, 2 U,
as tests/test_gpu_disc_kernels.py counts what is not specified to round to nearest).  Inputs are 16-bit values: a_c^2 is exact in fp32.
    q = sum_c a_c^2      8 channels in a lane then log2(C / 8) <= 6 shuffle steps: <= 13 additions of positive terms     13 U   (14 taken)
    na = sqrt(q)         14 / 2 + 2                                                                                       9 U
    na + eps             + 1                                                                                             10 U
    ia = 1 / (na + eps)  + 2                                                                                             12 U
    ah_c = a_c ia        + 1                                                                                             13 U
    d_c = ah_c - bh_c    |err| <= 13 U (|ah_c| + |bh_c|) + U |d_c| <= 14 U m_c,   m_c = |ah_c| + |bh_c|
  forward
    t_c = (w_c d_c) d_c  |err| <= |w_c| (2 |d_c| + 14 U m_c) 14 U m_c + 2 U |w_c| d_c^2
    sum over c           + 14 U sum |t_c|            together <= 44 U sum_c |w_c| (|d_c| + 14 U m_c) m_c    =: err_pixel  (|d_c| <= m_c)
    sum over pixels      a group's pixels in order, the <= 32 groups of a workgroup, the workgroups, the division by HW: a chain of at most
                         HW + 35 roundings on terms of magnitude sum_c |w_c| d_c^2
  backward
    e_c = 2 w_c d_c      |err| <= 2 |w_c| 14 U m_c + U |e_c| <= 30 U |w_c| m_c                                   (|e_c| <= 2 |w_c| m_c)
    s = sum_c e_c a_c    |err| <= sum |a_c| err(e_c) + 15 U sum |e_c a_c| <= 60 U M,   M = sum_c |w_c a_c| m_c      (|s| <= 2 M)
    t1_c = e_c ia        |err| <= ia err(e_c) + 13 U |e_c| ia <= 56 U ia |w_c| m_c
    den = na ((na + eps)(na + eps))      9 + 10 + 10 + 2 = 31 U;   k = s / den   + 2
    t2_c = a_c k         |err| <= |a_c| / den (err(s) + 34 U |s|) <= 128 U |a_c| M / den
    gs = g / HW (2 U),  da_c = gs (t1_c - t2_c) (1 U for the difference, 1 U for the product): 4 U |gs| (|t1_c| + |t2_c|)
    together             |gs| U (64 ia |w_c| m_c + 136 |a_c| M / den)
A pixel with one non-zero channel has t1_c = t2_c up to eps / na: the exact gradient there is ~0 and the slack (relative to t1, t2, not to
their difference) is what bounds it."""
import torch

U = 2.0 ** -24


def head64(a, b, w, g=None, eps=1e-10):
    """a, b: [B, H, W, C] (any float dtype; read as exact values); w: [C]; g: [B] or None; eps: the fp32 value the kernel receives.
    -> dict(out [B], out_tol [B], da [B, H, W, C], da_slack) in fp64 (da*: only with g)."""
    a, b, w = a.double(), b.double(), w.double().reshape(-1)
    B, H, W, C = a.shape
    HW = H * W
    na, nb = a.pow(2).sum(-1, keepdim=True).sqrt(), b.pow(2).sum(-1, keepdim=True).sqrt()
    ia, ib = 1.0 / (na + eps), 1.0 / (nb + eps)
    ah, bh = a * ia, b * ib
    d, m = ah - bh, ah.abs() + bh.abs()
    t = w * d * d
    res = {"out": t.sum(dim=(1, 2, 3)) / HW}
    err_pixel = 44 * U * (w.abs() * (d.abs() + 14 * U * m) * m).sum(dim=(1, 2, 3))
    res["out_tol"] = (err_pixel + (HW + 35) * U * t.abs().sum(dim=(1, 2, 3))) / HW + 1e-300
    if g is not None:
        gs = (g.double() / HW).view(B, 1, 1, 1)
        e = 2 * w * d
        s = (e * a).sum(-1, keepdim=True)
        zero = na == 0
        den = torch.where(zero, torch.ones_like(na), na * (na + eps) ** 2)
        da = gs * (e * ia - a * s / den)
        res["da"] = torch.where(zero, torch.zeros_like(da), da)
        M = (w.abs() * a.abs() * m).sum(-1, keepdim=True)
        slack = gs.abs() * U * (64 * ia * w.abs() * m + 136 * a.abs() * M / den)
        res["da_slack"] = torch.where(zero, torch.zeros_like(slack), slack)
    return res


def head_autograd64(a, b, w, g, eps=1e-10):
    """(out [B], d (sum_i g_i out_i) / da) by fp64 autograd of the published forward, restated on NHWC: NaN at an all-zero pixel of a."""
    a = a.double().clone().requires_grad_(True)
    b, w = b.double(), w.double().reshape(-1)
    ah = a / (torch.sqrt(torch.sum(a ** 2, dim=-1, keepdim=True)) + eps)
    bh = b / (torch.sqrt(torch.sum(b ** 2, dim=-1, keepdim=True)) + eps)
    out = (w * (ah - bh) ** 2).sum(-1).mean(dim=(1, 2))
    (da,) = torch.autograd.grad((out * g.double()).sum(), a)
    return out.detach(), da


def affine64(x, mul, add=None):
    """x * mul[c] (+ add[c]) on [..., C] with mul, add the fp32 values the kernel reads; one fused rounding: tol = U |exact|."""
    y = x.double() * mul.double()
    if add is not None:
        y = y + add.double()
    return y, U * y.abs() + 1e-300
