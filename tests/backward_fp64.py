"""The adjoints of the streaming kernels restated in plain torch, for fp64 operands: the references of test_gpu_backward_edges.py.
Each is written from the mathematics in the header comments of csrc/flow_bwd.hip and csrc/train_ops.hip (the forward operation and
its derivative), not from the kernels' loops, and test_backward_fp64_host.py checks every one against fp64 AUTOGRAD of the forward
operation -- so that the GPU test's reference is not a copy of the code under test.  Tensors keep the kernels' layouts (channels
last); where a kernel leaves per-block partial sums, the restatement returns the per-pixel TERMS of the sum and the test adds
them over the pixels it expects a block to own.  A plain module like tolerances.py."""
import torch
import torch.nn.functional as F

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]          # tap t of a 3x3 filter reads the pixel at offset (dy, dx)


def per_sample(v, like):
    """[B] -> [B, 1, ...] broadcastable against `like` ([B, ...])"""
    return v.reshape([-1] + [1] * (like.dim() - 1))


# ---- Gaussian log-density: logp[b] = sum -0.5 ((z - mean)^2 + log 2 pi) ----------------------------------------------------------
def nll_backward(z, mean, g_logp):
    """-> (gz, gmean): d logp / d mean = z - mean, d logp / d z = -(z - mean), times the sample's g_logp"""
    g = per_sample(g_logp, z) * (z - mean)
    return -g, g


# ---- affine coupling: scale = sigmoid(raw + 2) + eps ------------------------------------------------------------------------------
def coupling_scale(raw, eps):
    sg = torch.sigmoid(raw + 2.0)
    return sg, sg + eps


def _coupling_adjoint(g, pre, shift, raw, gl, eps):
    """out = (pre + shift) * scale and logdet += log scale  ->  (g_pre = g_shift, g_raw):
    d out / d pre = d out / d shift = scale;  d / d raw = (g (pre + shift) + gl / scale) scale'(raw), scale' = sg (1 - sg)"""
    sg, s = coupling_scale(raw, eps)
    return g * s, (g * (pre + shift) + gl / s) * sg * (1.0 - sg)


def post_backward(gz, z_pre, h4, g_logdet, eps):
    """z''[0] = z'[0]; z''[1 + c] = (z'[1 + c] + h4[2c]) * scale(h4[2c + 1]); logdet[b] += sum log scale.
    gz, z_pre [B, ..., 3]; h4 [B, ..., 4] -> (gz' [B, ..., 3], gh4 [B, ..., 4])"""
    gl = per_sample(g_logdet, gz[..., 0])
    cols, gh = [gz[..., 0]], []
    for c in range(2):
        gp, gr = _coupling_adjoint(gz[..., 1 + c], z_pre[..., 1 + c], h4[..., 2 * c], h4[..., 2 * c + 1], gl, eps)
        cols.append(gp)
        gh += [gp, gr]
    return torch.stack(cols, -1), torch.stack(gh, -1)


def pre_backward(gz, z_in, f6, g_logdet, M, t, eps):
    """y = M z + t; z'[i] = (y[i] + f6[2i]) * scale(f6[2i + 1]); logdet[b] += sum log scale.
    -> (gz_in = M^T gy, gf6 [B, ..., 6], gy [B, ..., 3]); gM = sum over pixels of gy (x) z, gt = sum of gy: see pre_terms"""
    gl = per_sample(g_logdet, gz[..., 0])
    y = z_in @ M.t() + t
    gy, gf = [], []
    for i in range(3):
        gp, gr = _coupling_adjoint(gz[..., i], y[..., i], f6[..., 2 * i], f6[..., 2 * i + 1], gl, eps)
        gy.append(gp)
        gf += [gp, gr]
    gy = torch.stack(gy, -1)
    return gy @ M, torch.stack(gf, -1), gy


def pre_terms(gy, z_in):
    """per-pixel terms of (gM row-major, gt): [B, ..., 12]"""
    return torch.cat([(gy.unsqueeze(-1) * z_in.unsqueeze(-2)).flatten(-2), gy], -1)


# ---- h1 = conv3x3(z0 -> 64 channels, pad 1) ---------------------------------------------------------------------------------------
def _shifted(img, dy, dx):
    """[B, H, W, ...] -> the image read at offset (dy, dx): out[y, x] = img[y + dy, x + dx], zero outside"""
    B, H, W = img.shape[:3]
    out = torch.zeros_like(img)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[:, ys, xs] = img[:, yd, xd]
    return out


def h1_backward_data(g, wz):
    """g [B, H, W, 64], wz [64, 9] -> the gradient of z0 [B, H, W]: z0[p] fed h1[p - d_t] through tap t"""
    return sum(_shifted(g, -dy, -dx) @ wz[:, t] for t, (dy, dx) in enumerate(TAPS))


def h1_filter_terms(g, z0):
    """per-pixel terms of the filter gradient [B, H, W, 64, 9]: h1[p] saw z0[p + d_t] through tap t"""
    zt = torch.stack([_shifted(z0, dy, dx) for dy, dx in TAPS], -1)
    return g.unsqueeze(-1) * zt.unsqueeze(-2)


# ---- GroupNorm(32) [+ swish] ------------------------------------------------------------------------------------------------------
def swish_grad(u):
    s = torch.sigmoid(u)
    return s * (1.0 + u * (1.0 - s))


def groupnorm_backward(x, dy, gamma, beta, mean, rstd, swish):
    """x, dy [B, HW, C]; mean, rstd [B, 32] (of the group's HW * C / 32 values).  u = xh gamma + beta, xh = (x - mean) rstd,
    y = swish(u) or u.  du = dy swish'(u);  s1 = sum_p du, s2 = sum_p du xh  (dbeta, dgamma = their sums over the images);
    dx = rstd (du gamma - mean_group(du gamma) - xh mean_group(du gamma xh))  -> (dx, s1 [B, C], s2 [B, C], xh, du)"""
    B, HW, C = x.shape
    cpg = C // 32
    mu, r = (v.repeat_interleave(cpg, 1).unsqueeze(1) for v in (mean, rstd))
    xh = (x - mu) * r
    du = dy * swish_grad(xh * gamma + beta) if swish else dy
    s1, s2 = du.sum(1), (du * xh).sum(1)
    m = float(HW * cpg)
    a = ((s1 * gamma).view(B, 32, cpg).sum(2) / m).repeat_interleave(cpg, 1).unsqueeze(1)
    q = ((s2 * gamma).view(B, 32, cpg).sum(2) / m).repeat_interleave(cpg, 1).unsqueeze(1)
    return r * (du * gamma - a - xh * q), s1, s2, xh, du


# ---- mix: out = s a + (1 - s) b, s = sigmoid(w) -----------------------------------------------------------------------------------
def mix_backward(g, a, b, w):
    """-> (ga, gb, dw): d out / d w = (a - b) s (1 - s)"""
    s = torch.sigmoid(w)
    return s * g, (1.0 - s) * g, s * (1.0 - s) * (g * (a - b)).sum()


# ---- mean rescale: out = h + xw r, r = sum h / sum xw over the sample (or over the batch) -------------------------------------
def mean_rescale_sums(g, h, xw, whole):
    """[B, n] -> (D = sum g xw, Sh, Sx), each [B] (the batch's totals repeated when `whole`)"""
    D, Sh, Sx = (g * xw).sum(1), h.sum(1), xw.sum(1)
    if whole:
        D, Sh, Sx = (v.sum().expand(g.shape[0]) for v in (D, Sh, Sx))
    return D, Sh, Sx


def mean_rescale_backward(g, h, xw, whole):
    """d out_j / d h_i = delta_ij + xw_j / Sx;  d out_j / d xw_i = delta_ij r - xw_j Sh / Sx^2
    -> (gh = g + D / Sx, gxw = g r - D Sh / Sx^2)"""
    D, Sh, Sx = (v.unsqueeze(1) for v in mean_rescale_sums(g, h, xw, whole))
    return g + D / Sx, g * (Sh / Sx) - D * Sh / (Sx * Sx)


# ---- activations the forward convs fuse: the derivative in terms of the OUTPUT y --------------------------------------------------
def act_backward(g, y, act):
    if act == "relu":
        return torch.where(y > 0, g, torch.zeros_like(g))
    assert act == "sigmoid"
    return g * y * (1.0 - y)


# ---- the forward operations (for autograd; test_backward_fp64_host.py) ------------------------------------------------------------
def h1_forward(z0, wz):
    """z0 [B, H, W], wz [64, 9] -> [B, H, W, 64]"""
    return F.conv2d(z0.unsqueeze(1), wz.view(64, 1, 3, 3), padding=1).permute(0, 2, 3, 1)
